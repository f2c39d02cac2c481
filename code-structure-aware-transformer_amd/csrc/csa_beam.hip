// Beam search on top of the KV-cached, device-stepped decode step (csa_decode.hip): the two kernels of one beam step
// that are neither a GEMM nor the attention. Rows are R = B * W hypotheses, row r = b * W + w of AST b, W <= 8.
//
//   k_beam_row_topk  per row of the (R, V) last-position logits: lse = log sum exp (fp32, online) and the row's W
//                    largest logits with their indices, descending, lowest index first among equals. Within a row
//                    log p = z - lse is monotone in z and an AST takes at most W candidates from one row, so the
//                    row's top W are all the selection can need.
//   k_beam_select    per AST: merges the W x W candidates (score = cum[r] + (z - lse[r]); a finished row offers only
//                    (cum[r], PAD)), ordered by score descending, then parent row, then token, and rewrites the
//                    hypotheses' state in place: cum, fin, the token buffer, the PAD key mask and the ancestry table
//                    that k_decode_attn<BEAM> follows into the K/V cache (anc[r, j] = the cache row holding key j of
//                    hypothesis r). The cache itself is never moved.
//
// Both read the step t from the decode step's 4-byte device counter (one captured graph serves every step); a t
// outside its range stores nothing and reads no row. fp32, wave64; every reduction has a fixed order (no atomics), so
// results repeat bitwise; nothing allocates or syncs.
//
// k_beam_row_topk: one workgroup of 256 threads per row, one pass with 16-byte loads. A thread keeps the online
// (max, sum exp) of its columns and their sorted top-W list in registers (insertion from the tail, compile-time
// indices only); the workgroup then takes W rounds of an arg-max over the threads' list heads, the winner's owner
// advancing its head. -inf entries carry their real index, so an all -inf row gives indices 0 .. W-1.
//
// k_beam_select: one workgroup per AST. Each of the W * W candidates counts the candidates that come before it (its
// rank; the order is total, so ranks are distinct) and the first W take child slots 0 .. W-1. All W parent rows
// (columns 0 .. t of tokens and pad, 0 .. t-1 of anc) are staged in LDS, the workgroup crosses a barrier and only then
// writes: an AST's rows belong to one workgroup, so two children of one parent and a swap of two rows come out right
// in place. LDS: 13 W T bytes at the limits W = 8, T = 256 (csa_beam_supported).
#include "csa_common.hpp"
#include "csa_row_select.hpp"
#include "../../include/csa_hip.h"

#include <math.h>

using namespace csa;

namespace {

constexpr int BEAM_THREADS = 256;
constexpr int BEAM_MAX_W = 8;
constexpr int BEAM_MAX_T = 256;

template <int WM>
__global__ __launch_bounds__(BEAM_THREADS) void k_beam_row_topk(const float* __restrict__ z, int64_t V, int W,
                                                                float* __restrict__ lse, float* __restrict__ topv,
                                                                int32_t* __restrict__ topi,
                                                                const int32_t* __restrict__ t_dev, int t_end) {
  if (t_dev) {  // one value for the whole grid, before any barrier
    const int t = *t_dev;
    if (t < 0 || t >= t_end) return;
  }
  __shared__ float rm[BEAM_THREADS / 64], rs[BEAM_THREADS / 64];
  __shared__ float wv[BEAM_THREADS / 64];
  __shared__ int wi[BEAM_THREADS / 64];
  const int64_t row = blockIdx.x;
  const float* zr = z + row * V;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  float tv[WM];
  int ti[WM];
#pragma unroll
  for (int k = 0; k < WM; ++k) { tv[k] = -INFINITY; ti[k] = NO_IDX; }
  float m = -INFINITY, s = 0.f;

  const auto take = [&](float v, int i) {
    if (ahead(v, i, tv[WM - 1], ti[WM - 1])) {
      tv[WM - 1] = v;
      ti[WM - 1] = i;
#pragma unroll
      for (int k = WM - 1; k > 0; --k) {
        if (ahead(tv[k], ti[k], tv[k - 1], ti[k - 1])) {
          const float fv = tv[k]; tv[k] = tv[k - 1]; tv[k - 1] = fv;
          const int fi = ti[k]; ti[k] = ti[k - 1]; ti[k - 1] = fi;
        }
      }
    }
  };

  if (V % 4 == 0) {
    // a base that is only 4-byte aligned loads the same four columns one by one: the thread's columns and the order of
    // its sum do not depend on where the logits lie, so neither do the bits of lse
    const bool vec = (((uintptr_t)z) & 15) == 0;
    for (int64_t c = 4 * (int64_t)tid; c < V; c += 4 * BEAM_THREADS) {
      f32x4 q;
      if (vec) q = *reinterpret_cast<const f32x4*>(zr + c);
      else q = f32x4{zr[c], zr[c + 1], zr[c + 2], zr[c + 3]};
      const float mx = fmaxf(fmaxf(q[0], q[1]), fmaxf(q[2], q[3]));
      if (mx > m) {
        s = (m > -INFINITY) ? s * expf(m - mx) : 0.f;
        m = mx;
      }
      if (m > -INFINITY) {
#pragma unroll
        for (int e = 0; e < 4; ++e) s += expf(q[e] - m);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) take(q[e], (int)c + e);
    }
  } else {
    for (int64_t c = tid; c < V; c += BEAM_THREADS) {
      const float q = zr[c];
      if (q > m) {
        s = (m > -INFINITY) ? s * expf(m - q) : 0.f;
        m = q;
      }
      if (m > -INFINITY) s += expf(q - m);
      take(q, (int)c);
    }
  }

  // ---- lse: xor butterfly inside the wave (both partners compute the same sum), then the waves in order ----
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float mo = __shfl_xor(m, o, 64);
    const float so = __shfl_xor(s, o, 64);
    lse_merge(m, s, mo, so);
  }
  if (lane == 0) { rm[wave] = m; rs[wave] = s; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < BEAM_THREADS / 64; ++k) lse_merge(m, s, rm[k], rs[k]);
    lse[row] = (m > -INFINITY) ? m + logf(s) : -INFINITY;
  }

  // ---- W rounds of a workgroup arg-max over the threads' list heads ----
  int head = 0;
  for (int k = 0; k < W; ++k) {
    float cv = -INFINITY;
    int ci = NO_IDX;  // an exhausted list offers nothing
#pragma unroll
    for (int u = 0; u < WM; ++u)
      if (u == head) { cv = tv[u]; ci = ti[u]; }
    float bv = cv;
    int bi = ci;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float vo = __shfl_xor(bv, o, 64);
      const int io = __shfl_xor(bi, o, 64);
      if (ahead(vo, io, bv, bi)) { bv = vo; bi = io; }
    }
    if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
    __syncthreads();
    bv = wv[0];
    bi = wi[0];
#pragma unroll
    for (int x = 1; x < BEAM_THREADS / 64; ++x)
      if (ahead(wv[x], wi[x], bv, bi)) { bv = wv[x]; bi = wi[x]; }
    if (bi != NO_IDX && ci == bi) ++head;  // indices are distinct: exactly one owner
    if (tid == 0) {
      topv[row * W + k] = bv;
      topi[row * W + k] = (bi == NO_IDX) ? k : bi;  // nothing comparable left (NaN): still inside [0, V)
    }
    __syncthreads();  // wv / wi are rewritten by the next round
  }
}

struct SelArgs {
  int W, T;
  const float* topv; const int32_t* topi; const float* lse;
  float* cum; uint8_t* fin;
  int64_t* tok; int64_t tok_s;
  uint8_t* pad; int64_t pad_s;
  int32_t* anc; int64_t anc_s;
  int32_t* parent;
  int64_t eos_id, pad_id;
  const int32_t* t_dev;
};

__global__ __launch_bounds__(BEAM_THREADS) void k_beam_select(const SelArgs a) {
  const int t = *a.t_dev;
  if (t < 0 || t >= a.T - 1) return;  // the whole grid, before any barrier
  constexpr int NC = BEAM_MAX_W * BEAM_MAX_W;
  __shared__ float c_score[NC];
  __shared__ int64_t c_tok[NC];
  __shared__ uint8_t c_valid[NC];
  __shared__ uint8_t p_fin[BEAM_MAX_W];
  __shared__ int s_parent[BEAM_MAX_W];
  __shared__ int64_t s_newtok[BEAM_MAX_W];
  __shared__ float s_score[BEAM_MAX_W];
  __shared__ int64_t r_tok[BEAM_MAX_W * BEAM_MAX_T];
  __shared__ int32_t r_anc[BEAM_MAX_W * BEAM_MAX_T];
  __shared__ uint8_t r_pad[BEAM_MAX_W * BEAM_MAX_T];
  const int W = a.W, T = a.T, tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * W;  // the AST's first row
  const int ncol = t + 1;                      // live columns of a parent row

  // ---- candidates (w, k): row w's k-th best token, or the single (cum, PAD) of a finished row ----
  if (tid < W * W) {
    const int w = tid / W, k = tid - w * W;
    const int64_t r = r0 + w;
    const bool f = a.fin[r] != 0;
    const float c = a.cum[r];
    float sc = c;
    int64_t tk = a.pad_id;
    if (!f) {
      sc = c + (a.topv[r * W + k] - a.lse[r]);
      tk = a.topi[r * W + k];
    }
    if (!(sc > -INFINITY)) sc = -INFINITY;  // -inf (and NaN) loses to any finite score
    c_score[tid] = sc;
    c_tok[tid] = tk;
    c_valid[tid] = (!f || k == 0) ? 1 : 0;
    if (k == 0) p_fin[w] = f ? 1 : 0;
  }
  // ---- the W parent rows into LDS ----
  for (int x = tid; x < W * ncol; x += BEAM_THREADS) {
    const int w = x / ncol, j = x - w * ncol;
    r_tok[w * T + j] = a.tok[(r0 + w) * a.tok_s + j];
    r_pad[w * T + j] = a.pad[(r0 + w) * a.pad_s + j];
    r_anc[w * T + j] = a.anc[(r0 + w) * a.anc_s + j];
  }
  __syncthreads();

  // ---- rank = how many offered candidates come first; at least W are offered and the order is total ----
  if (tid < W * W && c_valid[tid]) {
    const int w = tid / W;
    const float sc = c_score[tid];
    const int64_t tk = c_tok[tid];
    int rank = 0;
    for (int o = 0; o < W * W; ++o) {
      if (o == tid || !c_valid[o]) continue;
      const int wo = o / W;
      const float so = c_score[o];
      if (so > sc || (so == sc && (wo < w || (wo == w && c_tok[o] < tk)))) ++rank;
    }
    if (rank < W) {
      s_parent[rank] = w;
      s_newtok[rank] = tk;
      s_score[rank] = sc;
    }
  }
  __syncthreads();  // every read of the old state is done: write in place

  for (int x = tid; x < W * ncol; x += BEAM_THREADS) {
    const int c = x / ncol, j = x - c * ncol;
    const int p = s_parent[c];
    a.tok[(r0 + c) * a.tok_s + j] = r_tok[p * T + j];
    a.pad[(r0 + c) * a.pad_s + j] = r_pad[p * T + j];
    if (j < t) a.anc[(r0 + c) * a.anc_s + j] = r_anc[p * T + j];
  }
  if (tid < W) {
    const int p = s_parent[tid];
    const int64_t r = r0 + tid, tk = s_newtok[tid];
    a.tok[r * a.tok_s + t + 1] = tk;
    a.pad[r * a.pad_s + t + 1] = (tk == a.pad_id) ? 1 : 0;
    a.anc[r * a.anc_s + t] = (int32_t)(r0 + p);  // key t of the child sits where the parent stored it
    a.cum[r] = s_score[tid];
    a.fin[r] = (p_fin[p] || tk == a.eos_id) ? 1 : 0;
    if (a.parent) a.parent[r] = (int32_t)(r0 + p);
  }
}

}  // namespace

extern "C" {

int csa_beam_supported(int64_t W, int64_t T) {
  return (W >= 1 && W <= BEAM_MAX_W && T >= 2 && T <= BEAM_MAX_T) ? 1 : 0;
}

csa_status csa_beam_row_topk(const float* z, int64_t rows, int64_t V, int64_t W, float* lse, float* topv, int32_t* topi,
                             const int32_t* t_dev, int64_t t_end, void* stream) {
  if (W < 1 || W > BEAM_MAX_W) return fail(CSA_UNSUPPORTED_SHAPE, "csa_beam_row_topk: W must be in [1, 8]");
  if (rows < 0 || rows > 0x7fffffff || V < 1 || V >= 0x7fffffff || t_end < 0 || t_end > 0x7fffffff)
    return fail(CSA_INVALID_ARG, "csa_beam_row_topk: bad rows / V / t_end");
  if (V < W) return fail(CSA_INVALID_ARG, "csa_beam_row_topk: V must be at least W");
  if (!z || !lse || !topv || !topi) return fail(CSA_INVALID_ARG, "csa_beam_row_topk: null pointer");
  if (!aligned(z, 4) || !aligned(lse, 4) || !aligned(topv, 4) || !aligned(topi, 4) || !aligned(t_dev, 4))
    return fail(CSA_INVALID_ARG, "csa_beam_row_topk: misaligned pointer (4 bytes each)");
  if (rows == 0) return CSA_OK;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
#define CSA_TOPK_LAUNCH(WM)                                                                                       \
  hipLaunchKernelGGL(k_beam_row_topk<WM>, dim3((unsigned)rows), dim3(BEAM_THREADS), 0, st, z, V, (int)W, lse, topv, \
                     topi, t_dev, (int)t_end)
  if (W == 1) CSA_TOPK_LAUNCH(1);
  else if (W == 2) CSA_TOPK_LAUNCH(2);
  else if (W <= 4) CSA_TOPK_LAUNCH(4);
  else CSA_TOPK_LAUNCH(8);
#undef CSA_TOPK_LAUNCH
  return launched("csa_beam_row_topk");
}

csa_status csa_beam_select(const csa_beam_select_args* a, void* stream) {
  if (!a) return fail(CSA_INVALID_ARG, "csa_beam_select: null args");
  if (!csa_beam_supported(a->W, a->T))
    return fail(CSA_UNSUPPORTED_SHAPE, "csa_beam_select: W must be in [1, 8] and T in [2, 256]");
  if (a->B < 0 || a->B * a->W > 0x7fffffff || a->tok_stride < a->T || a->pad_stride < a->T || a->anc_stride < a->T)
    return fail(CSA_INVALID_ARG, "csa_beam_select: bad B or a row stride below T");
  if (!a->topv || !a->topi || !a->lse || !a->cum || !a->fin || !a->tokens || !a->pad || !a->anc || !a->t_dev)
    return fail(CSA_INVALID_ARG, "csa_beam_select: null pointer");
  if (!aligned(a->topv, 4) || !aligned(a->topi, 4) || !aligned(a->lse, 4) || !aligned(a->cum, 4) ||
      !aligned(a->tokens, 8) || !aligned(a->anc, 4) || !aligned(a->parent, 4) || !aligned(a->t_dev, 4))
    return fail(CSA_INVALID_ARG, "csa_beam_select: misaligned pointer (tokens 8, the fp32 / int32 arrays 4 bytes)");
  if (a->B == 0) return CSA_OK;
  SelArgs d;
  d.W = (int)a->W; d.T = (int)a->T;
  d.topv = a->topv; d.topi = a->topi; d.lse = a->lse;
  d.cum = a->cum; d.fin = a->fin;
  d.tok = a->tokens; d.tok_s = a->tok_stride;
  d.pad = a->pad; d.pad_s = a->pad_stride;
  d.anc = a->anc; d.anc_s = a->anc_stride;
  d.parent = a->parent;
  d.eos_id = a->eos_id; d.pad_id = a->pad_id;
  d.t_dev = a->t_dev;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  hipLaunchKernelGGL(k_beam_select, dim3((unsigned)a->B), dim3(BEAM_THREADS), 0, st, d);
  return launched("csa_beam_select");
}

}  // extern "C"
