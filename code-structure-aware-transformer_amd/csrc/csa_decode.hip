// Incremental (KV-cached) greedy decoding on gfx950: the two kernels of one decode step that are not a GEMM.
//
//   k_decode_attn   softmax(q K^T * scale + key mask) V for ONE query row per (batch, head): the decoder's
//                   self-attention against its K/V cache (optionally appending this step's key/value row) and
//                   its cross-attention against the projected encoder memory, both through strides.
//   k_argmax_rows   row argmax of the last-position logits, written straight into ys[:, t+1] together with
//                   the next step's PAD key-mask byte.
//
// Device-stepped variants (one captured HIP graph then serves every step of a batch): the step index t is read by
// the kernel from a 4-byte device counter instead of being baked into the launch.
//   k_decode_attn       with DecArgs.t_dev set: append at row *t_dev, t + 1 keys; the grid never depended on the length
//   k_argmax_rows_step  k_argmax_rows writing column *t_dev + 1 of ys / pad and of the per-head (H, B, T) key mask
//   k_decode_embed      LayerNorm(W[ys[b, t]] + pe[t]), the target embedding of position t, on the LayerNorm
//                       forward's row function (csa_ln_row.hpp): bitwise the gather + add + csa_layernorm_fwd
// A counter outside its range makes the launch store nothing and read no row.
//
// Early stop at EOS (one finished flag per row, fin):
//   k_argmax_rows_fin_step  k_argmax_rows_step in which a finished row takes PAD and a row that draws EOS finishes
//   k_decode_advance        ends the step in place of the counter's increment: counts it and, once every row has
//                           finished (or after the last step), parks the counter at -1, the value for which every
//                           step kernel stores nothing, so replays issued after that are harmless
//
// Beam search (csa_decode_attn_beam) is the same kernel with BEAM = true, two uniform changes of addressing only:
//   ancestry  (anc set, self-attention) key / value j < t of row r is read from cache row anc[r, j]: a hypothesis'
//             history stays where its ancestors stored it and no cache row is ever moved; row (r, t) is stored as above;
//   kv_group  (cross-attention) K, V and the mask are read at batch index r / kv_group: the hypotheses of an AST
//             share one memory projection.
// The chunk walk, the online softmax and the P.V order are the ones below, so for a cache that really was gathered
// the two instantiations agree bitwise.
//
// M = 1, so there is no matrix product to feed an MFMA: both kernels are bound by memory latency (a few
// hundred KB to a few tens of MB per launch) and are written for wave64 with 16-byte global loads.
//
// k_decode_attn: one wave per (b, h), DEC_WAVES waves per workgroup. Keys are walked in chunks of 64:
//   scores   lane l owns key 64 c + l and reads its whole row as float4 (q is broadcast from LDS);
//   softmax  online over chunks (running max m, running sum l). A chunk whose 64 keys are all masked while
//            m is still -inf is skipped outright, and the rescale factor of the first live chunk is 0 by
//            construction, so exp(-inf - (-inf)) is never evaluated; tail lanes (key >= len) score -inf and
//            their probability is an exact 0;
//   P.V      the chunk's probabilities sit in LDS; lane l owns the float4 column group l % (hd/4) and the key
//            group l / (hd/4), so a row of V is read by hd/4 adjacent lanes (coalesced). The key groups are
//            summed through LDS in a fixed order.
// Every sum has a fixed order: results are bitwise reproducible.
// A row whose keys are all masked ends with l = 0 and gives 0/0 = NaN (as SDPA does for an all -inf mask).
// Append mode: the wave copies k_new / v_new into cache row t and reads key t from k_new / v_new themselves,
// never from the row it has just stored (no read-after-write through global memory).
#include "csa_common.hpp"
#include "csa_ln_row.hpp"
#include "../../include/csa_hip.h"

#include <math.h>

using namespace csa;

namespace {

constexpr int DEC_WAVES = 4;      // (b, h) pairs per workgroup
constexpr int DEC_MAX_HD = 128;
constexpr int PV_U = 8;           // V rows a lane keeps in flight in the P.V phase
constexpr int ARG_T = 256;

struct DecArgs {
  int BH, H, hd, len, t;  // t < 0: no append
  const int32_t* t_dev;   // device-stepped append: t = *t_dev, len (the capacity here) becomes t + 1
  const float* q; int64_t q_sb, q_sh;
  float* K; int64_t k_sb, k_sh, k_sn;
  float* V; int64_t v_sb, v_sh, v_sn;
  const float* k_new; int64_t kn_sb, kn_sh;
  const float* v_new; int64_t vn_sb, vn_sh;
  const uint8_t* mask; int64_t mask_sb, mask_sh;
  float scale;
  float* out;
  // BEAM only
  const int32_t* anc; int64_t anc_s;  // (B, >= len) cache row of key j of row b, or null
  int kv_group, B;                    // K / V / mask batch index = b / kv_group
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// The cache row that holds key j of this hypothesis, clamped into [0, B): a bad table reads a wrong row, never
// outside the cache.
__device__ __forceinline__ int64_t anc_row(const int32_t* __restrict__ arow, int j, int B) {
  const int r = arow[j];
  return r < 0 ? 0 : (r >= B ? B - 1 : r);
}

template <bool BEAM>
__global__ __launch_bounds__(64 * DEC_WAVES) void k_decode_attn(const DecArgs a) {
  __shared__ f32x4 qs[DEC_WAVES][DEC_MAX_HD / 4];
  __shared__ float ps[DEC_WAVES][64];
  __shared__ f32x4 red[DEC_WAVES][64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int t = a.t, len = a.len;
  if (a.t_dev) {  // one value for the whole grid: every wave of every workgroup leaves here, before any barrier
    t = *a.t_dev;
    if (t < 0 || t >= a.len) return;
    len = t + 1;
  }
  const int bh_raw = blockIdx.x * DEC_WAVES + w;
  // the workgroup's barriers need every wave: a wave past the last (b, h) redoes the last pair and stores nothing
  const bool valid = bh_raw < a.BH;
  const int bh = valid ? bh_raw : a.BH - 1;
  const int b = bh / a.H, h = bh - b * a.H;
  const int DC = a.hd >> 2;   // float4 column groups per row (<= 32)
  const int KG = 64 / DC;     // key groups of the P.V phase (>= 2)
  const bool append = t >= 0;

  const int bk = BEAM ? b / a.kv_group : b;  // the batch index of K, V and the mask
  const int32_t* arow = (BEAM && a.anc) ? a.anc + b * a.anc_s : nullptr;
  const float* qrow = a.q + b * a.q_sb + h * a.q_sh;
  float* Kb = a.K + bk * a.k_sb + h * a.k_sh;
  float* Vb = a.V + bk * a.v_sb + h * a.v_sh;
  const float* knew = append ? a.k_new + b * a.kn_sb + h * a.kn_sh : nullptr;
  const float* vnew = append ? a.v_new + b * a.vn_sb + h * a.vn_sh : nullptr;
  const uint8_t* mrow = a.mask ? a.mask + bk * a.mask_sb + h * a.mask_sh : nullptr;

  if (lane < DC) {
    qs[w][lane] = reinterpret_cast<const f32x4*>(qrow)[lane];
    if (append && valid) {  // this step's key / value row -> cache row t (rows above t are never touched)
      reinterpret_cast<f32x4*>(Kb + (int64_t)t * a.k_sn)[lane] = reinterpret_cast<const f32x4*>(knew)[lane];
      reinterpret_cast<f32x4*>(Vb + (int64_t)t * a.v_sn)[lane] = reinterpret_cast<const f32x4*>(vnew)[lane];
    }
  }
  __syncthreads();

  const int dc = lane % DC, kg = lane / DC;
  const bool pv_lane = kg < KG;  // 64 % DC lanes idle when hd/4 does not divide 64
  float m = -INFINITY, l = 0.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};

  for (int j0 = 0; j0 < len; j0 += 64) {
    // ---- scores of keys j0 .. j0 + 63 (lane = key) ----
    const int j = j0 + lane;
    const bool in = j < len;
    const int jc = in ? j : len - 1;  // always a readable row; the value is dropped below
    const float* krow = (append && jc == t) ? knew : Kb + (int64_t)jc * a.k_sn;
    if (BEAM && arow && jc != t) krow = a.K + anc_row(arow, jc, a.B) * a.k_sb + h * a.k_sh + (int64_t)jc * a.k_sn;
    float s = 0.f;
#pragma unroll 8
    for (int c = 0; c < DC; ++c) {
      const f32x4 kv = reinterpret_cast<const f32x4*>(krow)[c];
      const f32x4 qv = qs[w][c];
      s += qv[0] * kv[0];
      s += qv[1] * kv[1];
      s += qv[2] * kv[2];
      s += qv[3] * kv[3];
    }
    s *= a.scale;
    const bool masked = mrow ? mrow[jc] != 0 : false;
    s = (in && !masked) ? s : -INFINITY;

    // ---- online softmax ----
    const float mn = fmaxf(m, wave_max(s));  // wave-uniform
    // mn == -inf: nothing live yet (this chunk included): p = 0 everywhere, state unchanged
    const bool live = mn > -INFINITY;
    const float alpha = (m > -INFINITY) ? expf(m - mn) : 0.f;  // first live chunk: acc and l are 0 anyway
    const float p = (live && s > -INFINITY) ? expf(s - mn) : 0.f;
    __syncthreads();  // the previous chunk's P.V reads of ps are done
    ps[w][lane] = p;
    __syncthreads();
    if (live) {
      l = l * alpha + ln_wave_sum(p);
      m = mn;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] *= alpha;
      // ---- acc += P V over this chunk's keys (lane = key group x float4 column group) ----
      const int nk = (len - j0 < 64) ? len - j0 : 64;
      if (pv_lane) {
        // PV_U rows in flight per lane: the loads of a group are independent (issued together, row index clamped
        // to a real row and the value zeroed past the chunk), the FMAs keep the key order
        for (int jj = kg; jj < nk; jj += PV_U * KG) {
          f32x4 vv[PV_U];
          float pj[PV_U];
#pragma unroll
          for (int u = 0; u < PV_U; ++u) {
            const int ju = jj + u * KG;
            const bool ok = ju < nk;
            const int jl = ok ? ju : jj;
            const int jk = j0 + jl;
            const float* vrow = (append && jk == t) ? vnew : Vb + (int64_t)jk * a.v_sn;
            if (BEAM && arow && jk != t) vrow = a.V + anc_row(arow, jk, a.B) * a.v_sb + h * a.v_sh + (int64_t)jk * a.v_sn;
            const f32x4 x = reinterpret_cast<const f32x4*>(vrow)[dc];
            pj[u] = ok ? ps[w][jl] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) vv[u][e] = ok ? x[e] : 0.f;
          }
#pragma unroll
          for (int u = 0; u < PV_U; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += pj[u] * vv[u][e];
        }
      }
    }
  }

  // ---- sum the key groups in a fixed order, normalise, store ----
  red[w][lane] = acc;
  __syncthreads();
  if (lane < DC && valid) {
    f32x4 o = red[w][lane];
    for (int g = 1; g < KG; ++g) {
      const f32x4 r = red[w][g * DC + lane];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] += r[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = o[e] / l;  // all keys masked: 0 / 0 = NaN
    reinterpret_cast<f32x4*>(a.out + ((int64_t)b * a.H + h) * a.hd)[lane] = o;
  }
}

// ---- row argmax: lowest index among the maxima; an all -inf row gives index 0 ----
__device__ __forceinline__ void arg_merge(float& v, int64_t& i, float vo, int64_t io) {
  if (vo > v || (vo == v && io < i)) { v = vo; i = io; }
}

// The row's (maximum, lowest index of it), valid in thread 0 of the workgroup; ARG_T threads, all of them call.
__device__ __forceinline__ void argmax_row(const float* __restrict__ xr, int64_t V, bool vec, float& v, int64_t& i) {
  __shared__ float rv[ARG_T / 64];
  __shared__ int64_t ri[ARG_T / 64];
  // a thread walks its columns in increasing order with a strict >, so it keeps the lowest index of its maximum;
  // i = V marks "nothing above -inf seen" and loses every tie against a real index
  v = -INFINITY;
  i = V;
  if (vec) {
    for (int64_t c = 4 * (int64_t)threadIdx.x; c < V; c += 4 * ARG_T) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(xr + c);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (q[e] > v) { v = q[e]; i = c + e; }
    }
  } else {
    for (int64_t c = threadIdx.x; c < V; c += ARG_T) {
      const float q = xr[c];
      if (q > v) { v = q; i = c; }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float vo = __shfl_xor(v, o, 64);
    const int64_t io = __shfl_xor(i, o, 64);
    arg_merge(v, i, vo, io);
  }
  if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = v; ri[threadIdx.x >> 6] = i; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < ARG_T / 64; ++k) arg_merge(v, i, rv[k], ri[k]);
    if (i >= V) i = 0;  // all -inf (or NaN): index 0, always inside [0, V)
  }
}

__global__ __launch_bounds__(ARG_T) void k_argmax_rows(const float* __restrict__ x, int64_t V, int64_t* __restrict__ idx,
                                                      int64_t idx_stride, uint8_t* __restrict__ is_pad,
                                                      int64_t pad_stride, int64_t pad_id, float* __restrict__ maxval) {
  const int64_t row = blockIdx.x;
  float v;
  int64_t i;
  argmax_row(x + row * V, V, (V % 4 == 0) && (((uintptr_t)x) & 15) == 0, v, i);
  if (threadIdx.x == 0) {
    idx[row * idx_stride] = i;
    if (is_pad) is_pad[row * pad_stride] = (i == pad_id) ? 1 : 0;
    if (maxval) maxval[row] = v;
  }
}

// k_argmax_rows with the destination column t + 1 read from the device counter: ys[r, t+1], pad[r, t+1] and, for a
// (rows, H, T) per-head mask viewed as (H, rows, T), head_pad[h, r, t+1] for every h (what BaseDecoder.step copies
// from pad at the top of step t + 1). A column outside [1, T) stores nothing.
__global__ __launch_bounds__(ARG_T) void k_argmax_rows_step(const float* __restrict__ x, int64_t V, int64_t* __restrict__ ys,
                                                           int64_t ys_stride, int64_t T, uint8_t* __restrict__ pad,
                                                           int64_t pad_stride, uint8_t* __restrict__ head_pad, int H,
                                                           int64_t pad_id, const int32_t* __restrict__ t_dev) {
  const int64_t col = (int64_t)*t_dev + 1;
  if (col < 1 || col >= T) return;  // the whole grid, before the barrier
  const int64_t row = blockIdx.x, rows = gridDim.x;
  float v;
  int64_t i;
  argmax_row(x + row * V, V, (V % 4 == 0) && (((uintptr_t)x) & 15) == 0, v, i);
  if (threadIdx.x == 0) {
    const uint8_t p = (i == pad_id) ? 1 : 0;
    ys[row * ys_stride + col] = i;
    if (pad) pad[row * pad_stride + col] = p;
    if (head_pad)
      for (int h = 0; h < H; ++h) head_pad[((int64_t)h * rows + row) * T + col] = p;
  }
}

// k_argmax_rows_step with a finished flag per row: a row with fin != 0 takes pad_id and PAD byte 1 without reading its
// logits (the branch is uniform over the row's workgroup, so no barrier is skipped by part of it); a live row whose
// argmax is eos_id sets its flag. eos_id < 0: no token finishes a row.
__global__ __launch_bounds__(ARG_T) void k_argmax_rows_fin_step(const float* __restrict__ x, int64_t V,
                                                               int64_t* __restrict__ ys, int64_t ys_stride, int64_t T,
                                                               uint8_t* __restrict__ pad, int64_t pad_stride,
                                                               uint8_t* __restrict__ head_pad, int H, int64_t pad_id,
                                                               uint8_t* __restrict__ fin, int64_t eos_id,
                                                               const int32_t* __restrict__ t_dev) {
  const int64_t col = (int64_t)*t_dev + 1;
  if (col < 1 || col >= T) return;  // the whole grid, before the barrier
  const int64_t row = blockIdx.x, rows = gridDim.x;
  const bool done = fin[row] != 0;
  float v = 0.f;
  int64_t i = pad_id;
  if (!done) argmax_row(x + row * V, V, (V % 4 == 0) && (((uintptr_t)x) & 15) == 0, v, i);
  if (threadIdx.x == 0) {
    const uint8_t p = (done || i == pad_id) ? 1 : 0;
    ys[row * ys_stride + col] = i;
    if (pad) pad[row * pad_stride + col] = p;
    if (head_pad)
      for (int h = 0; h < H; ++h) head_pad[((int64_t)h * rows + row) * T + col] = p;
    if (!done && eos_id >= 0 && i == eos_id) fin[row] = 1;
  }
}

// The end of an early-stopping decode step, in place of the counter's increment: one workgroup reduces the finished
// flags to all_now (every byte of fin[0..R) non-zero) and thread 0 moves the latch st = {all_prev, steps_run, parked,
// reserved}. Parked: nothing changes. Otherwise the step that just ran is counted and the counter either parks at -1
// (this step began with every row finished, or it was the last one), which makes every later launch of the step store
// nothing, or moves on. fin is read byte by byte (any alignment); the reduction is an OR, the same in any order.
constexpr int ADV_T = 256;

__global__ __launch_bounds__(ADV_T) void k_decode_advance(const uint8_t* __restrict__ fin, int64_t R, int64_t T,
                                                         int32_t* __restrict__ t_dev, int32_t* __restrict__ st) {
  __shared__ int live_w[ADV_T / 64];
  bool live = false;
  for (int64_t r = threadIdx.x; r < R; r += ADV_T) live |= fin[r] == 0;
  const bool wave_live = __ballot(live) != 0;
  if ((threadIdx.x & 63) == 0) live_w[threadIdx.x >> 6] = wave_live ? 1 : 0;
  __syncthreads();
  if (threadIdx.x != 0) return;
  int any_live = 0;
#pragma unroll
  for (int k = 0; k < ADV_T / 64; ++k) any_live |= live_w[k];
  if (st[2] != 0) return;
  const int64_t t = *t_dev;
  st[1] += 1;
  if (st[0] != 0 || t + 1 >= T - 1) {
    *t_dev = -1;
    st[2] = 1;
  } else {
    *t_dev = (int32_t)(t + 1);
    st[0] = any_live ? 0 : 1;
  }
}

// x[b] = LayerNorm(W[ys[b, t]] + pe[t]) for the position t read from the device counter (Embeddings.step): one wave
// per row, the gathered row in registers, normalised by the LayerNorm forward's own row function. pe may be null
// (no positional term). A token id outside [0, vocab) is clamped; a t outside [0, t_end) stores nothing.
template <int CPL>
__global__ __launch_bounds__(256) void k_decode_embed(const int64_t* __restrict__ ys, int64_t ys_stride, int64_t B,
                                                      int64_t t_end, const int32_t* __restrict__ t_dev,
                                                      const float* __restrict__ W, int64_t vocab,
                                                      const float* __restrict__ pe, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, float* __restrict__ x,
                                                      int E) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t t = *t_dev;
  if (t < 0 || t >= t_end || row >= B) return;
  int64_t id = ys[row * ys_stride + t];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float* wr = W + id * E;
  const float* pr = pe ? pe + t * E : nullptr;
  f32x4 v[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int c = 4 * (lane + 64 * q);
    v[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < E) {
      v[q] = *reinterpret_cast<const f32x4*>(wr + c);
      if (pr) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(pr + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[q][e] += p[e];
      }
    }
  }
  float mean, rstd;
  ln_row_fwd<CPL>(v, lane, E, eps, gamma, beta, x + row * E, mean, rstd);
}

inline bool m4(int64_t s) { return s % 4 == 0; }

// csa_decode_attn (step == false: host t, len = key count) and csa_decode_attn_step (step == true: t read from
// t_dev by the kernel, len = the capacity of K / V / mask): one validation, one kernel. csa_decode_attn_beam
// (beam == true) is either of them, by t_dev, on the BEAM instantiation with its ancestry table and group.
csa_status decode_attn_impl(const char* fn, const csa_decode_attn_args* a, bool step, const int32_t* t_dev, void* stream,
                            bool beam = false, const int32_t* anc = nullptr, int64_t anc_stride = 0, int64_t kv_group = 1) {
  const auto fail = [fn](csa_status s, const char* m) {
    csa::set_error("%s: %s", fn, m);
    return s;
  };
  if (!a) return fail(CSA_INVALID_ARG, "null args");
  if (a->B < 0 || a->H < 1 || a->len < 1 || a->B * a->H > 0x7fffffff || a->len > 0x7fffffff)
    return fail(CSA_INVALID_ARG, "B, H, len must be positive (len >= 1)");
  if (!csa_decode_attn_supported(a->hd)) return fail(CSA_UNSUPPORTED_SHAPE, "hd must be a multiple of 4 in [4, 128]");
  const bool append = a->k_new || a->v_new;
  if (append && (!a->k_new || !a->v_new)) return fail(CSA_INVALID_ARG, "k_new and v_new go together");
  if (step) {
    if (!append) return fail(CSA_INVALID_ARG, "k_new and v_new are required");
    if (!t_dev || !aligned(t_dev, 4)) return fail(CSA_INVALID_ARG, "t_dev must be a 4-byte aligned device pointer");
  } else if (append && (a->t < 0 || a->t + 1 != a->len)) {
    return fail(CSA_INVALID_ARG, "append mode needs len == t + 1");
  }
  if (beam) {
    if (kv_group < 1 || kv_group > 0x7fffffff || a->B % kv_group != 0)
      return fail(CSA_INVALID_ARG, "kv_group must be positive and divide the row count B");
    if (anc && (kv_group != 1 || !append))
      return fail(CSA_INVALID_ARG, "an ancestry table goes with append mode and kv_group == 1");
    if (anc && (!aligned(anc, 4) || anc_stride < a->len))
      return fail(CSA_INVALID_ARG, "anc must be 4-byte aligned with a row stride >= len");
  }
  if (a->B == 0) return CSA_OK;
  if (!a->q || !a->K || !a->V || !a->out) return fail(CSA_INVALID_ARG, "null pointer");
  if (!aligned(a->q, 16) || !aligned(a->K, 16) || !aligned(a->V, 16) || !aligned(a->out, 16) || !aligned(a->k_new, 16) ||
      !aligned(a->v_new, 16) ||
      !m4(a->q_sb) || !m4(a->q_sh) || !m4(a->k_sb) || !m4(a->k_sh) || !m4(a->k_sn) || !m4(a->v_sb) || !m4(a->v_sh) ||
      !m4(a->v_sn) || (append && (!m4(a->kn_sb) || !m4(a->kn_sh) || !m4(a->vn_sb) || !m4(a->vn_sh))))
    return fail(CSA_INVALID_ARG, "pointers must be 16-byte aligned and strides multiples of 4 elements");
  DecArgs d;
  d.BH = (int)(a->B * a->H); d.H = (int)a->H; d.hd = (int)a->hd; d.len = (int)a->len;
  d.t = step ? 0 : (append ? (int)a->t : -1);
  d.t_dev = step ? t_dev : nullptr;
  d.q = a->q; d.q_sb = a->q_sb; d.q_sh = a->q_sh;
  d.K = a->K; d.k_sb = a->k_sb; d.k_sh = a->k_sh; d.k_sn = a->k_sn;
  d.V = a->V; d.v_sb = a->v_sb; d.v_sh = a->v_sh; d.v_sn = a->v_sn;
  d.k_new = a->k_new; d.kn_sb = a->kn_sb; d.kn_sh = a->kn_sh;
  d.v_new = a->v_new; d.vn_sb = a->vn_sb; d.vn_sh = a->vn_sh;
  d.mask = a->mask; d.mask_sb = a->mask_sb; d.mask_sh = a->mask_sh;
  d.scale = a->scale;
  d.out = a->out;
  d.anc = anc; d.anc_s = anc_stride; d.kv_group = (int)kv_group; d.B = (int)a->B;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  const dim3 grid((unsigned)((d.BH + DEC_WAVES - 1) / DEC_WAVES));
  if (beam)
    hipLaunchKernelGGL(k_decode_attn<true>, grid, dim3(64 * DEC_WAVES), 0, st, d);
  else
    hipLaunchKernelGGL(k_decode_attn<false>, grid, dim3(64 * DEC_WAVES), 0, st, d);
  return launched(fn);
}

// csa_argmax_rows_step and csa_argmax_rows_fin_step (with_fin: the finished flags and eos_id): one validation, the
// entry point's own kernel.
csa_status argmax_step_impl(const char* fn, const float* x, int64_t rows, int64_t V, int64_t* ys, int64_t ys_stride,
                            int64_t T, uint8_t* pad, int64_t pad_stride, uint8_t* head_pad, int64_t H, int64_t pad_id,
                            bool with_fin, uint8_t* fin, int64_t eos_id, const int32_t* t_dev, void* stream) {
  const auto fail = [fn](csa_status s, const char* m) {
    csa::set_error("%s: %s", fn, m);
    return s;
  };
  if (rows < 0 || V < 1 || rows > 0x7fffffff || T < 1 || ys_stride < T || (pad && pad_stride < T) ||
      (head_pad && (H < 1 || H > 0x7fffffff)))
    return fail(CSA_INVALID_ARG, "bad rows / V / T / strides / H");
  if (!x || !ys || (with_fin && !fin) || !t_dev) return fail(CSA_INVALID_ARG, "null pointer");
  if (!aligned(x, 4) || !aligned(ys, 8) || !aligned(t_dev, 4)) return fail(CSA_INVALID_ARG, "misaligned pointer");
  if (rows == 0) return CSA_OK;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  if (with_fin)
    hipLaunchKernelGGL(k_argmax_rows_fin_step, dim3((unsigned)rows), dim3(ARG_T), 0, st, x, V, ys, ys_stride, T, pad,
                       pad_stride, head_pad, (int)H, pad_id, fin, eos_id, t_dev);
  else
    hipLaunchKernelGGL(k_argmax_rows_step, dim3((unsigned)rows), dim3(ARG_T), 0, st, x, V, ys, ys_stride, T, pad,
                       pad_stride, head_pad, (int)H, pad_id, t_dev);
  return launched(fn);
}

}  // namespace

extern "C" {

int csa_decode_attn_supported(int64_t hd) { return (hd >= 4 && hd <= DEC_MAX_HD && hd % 4 == 0) ? 1 : 0; }

csa_status csa_decode_attn(const csa_decode_attn_args* a, void* stream) {
  return decode_attn_impl("csa_decode_attn", a, false, nullptr, stream);
}

csa_status csa_decode_attn_step(const csa_decode_attn_args* a, const int32_t* t_dev, void* stream) {
  return decode_attn_impl("csa_decode_attn_step", a, true, t_dev, stream);
}

csa_status csa_decode_attn_beam(const csa_decode_attn_args* a, const int32_t* t_dev, const int32_t* anc,
                                int64_t anc_stride, int64_t kv_group, void* stream) {
  return decode_attn_impl("csa_decode_attn_beam", a, t_dev != nullptr, t_dev, stream, true, anc, anc_stride, kv_group);
}

csa_status csa_decode_embed(const int64_t* ys, int64_t ys_stride, int64_t B, int64_t T, const int32_t* t_dev,
                            const float* W, int64_t vocab, const float* pe, int64_t max_len, const float* gamma,
                            const float* beta, float eps, float* x, int64_t E, void* stream) {
  const int cpl = ln_cpl(E);
  if (cpl == 0) return fail(CSA_UNSUPPORTED_SHAPE, "csa_decode_embed: E must be a multiple of 4 in [4, 1024]");
  if (B < 0 || B > 0x7fffffff || T < 1 || vocab < 1 || (pe && max_len < 1) || ys_stride < T)
    return fail(CSA_INVALID_ARG, "csa_decode_embed: bad B / T / vocab / max_len / ys_stride");
  if (!ys || !t_dev || !W || !gamma || !beta || !x) return fail(CSA_INVALID_ARG, "csa_decode_embed: null pointer");
  if (!aligned(ys, 8) || !aligned(t_dev, 4) || !aligned(W, 16) || !aligned(pe, 16) || !aligned(gamma, 16) ||
      !aligned(beta, 16) || !aligned(x, 16))
    return fail(CSA_INVALID_ARG, "csa_decode_embed: misaligned pointer (ys 8, t_dev 4, the fp32 rows 16 bytes)");
  if (B == 0) return CSA_OK;
  const int64_t t_end = (pe && max_len < T) ? max_len : T;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  const dim3 grid((unsigned)((B + 3) / 4));
#define CSA_EMBED_LAUNCH(C)                                                                                         \
  hipLaunchKernelGGL(k_decode_embed<C>, grid, dim3(256), 0, st, ys, ys_stride, B, t_end, t_dev, W, vocab, pe, gamma, \
                     beta, eps, x, (int)E)
  switch (cpl) {
    case 1: CSA_EMBED_LAUNCH(1); break;
    case 2: CSA_EMBED_LAUNCH(2); break;
    case 3: CSA_EMBED_LAUNCH(3); break;
    default: CSA_EMBED_LAUNCH(4);
  }
#undef CSA_EMBED_LAUNCH
  return launched("csa_decode_embed");
}

csa_status csa_argmax_rows(const float* x, int64_t rows, int64_t V, int64_t* idx, int64_t idx_stride, uint8_t* is_pad,
                           int64_t pad_stride, int64_t pad_id, float* maxval, void* stream) {
  if (rows < 0 || V < 1 || rows > 0x7fffffff) return fail(CSA_INVALID_ARG, "csa_argmax_rows: bad rows / V");
  if (!x || !idx) return fail(CSA_INVALID_ARG, "csa_argmax_rows: null pointer");
  if (!aligned(x, 4) || !aligned(idx, 8)) return fail(CSA_INVALID_ARG, "csa_argmax_rows: misaligned pointer");
  if (rows == 0) return CSA_OK;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  hipLaunchKernelGGL(k_argmax_rows, dim3((unsigned)rows), dim3(ARG_T), 0, st, x, V, idx, idx_stride, is_pad, pad_stride,
                     pad_id, maxval);
  return launched("csa_argmax_rows");
}

csa_status csa_argmax_rows_step(const float* x, int64_t rows, int64_t V, int64_t* ys, int64_t ys_stride, int64_t T,
                                uint8_t* pad, int64_t pad_stride, uint8_t* head_pad, int64_t H, int64_t pad_id,
                                const int32_t* t_dev, void* stream) {
  return argmax_step_impl("csa_argmax_rows_step", x, rows, V, ys, ys_stride, T, pad, pad_stride, head_pad, H, pad_id, false,
                          nullptr, 0, t_dev, stream);
}

csa_status csa_argmax_rows_fin_step(const float* x, int64_t rows, int64_t V, int64_t* ys, int64_t ys_stride, int64_t T,
                                    uint8_t* pad, int64_t pad_stride, uint8_t* head_pad, int64_t H, int64_t pad_id,
                                    uint8_t* fin, int64_t eos_id, const int32_t* t_dev, void* stream) {
  return argmax_step_impl("csa_argmax_rows_fin_step", x, rows, V, ys, ys_stride, T, pad, pad_stride, head_pad, H, pad_id,
                          true, fin, eos_id, t_dev, stream);
}

csa_status csa_decode_advance(const uint8_t* fin, int64_t rows, int64_t T, int32_t* t_dev, int32_t* state,
                              void* stream) {
  if (rows < 0 || T < 2) return fail(CSA_INVALID_ARG, "csa_decode_advance: bad rows / T (rows >= 0, T >= 2)");
  if (!t_dev || !state || (rows > 0 && !fin)) return fail(CSA_INVALID_ARG, "csa_decode_advance: null pointer");
  if (!aligned(t_dev, 4) || !aligned(state, 4))
    return fail(CSA_INVALID_ARG, "csa_decode_advance: misaligned pointer (t_dev and state 4 bytes; fin any)");
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  hipLaunchKernelGGL(k_decode_advance, dim3(1), dim3(ADV_T), 0, st, fin, rows, T, t_dev, state);
  return launched("csa_decode_advance");
}

}  // extern "C"
