// Full-sequence (teacher-forced) decoder attention, forward and backward, fp32 throughout:
//
//   out[r, i, h*hd:(h+1)*hd] = sum_j softmax_j(scale * q[r,h,i] . K[kb,h,j] + m(r,h,i,j)) * V[kb,h,j],  kb = r / kv_group
//
// with the causal, PAD and memory masks applied in the kernel from uint8 rows, the kv_group query rows of an AST
// reading ONE K/V (the un-repeated memory projection), and their dK / dV summed inside the key-side backward kernel in
// index order. No tensor of size (R, H, T, S) exists: the forward keeps an online softmax per query row and saves
// lse (R, H, T); the backward recomputes P = exp(scale * s - lse) tile by tile.
//
// One wave per workgroup, 16 x 16 tiles on the exact-fp32 v_mfma_f32_16x16x4_f32 (mfma16, csa_common.hpp). Lane
// l = (x = l & 15, g = l >> 4). Two product forms cover all seven contractions:
//   "lin"  D[a][b] = sum_c A[a][c] B[b][c] over the head dim: both operands are ROW fragments, lane (x, g) holding
//          columns g * hd/4 + s (s = MFMA step) of row x of its 16-row tile (dwordx4 loads for hd = 64). The result sits
//          in the C layout: register e of lane (x, g) = D[4 g + e][x].
//   "acc"  D^T[d][b] += sum_t X[t][d] P[t][b] over the 16 rows t of a tile, P being a C-layout tile as the lin form
//          leaves it: step s takes P's register s as the B operand (t = 4 g + s), and X[t][16 dt + x] as the A operand,
//          so a probability tile feeds the next product with no data movement and no LDS.
// The forward and the query-side backward compute S^T (A = K rows, B = Q rows): a lane then owns ONE query x and four
// keys 4 g + e, the row statistics need two shuffles (over g), and O^T / dQ^T accumulate by the acc form over keys. The
// key-side backward computes S (A = Q rows, B = K rows): a lane owns one key x, and dV^T / dK^T accumulate by the acc
// form over queries, for every row of the group and every query tile in ascending order: a fixed summation order, no
// atomics. hd = 8 (the tiny test model) runs the same code with the one 16-wide head-dim tile of the acc form half
// padding (zero A operands, nothing stored).
//
// Every row index is clamped into its tensor before a load and the VALUE is selected afterwards, so no load is ever out
// of bounds whatever T and S are; a masked key's probability is selected to 0, never computed as exp(-inf - x). A query
// row with every key masked gets l = 0 and out = 0 * (1 / 0) = NaN, lse = -inf; in the backward all its keys are
// masked, so it contributes exact zeros (its own dq is zero).
#include "csa_common.hpp"
#include "../../include/csa_hip.h"

#include <math.h>
#include <stdio.h>

using namespace csa;

namespace {

constexpr int TILE = 16;
constexpr int64_t MAX_T = 256;

struct SaArgs {
  int R, H, T, S, G, causal, mask_mode;
  const float* q; int64_t q_sr, q_sh, q_st;
  const float* k; int64_t k_sb, k_sh, k_sn;
  const float* v; int64_t v_sb, v_sh, v_sn;
  const uint8_t* mask; int64_t mask_ld;
  float scale;
  float* out; float* lse;
  // backward
  const float* dout; float* dsum;  // dsum (R, H, T): rowsum(dO * O), written by the query side, read by the key side
  float* dq; int64_t dq_sr, dq_sh, dq_st;
  float* dk; int64_t dk_sb, dk_sh, dk_sn;
  float* dv; int64_t dv_sb, dv_sh, dv_sn;
};

template <int HD> constexpr int ndt() { return (HD + 15) / 16; }

__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// row fragment of the lin form: columns g * HD/4 .. + HD/4 of row min(row0 + x, nrows - 1)
template <int HD>
__device__ __forceinline__ void load_lin(float* f, const float* __restrict__ base, int64_t stride, int row0, int nrows) {
  const int x = lane_id() & 15, g = lane_id() >> 4;
  const float* p = base + (int64_t)imin(row0 + x, nrows - 1) * stride + g * (HD / 4);
  if constexpr (HD % 16 == 0) {
#pragma unroll
    for (int s = 0; s < HD / 4; s += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p + s);
      f[s] = t[0]; f[s + 1] = t[1]; f[s + 2] = t[2]; f[s + 3] = t[3];
    }
  } else {
#pragma unroll
    for (int s = 0; s < HD / 4; ++s) f[s] = p[s];
  }
}

template <int HD>
__device__ __forceinline__ f32x4 mm_lin(const float* a, const float* b) {
  f32x4 acc = zero4();
#pragma unroll
  for (int s = 0; s < HD / 4; ++s) acc = mfma16(a[s], b[s], acc);
  return acc;
}

// acc[dt] register e of lane (x, g) += sum_t X[row0 + t][16 dt + 4 g + e] * P[t][x]; rows past nrows are clamped: the
// caller has selected their P to zero
template <int HD>
__device__ __forceinline__ void mm_acc(f32x4* acc, const float* __restrict__ base, int64_t stride, int row0, int nrows,
                                       const f32x4 p) {
  const int x = lane_id() & 15, g = lane_id() >> 4;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float* row = base + (int64_t)imin(row0 + 4 * g + s, nrows - 1) * stride;
#pragma unroll
    for (int dt = 0; dt < ndt<HD>(); ++dt) {
      const int col = 16 * dt + x;
      const float v = row[imin(col, HD - 1)];
      acc[dt] = mfma16(col < HD ? v : 0.f, p[s], acc[dt]);
    }
  }
}

// a lane's four head-dim elements 16 dt + 4 g + e of row `dst` (hd contiguous, 16-byte aligned rows)
template <int HD>
__device__ __forceinline__ void store_rows(float* dst, const f32x4* acc, float mul) {
  const int g = lane_id() >> 4;
#pragma unroll
  for (int dt = 0; dt < ndt<HD>(); ++dt) {
    const int d0 = 16 * dt + 4 * g;
    if (d0 < HD) *reinterpret_cast<f32x4*>(dst + d0) = acc[dt] * mul;
  }
}

__device__ __forceinline__ float over_g_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float over_g_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// scale * s as ONE rounded product in all three kernels. Left to the compiler, the backward's scale * s - lse becomes an
// fma of the unrounded product while the forward's lse holds the rounded one, and a query with a single visible key
// gets p = exp(1 ulp) instead of exactly 1 (hd = 8: the scale is not a power of two).
__device__ __forceinline__ float scaled(float s, float scale) {
#pragma clang fp contract(off)
  return s * scale;
}

struct Block { int r, h, kb, tile; };

// blockIdx.x -> (row, head, tile): tiles of one (row, head) are neighbours
__device__ __forceinline__ Block block_of(int ntiles, int H, int G) {
  Block b;
  const int id = blockIdx.x, rh = id / ntiles;
  b.tile = id % ntiles;
  b.h = rh % H;
  b.r = rh / H;
  b.kb = b.r / G;
  return b;
}

__device__ __forceinline__ const uint8_t* mask_row(const SaArgs& a, int r, int h) {
  if (!a.mask) return nullptr;
  const int64_t row = a.mask_mode ? ((int64_t)r * a.H + h) % a.R : r / a.G;
  return a.mask + row * a.mask_ld;
}

// key j is masked for query i (both real indices; j < S)
__device__ __forceinline__ bool masked(const SaArgs& a, const uint8_t* mrow, int i, int j) {
  return j >= a.S || (a.causal && j > i) || (mrow && mrow[imin(j, a.S - 1)] != 0);
}

template <int HD>
__global__ __launch_bounds__(64) void k_seq_attn_fwd(const SaArgs a) {
  const Block b = block_of((a.T + TILE - 1) / TILE, a.H, a.G);
  const int x = lane_id() & 15, g = lane_id() >> 4;
  const int q0 = b.tile * TILE, i = q0 + x;
  const float* kbase = a.k + b.kb * a.k_sb + b.h * a.k_sh;
  const float* vbase = a.v + b.kb * a.v_sb + b.h * a.v_sh;
  const uint8_t* mrow = mask_row(a, b.r, b.h);
  float qf[HD / 4];
  load_lin<HD>(qf, a.q + b.r * a.q_sr + b.h * a.q_sh, a.q_st, q0, a.T);
  f32x4 o[ndt<HD>()];
#pragma unroll
  for (int dt = 0; dt < ndt<HD>(); ++dt) o[dt] = zero4();
  float m = -INFINITY, l = 0.f;
  const int kend = a.causal ? imin(a.S, q0 + TILE) : a.S;
  for (int j0 = 0; j0 < kend; j0 += TILE) {
    float kf[HD / 4];
    load_lin<HD>(kf, kbase, a.k_sn, j0, a.S);
    f32x4 s = mm_lin<HD>(kf, qf);  // register e: key j0 + 4 g + e, query x
    bool dead[4];
    float tmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dead[e] = masked(a, mrow, i, j0 + 4 * g + e);
      s[e] = dead[e] ? -INFINITY : scaled(s[e], a.scale);
      tmax = fmaxf(tmax, s[e]);
    }
    const float m_new = fmaxf(m, over_g_max(tmax));
    const float m_ref = m_new == -INFINITY ? 0.f : m_new;  // nothing unmasked yet: every p below is selected to 0
    const float alpha = expf(m - m_ref);
    f32x4 p;
    float ps = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      p[e] = dead[e] ? 0.f : expf(s[e] - m_ref);
      ps += p[e];
    }
    l = l * alpha + over_g_sum(ps);
    m = m_new;
#pragma unroll
    for (int dt = 0; dt < ndt<HD>(); ++dt) o[dt] *= alpha;
    mm_acc<HD>(o, vbase, a.v_sn, j0, a.S, p);
  }
  if (i < a.T) {
    store_rows<HD>(a.out + (((int64_t)b.r * a.T + i) * a.H + b.h) * HD, o, 1.f / l);  // l == 0: 0 * inf = NaN
    if (g == 0) a.lse[((int64_t)b.r * a.H + b.h) * a.T + i] = m + logf(l);
  }
}

// query side: dq, and dsum for the key side
template <int HD>
__global__ __launch_bounds__(64) void k_seq_attn_bwd_q(const SaArgs a) {
  const Block b = block_of((a.T + TILE - 1) / TILE, a.H, a.G);
  const int x = lane_id() & 15, g = lane_id() >> 4;
  const int q0 = b.tile * TILE, i = q0 + x, ic = imin(i, a.T - 1);
  const float* kbase = a.k + b.kb * a.k_sb + b.h * a.k_sh;
  const float* vbase = a.v + b.kb * a.v_sb + b.h * a.v_sh;
  const uint8_t* mrow = mask_row(a, b.r, b.h);
  const int64_t orow = ((int64_t)b.r * a.T * a.H + b.h) * HD, ost = (int64_t)a.H * HD;  // (R, T, H*hd) rows of this head
  const int64_t stat = ((int64_t)b.r * a.H + b.h) * a.T;
  float qf[HD / 4], dof[HD / 4], of[HD / 4];
  load_lin<HD>(qf, a.q + b.r * a.q_sr + b.h * a.q_sh, a.q_st, q0, a.T);
  load_lin<HD>(dof, a.dout + orow, ost, q0, a.T);
  load_lin<HD>(of, a.out + orow, ost, q0, a.T);
  float dsum = 0.f;
#pragma unroll
  for (int s = 0; s < HD / 4; ++s) dsum = fmaf(dof[s], of[s], dsum);
  dsum = over_g_sum(dsum);
  if (i < a.T && g == 0) a.dsum[stat + i] = dsum;
  const float lse = a.lse[stat + ic];
  f32x4 dq[ndt<HD>()];
#pragma unroll
  for (int dt = 0; dt < ndt<HD>(); ++dt) dq[dt] = zero4();
  const int kend = a.causal ? imin(a.S, q0 + TILE) : a.S;
  for (int j0 = 0; j0 < kend; j0 += TILE) {
    float kf[HD / 4], vf[HD / 4];
    load_lin<HD>(kf, kbase, a.k_sn, j0, a.S);
    load_lin<HD>(vf, vbase, a.v_sn, j0, a.S);
    const f32x4 s = mm_lin<HD>(kf, qf);
    const f32x4 dp = mm_lin<HD>(vf, dof);
    f32x4 ds;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool dead = masked(a, mrow, i, j0 + 4 * g + e);
      const float p = expf(scaled(s[e], a.scale) - lse);
      ds[e] = dead ? 0.f : p * (dp[e] - dsum);
    }
    mm_acc<HD>(dq, kbase, a.k_sn, j0, a.S, ds);
  }
  if (i < a.T) store_rows<HD>(a.dq + b.r * a.dq_sr + b.h * a.dq_sh + i * a.dq_st, dq, a.scale);
}

// key side: dk, dv of one 16-key tile of (kb, h), summed over the group's rows and their query tiles in index order
template <int HD>
__global__ __launch_bounds__(64) void k_seq_attn_bwd_kv(const SaArgs a) {
  const int nkt = (a.S + TILE - 1) / TILE;
  const int id = blockIdx.x, bh = id / nkt, kt = id % nkt, h = bh % a.H, kb = bh / a.H;
  const int x = lane_id() & 15, g = lane_id() >> 4;
  const int j0 = kt * TILE, j = j0 + x;
  float kf[HD / 4], vf[HD / 4];
  load_lin<HD>(kf, a.k + kb * a.k_sb + h * a.k_sh, a.k_sn, j0, a.S);
  load_lin<HD>(vf, a.v + kb * a.v_sb + h * a.v_sh, a.v_sn, j0, a.S);
  f32x4 dk[ndt<HD>()], dv[ndt<HD>()];
#pragma unroll
  for (int dt = 0; dt < ndt<HD>(); ++dt) dk[dt] = dv[dt] = zero4();
  const int64_t ost = (int64_t)a.H * HD;
  for (int gi = 0; gi < a.G; ++gi) {
    const int r = kb * a.G + gi;
    const uint8_t* mrow = mask_row(a, r, h);
    const float* qbase = a.q + r * a.q_sr + h * a.q_sh;
    const float* dobase = a.dout + ((int64_t)r * a.T * a.H + h) * HD;
    const int64_t stat = ((int64_t)r * a.H + h) * a.T;
    for (int i0 = a.causal ? j0 : 0; i0 < a.T; i0 += TILE) {  // causal: the queries before this key tile see none of it
      float qf[HD / 4], dof[HD / 4];
      load_lin<HD>(qf, qbase, a.q_st, i0, a.T);
      load_lin<HD>(dof, dobase, ost, i0, a.T);
      const f32x4 s = mm_lin<HD>(qf, kf);  // register e: query i0 + 4 g + e, key x
      const f32x4 dp = mm_lin<HD>(dof, vf);
      f32x4 p, ds;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + 4 * g + e, ic = imin(i, a.T - 1);
        const float lse = a.lse[stat + ic], dsum = a.dsum[stat + ic];
        const bool dead = i >= a.T || masked(a, mrow, i, j);
        const float pe = expf(scaled(s[e], a.scale) - lse);
        p[e] = dead ? 0.f : pe;
        ds[e] = dead ? 0.f : pe * (dp[e] - dsum);
      }
      mm_acc<HD>(dv, dobase, ost, i0, a.T, p);
      mm_acc<HD>(dk, qbase, a.q_st, i0, a.T, ds);
    }
  }
  if (j < a.S) {
    store_rows<HD>(a.dk + kb * a.dk_sb + h * a.dk_sh + j * a.dk_sn, dk, a.scale);
    store_rows<HD>(a.dv + kb * a.dv_sb + h * a.dv_sh + j * a.dv_sn, dv, 1.f);
  }
}

inline bool strides_ok(int64_t s0, int64_t s1, int64_t s2) {
  return s0 >= 0 && s1 >= 0 && s2 >= 0 && ((s0 | s1 | s2) & 3) == 0;
}

csa_status check_fwd(const csa_seq_attn_args* a, const char* fn, SaArgs* d) {
  static thread_local char msg[160];
  auto bad = [&](csa_status s, const char* what) {
    snprintf(msg, sizeof msg, "%s: %s", fn, what);
    return fail(s, msg);
  };
  if (!a) return bad(CSA_INVALID_ARG, "null args");
  if (a->R < 1 || a->H < 1 || a->T < 1 || a->S < 1 || a->hd < 1 || a->kv_group < 1)
    return bad(CSA_INVALID_ARG, "R, H, T, S, hd, kv_group must be positive");
  if (a->R % a->kv_group) return bad(CSA_INVALID_ARG, "kv_group must divide R");
  if (a->causal && (a->S != a->T || a->kv_group != 1)) return bad(CSA_INVALID_ARG, "causal needs S == T and kv_group == 1");
  if (a->mask_mode != 0 && a->mask_mode != 1) return bad(CSA_INVALID_ARG, "mask_mode is 0 or 1");
  if (!csa_seq_attn_supported(a->hd, a->T, a->S)) return bad(CSA_UNSUPPORTED_SHAPE, "hd in {8, 64}, T <= 256");
  const int64_t tiles = (a->T + TILE - 1) / TILE > (a->S + TILE - 1) / TILE ? (a->T + TILE - 1) / TILE : (a->S + TILE - 1) / TILE;
  if (a->R > 0x7fffffff / a->H || a->R * a->H > 0x7fffffff / tiles)
    return bad(CSA_UNSUPPORTED_SHAPE, "R * H * tiles exceeds the grid limit");
  if (!a->q || !a->k || !a->v || !a->out || !a->lse) return bad(CSA_INVALID_ARG, "null pointer");
  if (!aligned(a->q, 16) || !aligned(a->k, 16) || !aligned(a->v, 16) || !aligned(a->out, 16) || !aligned(a->lse, 4))
    return bad(CSA_INVALID_ARG, "q, k, v, out must be 16-byte aligned");
  if (!strides_ok(a->q_sr, a->q_sh, a->q_st) || !strides_ok(a->k_sb, a->k_sh, a->k_sn) || !strides_ok(a->v_sb, a->v_sh, a->v_sn))
    return bad(CSA_INVALID_ARG, "strides must be non-negative multiples of 4 elements");
  if (a->mask && a->mask_ld < a->S) return bad(CSA_INVALID_ARG, "mask_ld < S");
  *d = SaArgs{};
  d->R = (int)a->R; d->H = (int)a->H; d->T = (int)a->T; d->S = (int)a->S; d->G = (int)a->kv_group;
  d->causal = a->causal ? 1 : 0; d->mask_mode = a->mask_mode;
  d->q = a->q; d->q_sr = a->q_sr; d->q_sh = a->q_sh; d->q_st = a->q_st;
  d->k = a->k; d->k_sb = a->k_sb; d->k_sh = a->k_sh; d->k_sn = a->k_sn;
  d->v = a->v; d->v_sb = a->v_sb; d->v_sh = a->v_sh; d->v_sn = a->v_sn;
  d->mask = a->mask; d->mask_ld = a->mask_ld;
  d->scale = a->scale; d->out = a->out; d->lse = a->lse;
  return CSA_OK;
}

}  // namespace

extern "C" {

int csa_seq_attn_supported(int64_t hd, int64_t T, int64_t S) {
  return ((hd == 64 || hd == 8) && T >= 1 && T <= MAX_T && S >= 1 && S <= 0x7fffffff - TILE) ? 1 : 0;
}

size_t csa_seq_attn_bwd_workspace_bytes(int64_t R, int64_t H, int64_t T) {
  return (R < 1 || H < 1 || T < 1) ? 0 : (size_t)R * (size_t)H * (size_t)T * sizeof(float);
}

csa_status csa_seq_attn_fwd(const csa_seq_attn_args* a, void* stream) {
  SaArgs d;
  const csa_status s = check_fwd(a, "csa_seq_attn_fwd", &d);
  if (s != CSA_OK) return s;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  const dim3 grid((unsigned)(a->R * a->H * ((a->T + TILE - 1) / TILE)));
  if (a->hd == 64) hipLaunchKernelGGL(k_seq_attn_fwd<64>, grid, dim3(64), 0, st, d);
  else hipLaunchKernelGGL(k_seq_attn_fwd<8>, grid, dim3(64), 0, st, d);
  return launched("csa_seq_attn_fwd");
}

csa_status csa_seq_attn_bwd(const csa_seq_attn_bwd_args* b, void* stream) {
  if (!b) return fail(CSA_INVALID_ARG, "csa_seq_attn_bwd: null args");
  SaArgs d;
  const csa_seq_attn_args* a = b->fwd;
  const csa_status s = check_fwd(a, "csa_seq_attn_bwd", &d);
  if (s != CSA_OK) return s;
  if (!b->dout || !b->dq || !b->dk || !b->dv || !b->workspace)
    return fail(CSA_INVALID_ARG, "csa_seq_attn_bwd: null pointer");
  if (!aligned(b->dout, 16) || !aligned(b->dq, 16) || !aligned(b->dk, 16) || !aligned(b->dv, 16) || !aligned(b->workspace, 4))
    return fail(CSA_INVALID_ARG, "csa_seq_attn_bwd: dout, dq, dk, dv must be 16-byte aligned");
  if (!strides_ok(b->dq_sr, b->dq_sh, b->dq_st) || !strides_ok(b->dk_sb, b->dk_sh, b->dk_sn) ||
      !strides_ok(b->dv_sb, b->dv_sh, b->dv_sn))
    return fail(CSA_INVALID_ARG, "csa_seq_attn_bwd: strides must be non-negative multiples of 4 elements");
  d.dout = b->dout; d.dsum = (float*)b->workspace;
  d.dq = b->dq; d.dq_sr = b->dq_sr; d.dq_sh = b->dq_sh; d.dq_st = b->dq_st;
  d.dk = b->dk; d.dk_sb = b->dk_sb; d.dk_sh = b->dk_sh; d.dk_sn = b->dk_sn;
  d.dv = b->dv; d.dv_sb = b->dv_sb; d.dv_sh = b->dv_sh; d.dv_sn = b->dv_sn;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  const dim3 gq((unsigned)(a->R * a->H * ((a->T + TILE - 1) / TILE)));
  const dim3 gk((unsigned)((a->R / a->kv_group) * a->H * ((a->S + TILE - 1) / TILE)));
  if (a->hd == 64) {
    hipLaunchKernelGGL(k_seq_attn_bwd_q<64>, gq, dim3(64), 0, st, d);
    hipLaunchKernelGGL(k_seq_attn_bwd_kv<64>, gk, dim3(64), 0, st, d);
  } else {
    hipLaunchKernelGGL(k_seq_attn_bwd_q<8>, gq, dim3(64), 0, st, d);
    hipLaunchKernelGGL(k_seq_attn_bwd_kv<8>, gk, dim3(64), 0, st, d);
  }
  return launched("csa_seq_attn_bwd");
}

}  // extern "C"
