// Log-probability of one given token per row of fp32 logits, fused (the scorer of given summaries):
//
//   logp[r] = z[r, t_r] - lse_r,  lse_r = m_r + log sum_j exp(z[r, j] - m_r),  m_r = max_j z[r, j]
//
// a true log-softmax at the target column (never log(softmax), which underflows to -inf), without ever writing the
// (rows, V) log-probabilities that log_softmax + gather materialise, save and read again. The backward is
//
//   dz[r, j] = g[r] * ([j == t_r] - exp(z[r, j] - lse_r))
//
// straight from the saved logits and the row's two statistics.
//
// lse_r is kept as the unevaluated pair {m_r, log S_r} (8 bytes per row): one fp32 m_r + log S_r would round at the
// size of m_r, and exp(z - lse) would inherit that as a relative error (5e-4 at |z| ~ 1e4). With the pair, the forward
// forms (z_t - m) - log S and the backward exp((z - m) - log S), both at the accuracy of the small differences.
//
// Forward launch classes are those of csa_gen.hip (one workgroup per row, a lane owns groups of 8 consecutive columns,
// two dwordx4 loads per group when the ROW's base address is 16-byte aligned, scalar loads otherwise):
//   r<NG>, NG = 1..6: 512 threads, the row stays in registers (NG groups per lane), V <= 4096 * NG:
//                     thresholds 4096, 8192, 12288, 16384, 20480, 24576; the max is taken before any exp and every
//                     element is read once;
//   stream:           V > 24576: 256 threads, a max pass and a sum pass over the row (the second from L2).
// The reductions are wave shuffles, then one LDS slot per wave, summed in a fixed order: deterministic, no atomics.
// The target's logit is one extra scalar load by thread 0.
//
// The backward needs no row reduction, so it has no classes: one workgroup of 512 threads per (row, slab of 4096
// columns), a lane reads its 8 logits, then writes its 8 gradients. Every element is read by the lane that writes
// it and before it is written, which is what lets dz alias logits.
#include "csa_common.hpp"
#include "../../include/csa_hip.h"

#include <math.h>

using namespace csa;

namespace {

constexpr int RT = 512;                 // register classes and the backward
constexpr int ST = 256;                 // streaming forward
constexpr int MAX_NG = 6;
constexpr int64_t SLAB = 8 * (int64_t)RT;    // columns per workgroup of a register group / of the backward
constexpr int64_t MAX_V = (int64_t)1 << 24;  // 4096 backward slabs per row (gridDim.y)

struct TlpArgs {
  const float* z; int64_t ld;
  const int64_t* target;
  int64_t rows, V, ignore_id;
  float* logp; float* lse;   // lse: (rows, 2) = {max, log sum}
};

struct TlpBwdArgs {
  const float* g; const float* z; int64_t ld;
  const int64_t* target; const float* lse;
  float* dz; int64_t dz_ld;
  int64_t rows, V, ignore_id;
};

// 8 values of group gi of a row (zero beyond V)
__device__ __forceinline__ void load8(const float* row, int64_t V, int64_t gi, bool vec, float* v) {
  const int64_t c0 = 8 * gi;
  if (vec && c0 + 8 <= V) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(row + c0);
    const f32x4 b = *reinterpret_cast<const f32x4*>(row + c0 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (c0 + e < V) ? row[c0 + e] : 0.f;
  }
}

__device__ __forceinline__ bool scored(int64_t t, const int64_t V, const int64_t ignore_id) {
  return t != ignore_id && t >= 0 && t < V;
}

template <int NT>
__device__ __forceinline__ float block_max(float m, float* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = red[0];
#pragma unroll
  for (int i = 1; i < NT / 64; ++i) m = fmaxf(m, red[i]);
  return m;
}

template <int NT>
__device__ __forceinline__ float block_sum(float s, float* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  s = red[0];
#pragma unroll
  for (int i = 1; i < NT / 64; ++i) s += red[i];
  return s;
}

// thread 0 of the row's workgroup: the row's outputs from its max m and sum S = sum exp(z - m)
__device__ __forceinline__ void finish_row(const TlpArgs& a, int64_t row, const float* zr, float m, float S) {
  const int64_t t = a.target[row];
  const bool ok = scored(t, a.V, a.ignore_id);
  const float zt = zr[ok ? t : 0];
  const float ls = logf(S);
  a.logp[row] = ok ? (zt - m) - ls : 0.f;
  a.lse[2 * row] = m;
  a.lse[2 * row + 1] = ls;
}

// fmaxf drops a NaN, so m is the max of the row's other entries (-inf when there are none) and the NaN reaches S
// through exp(NaN - m); an all -inf row gives exp(-inf + inf) = NaN as well, as torch.log_softmax does.
template <int NG>
__global__ __launch_bounds__(RT) void k_token_logp_fwd_r(const TlpArgs a) {
  __shared__ float red_m[RT / 64], red_s[RT / 64];
  const int64_t row = blockIdx.x;
  const float* zr = a.z + row * a.ld;
  const bool vec = (((uintptr_t)zr) & 15) == 0;
  const int64_t ng = (a.V + 7) / 8;
  float x[NG][8];
#pragma unroll
  for (int q = 0; q < NG; ++q) {
    const int64_t gi = threadIdx.x + (int64_t)q * RT;
    load8(zr, a.V, gi < ng ? gi : 0, vec, x[q]);
  }
  float m = -INFINITY;
#pragma unroll
  for (int q = 0; q < NG; ++q) {
    const int64_t gi = threadIdx.x + (int64_t)q * RT;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool in = gi < ng && 8 * gi + e < a.V;
      x[q][e] = in ? x[q][e] : -INFINITY;
      m = fmaxf(m, x[q][e]);
    }
  }
  m = block_max<RT>(m, red_m);
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < NG; ++q) {
    const int64_t gi = threadIdx.x + (int64_t)q * RT;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool in = gi < ng && 8 * gi + e < a.V;
      s += in ? expf(x[q][e] - m) : 0.f;  // selected, not exp(-inf - m): m may be -inf
    }
  }
  s = block_sum<RT>(s, red_s);
  if (threadIdx.x == 0) finish_row(a, row, zr, m, s);
}

__global__ __launch_bounds__(ST) void k_token_logp_fwd_s(const TlpArgs a) {
  __shared__ float red_m[ST / 64], red_s[ST / 64];
  const int64_t row = blockIdx.x;
  const float* zr = a.z + row * a.ld;
  const bool vec = (((uintptr_t)zr) & 15) == 0;
  const int64_t ng = (a.V + 7) / 8;
  float m = -INFINITY;
  for (int64_t gi = threadIdx.x; gi < ng; gi += ST) {
    float v[8];
    load8(zr, a.V, gi, vec, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, 8 * gi + e < a.V ? v[e] : -INFINITY);
  }
  m = block_max<ST>(m, red_m);
  float s = 0.f;
  for (int64_t gi = threadIdx.x; gi < ng; gi += ST) {
    float v[8];
    load8(zr, a.V, gi, vec, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += 8 * gi + e < a.V ? expf(v[e] - m) : 0.f;
  }
  s = block_sum<ST>(s, red_s);
  if (threadIdx.x == 0) finish_row(a, row, zr, m, s);
}

// z and dz are not __restrict__: they may be the same buffer
__global__ __launch_bounds__(RT) void k_token_logp_bwd(const TlpBwdArgs a) {
  const int64_t row = blockIdx.x;
  const int64_t gi = (int64_t)blockIdx.y * RT + threadIdx.x;
  const int64_t c0 = 8 * gi;
  if (c0 >= a.V) return;
  const float* zr = a.z + row * a.ld;
  float* out = a.dz + row * a.dz_ld;
  const bool vec = ((((uintptr_t)zr) | ((uintptr_t)out)) & 15) == 0;
  const int64_t t = a.target[row];
  const bool ok = scored(t, a.V, a.ignore_id);
  float o[8];
  if (ok) {
    const float m = a.lse[2 * row], ls = a.lse[2 * row + 1], gr = a.g[row];
    float v[8];
    load8(zr, a.V, gi, vec, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = gr * ((c0 + e == t ? 1.f : 0.f) - expf((v[e] - m) - ls));
  } else {  // an ignored row: zeros whatever g[r] holds
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
  }
  if (vec && c0 + 8 <= a.V) {
    *reinterpret_cast<f32x4*>(out + c0) = f32x4{o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4*>(out + c0 + 4) = f32x4{o[4], o[5], o[6], o[7]};
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (c0 + e < a.V) out[c0 + e] = o[e];
  }
}

// groups per lane of the register classes (1..6), 0 = the streaming kernel
inline int reg_groups(int64_t V) {
  const int64_t per = (V + SLAB - 1) / SLAB;
  return per <= MAX_NG ? (int)per : 0;
}

// CSA_OK with *launch = false: nothing to do
csa_status check_shape(const char* fn, int64_t rows, int64_t V, int64_t ld, int64_t dz_ld, bool* launch) {
  *launch = false;
  if (rows < 0 || V < 0 || rows > 0x7fffffff) return fail(CSA_INVALID_ARG, fn);
  if (rows == 0 || V == 0) return CSA_OK;
  if (ld < V || dz_ld < V) return fail(CSA_INVALID_ARG, fn);
  if (!csa_token_logp_supported(V)) return fail(CSA_UNSUPPORTED_SHAPE, fn);
  *launch = true;
  return CSA_OK;
}

}  // namespace

extern "C" {

int csa_token_logp_supported(int64_t V) { return (V >= 1 && V <= MAX_V) ? 1 : 0; }

csa_status csa_token_logp_fwd(const float* logits, int64_t ld, const int64_t* target, int64_t rows, int64_t V,
                              int64_t ignore_id, float* logp, float* lse, void* stream) {
  bool launch;
  const csa_status s = check_shape("csa_token_logp_fwd: bad rows / V / ld", rows, V, ld, ld, &launch);
  if (s != CSA_OK || !launch) return s;
  if (!logits || !target || !logp || !lse) return fail(CSA_INVALID_ARG, "csa_token_logp_fwd: null pointer");
  if (!aligned(logits, 4) || !aligned(target, 8) || !aligned(logp, 4) || !aligned(lse, 4))
    return fail(CSA_INVALID_ARG, "csa_token_logp_fwd: misaligned pointer");
  const TlpArgs a{logits, ld, target, rows, V, ignore_id, logp, lse};
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  const dim3 grid((unsigned)rows);
  switch (reg_groups(V)) {
    case 1: hipLaunchKernelGGL(k_token_logp_fwd_r<1>, grid, dim3(RT), 0, st, a); break;
    case 2: hipLaunchKernelGGL(k_token_logp_fwd_r<2>, grid, dim3(RT), 0, st, a); break;
    case 3: hipLaunchKernelGGL(k_token_logp_fwd_r<3>, grid, dim3(RT), 0, st, a); break;
    case 4: hipLaunchKernelGGL(k_token_logp_fwd_r<4>, grid, dim3(RT), 0, st, a); break;
    case 5: hipLaunchKernelGGL(k_token_logp_fwd_r<5>, grid, dim3(RT), 0, st, a); break;
    case 6: hipLaunchKernelGGL(k_token_logp_fwd_r<6>, grid, dim3(RT), 0, st, a); break;
    default: hipLaunchKernelGGL(k_token_logp_fwd_s, grid, dim3(ST), 0, st, a);
  }
  return launched("csa_token_logp_fwd");
}

csa_status csa_token_logp_bwd(const float* g, const float* logits, int64_t ld, const int64_t* target, const float* lse,
                              float* dz, int64_t dz_ld, int64_t rows, int64_t V, int64_t ignore_id, void* stream) {
  bool launch;
  const csa_status s = check_shape("csa_token_logp_bwd: bad rows / V / ld", rows, V, ld, dz_ld, &launch);
  if (s != CSA_OK || !launch) return s;
  if (!g || !logits || !target || !lse || !dz) return fail(CSA_INVALID_ARG, "csa_token_logp_bwd: null pointer");
  if (!aligned(g, 4) || !aligned(logits, 4) || !aligned(target, 8) || !aligned(lse, 4) || !aligned(dz, 4))
    return fail(CSA_INVALID_ARG, "csa_token_logp_bwd: misaligned pointer");
  if (dz == logits && dz_ld != ld) return fail(CSA_INVALID_ARG, "csa_token_logp_bwd: in place needs dz_ld == ld");
  const TlpBwdArgs a{g, logits, ld, target, lse, dz, dz_ld, rows, V, ignore_id};
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  const dim3 grid((unsigned)rows, (unsigned)((V + SLAB - 1) / SLAB));
  hipLaunchKernelGGL(k_token_logp_bwd, grid, dim3(RT), 0, st, a);
  return launched("csa_token_logp_bwd");
}

}  // extern "C"
