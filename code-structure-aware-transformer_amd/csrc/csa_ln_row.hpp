// The row path of the LayerNorm forward, shared by k_ln_fwd (csa_glue.hip) and k_decode_embed (csa_decode.hip):
// one wave holds one row in registers (CPL dwordx4 chunks per lane, lane l owns columns 4 (l + 64 q) .. + 3,
// chunks past `cols` hold zeros), two-pass mean / variance (no E[x^2] - mean^2 cancellation), then
// y = (x - mean) * rstd * gamma + beta. Every kernel that normalises a row through this function gives the same
// bits for the same row: the order of every sum is fixed here.
#pragma once
#include "csa_common.hpp"

namespace csa {

__device__ __forceinline__ float ln_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int CPL>
__device__ __forceinline__ void ln_row_fwd(const f32x4 (&v)[CPL], int lane, int cols, float eps,
                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                           float* __restrict__ yr, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < CPL; ++q) s += (v[q][0] + v[q][1]) + (v[q][2] + v[q][3]);
  mean = ln_wave_sum(s) / (float)cols;
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int c = 4 * (lane + 64 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = c < cols ? v[q][e] - mean : 0.f;
      ss = fmaf(d, d, ss);
    }
  }
  rstd = 1.f / sqrtf(ln_wave_sum(ss) / (float)cols + eps);
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int c = 4 * (lane + 64 * q);
    if (c < cols) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
      const f32x4 b = *reinterpret_cast<const f32x4*>(beta + c);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = fmaf((v[q][e] - mean) * rstd, g[e], b[e]);
      *reinterpret_cast<f32x4*>(yr + c) = o;
    }
  }
}

// chunks per lane for a row of `cols` floats: 1..4, or 0 when the row path does not take it
inline int ln_cpl(int64_t cols) {
  if (cols < 4 || cols % 4) return 0;
  const int64_t cpl = (cols + 255) / 256;
  return cpl <= 4 ? (int)cpl : 0;
}

}  // namespace csa
