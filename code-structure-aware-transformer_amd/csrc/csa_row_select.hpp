// Device helpers shared by the row kernels that pick tokens from a row of logits (csa_beam.hip, csa_sample.hip):
// the (value, index) order of their selections and the merge of their online log-sum-exp partials.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace csa {

constexpr int NO_IDX = 0x7fffffff;  // "no entry": loses every tie against a real index

// (v, i) comes before (vo, io): the larger value, then the lower index
__device__ __forceinline__ bool ahead(float v, int i, float vo, int io) { return v > vo || (v == vo && i < io); }

// (m, s) <- the online (max, sum exp) of the union of (m, s) and (mo, so); a side with m = -inf holds nothing
__device__ __forceinline__ void lse_merge(float& m, float& s, float mo, float so) {
  const float mn = fmaxf(m, mo);
  const float a = (m > -INFINITY) ? s * expf(m - mn) : 0.f;
  const float b = (mo > -INFINITY) ? so * expf(mo - mn) : 0.f;
  m = mn;
  s = a + b;
}

}  // namespace csa
