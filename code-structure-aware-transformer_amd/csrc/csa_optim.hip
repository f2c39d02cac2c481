// AdamW step of script/optimizer.py:49-106 (HF-style AdamW, used with correct_bias=False by
// script/train.py:80) as ONE multi-tensor kernel on gfx950.
//
// The reference walks the parameters in Python and issues 7 elementwise ops per tensor
// (mul_, add_, mul_, addcmul_, sqrt, add_, addcdiv_ [+ add_ for weight decay]), i.e. ~200 tensors x
// 7 launches and 7 read/write passes over the optimizer state per step. Here every element is read
// once (param, grad, exp_avg, exp_avg_sq) and written once (param, exp_avg, exp_avg_sq): 28 B per
// parameter, HBM-bound.
//
// Mixed precision: GradScaler hands the optimizer its scale and found_inf as device tensors
// (_step_supports_amp_scaling), so unscaling and the skip-on-inf happen here, with no host sync.
//
// Work decomposition: each tensor is cut into CSA_ADAMW_CHUNK-element chunks; one 256-thread
// workgroup per chunk; chunk_tensor[] / chunk_start[] (built once per parameter layout by the
// caller) map a chunk to its tensor and offset without a search.
#include "csa_common.hpp"
#include "../../include/csa_hip.h"

using csa::f32x4;

namespace {

struct AdamElem {
  float b1, b2, om_b1, om_b2, eps, neg_step, neg_decay;
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamElem& c) {
  m = fmaf(c.om_b1, g, m * c.b1);               // exp_avg.mul_(beta1).add_(grad, alpha=1-beta1)
  v = fmaf(c.om_b2 * g, g, v * c.b2);           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
  const float den = __builtin_sqrtf(v) + c.eps;  // exp_avg_sq.sqrt().add_(eps)
  p = fmaf(c.neg_step, m / den, p);             // p.addcdiv_(exp_avg, denom, value=-step_size)
  p = fmaf(c.neg_decay, p, p);                  // p.add_(p, alpha=-lr*weight_decay)  (0: no-op)
}

// The gradient as the update uses it. CLIP: unscale, then scale by the clip coefficient, two fp32
// multiplies in the order of GradScaler.unscale_ followed by clip_grad_norm_.
template <bool CLIP>
__device__ __forceinline__ float used_grad(float g, float inv, float coef) {
  return CLIP ? (g * inv) * coef : g * inv;
}

// CLIP = false is the unclipped step (clip is not read). CLIP = true reads the 4-float state of
// k_grad_norm_finish: skip the step when the global norm was not finite, else clip by state[1].
template <bool CLIP>
__global__ __launch_bounds__(256) void k_adamw(const csa_adamw_tensor* __restrict__ tensors,
                                               const int32_t* __restrict__ chunk_tensor,
                                               const int64_t* __restrict__ chunk_start, AdamElem c,
                                               const float* __restrict__ grad_scale,
                                               const float* __restrict__ found_inf,
                                               const float* __restrict__ clip) {
  if (found_inf != nullptr && *found_inf != 0.f) return;  // GradScaler: skip the step on inf/NaN grads
  if (CLIP && clip[2] != 0.f) return;                     // non-finite global norm: skip likewise
  const float inv = grad_scale != nullptr ? (float)(1.0 / (double)*grad_scale) : 1.f;
  const float coef = CLIP ? clip[1] : 1.f;
  const int64_t chunk = blockIdx.x;
  const int t = chunk_tensor[chunk];
  const csa_adamw_tensor T = tensors[t];
  const int64_t base = (chunk - chunk_start[t]) * CSA_ADAMW_CHUNK;
  const int64_t rem = T.numel - base;
  const int n = (int)(rem < CSA_ADAMW_CHUNK ? rem : CSA_ADAMW_CHUNK);
  float* __restrict__ p = T.param + base;
  const float* __restrict__ g = T.grad + base;
  float* __restrict__ m = T.exp_avg + base;
  float* __restrict__ v = T.exp_avg_sq + base;
  const bool vec = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;
  if (vec) {
    for (int i = 4 * (int)threadIdx.x; i < n; i += 4 * 256) {
      if (i + 4 <= n) {
        f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
        f32x4 mv = *reinterpret_cast<const f32x4*>(m + i);
        f32x4 vv = *reinterpret_cast<const f32x4*>(v + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pe = pv[e], me = mv[e], ve = vv[e];
          adam_elem(pe, used_grad<CLIP>(gv[e], inv, coef), me, ve, c);
          pv[e] = pe; mv[e] = me; vv[e] = ve;
        }
        *reinterpret_cast<f32x4*>(p + i) = pv;
        *reinterpret_cast<f32x4*>(m + i) = mv;
        *reinterpret_cast<f32x4*>(v + i) = vv;
      } else {
        for (int e = i; e < n; ++e) adam_elem(p[e], used_grad<CLIP>(g[e], inv, coef), m[e], v[e], c);
      }
    }
  } else {
    for (int i = threadIdx.x; i < n; i += 256) adam_elem(p[i], used_grad<CLIP>(g[i], inv, coef), m[i], v[i], c);
  }
}

// ---- global gradient norm (csa_grad_sumsq + csa_grad_norm_finish) ----
// Two launches instead of one with a last-block-done counter: no atomics and no fences, and the norm
// is a pure function of the gradients (fixed summation order), so every data-parallel rank gets the
// same bits from the same averaged gradients.

// Sum of v over the 256 threads of the workgroup in a fixed order (xor tree inside each wave, then
// the four wave sums in wave order); the result is valid in thread 0.
__device__ __forceinline__ double block_sum256(double v) {
  __shared__ double wave_sum[4];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

__device__ __forceinline__ double sq64(float g) { return (double)g * (double)g; }

// One workgroup per chunk, the chunks of k_adamw: partials[chunk] = sum of g^2 over the chunk, the raw
// (still scaled) gradients squared and accumulated in fp64, so neither 1e25-sized nor GradScaler-scaled
// gradients overflow. Reads only the descriptors' grad and numel.
__global__ __launch_bounds__(256) void k_grad_sumsq(const csa_adamw_tensor* __restrict__ tensors,
                                                    const int32_t* __restrict__ chunk_tensor,
                                                    const int64_t* __restrict__ chunk_start,
                                                    double* __restrict__ partials) {
  const int64_t chunk = blockIdx.x;
  const int t = chunk_tensor[chunk];
  const int64_t base = (chunk - chunk_start[t]) * CSA_ADAMW_CHUNK;
  const int64_t rem = tensors[t].numel - base;
  const int n = (int)(rem < CSA_ADAMW_CHUNK ? rem : CSA_ADAMW_CHUNK);
  const float* __restrict__ g = tensors[t].grad + base;
  double acc = 0.0;
  if ((((uintptr_t)g) & 15) == 0) {
    for (int i = 4 * (int)threadIdx.x; i < n; i += 4 * 256) {
      if (i + 4 <= n) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += sq64(gv[e]);
      } else {
        for (int e = i; e < n; ++e) acc += sq64(g[e]);
      }
    }
  } else {
    for (int i = threadIdx.x; i < n; i += 256) acc += sq64(g[i]);
  }
  acc = block_sum256(acc);
  if (threadIdx.x == 0) partials[chunk] = acc;
}

// One workgroup: total = sum of the n partials (strided per-lane loop, then block_sum256), and the
// 4-float state {norm of the unscaled gradients, clip coefficient, norm-is-not-finite flag, 0}.
__global__ __launch_bounds__(256) void k_grad_norm_finish(const double* __restrict__ partials, int64_t n,
                                                          const float* __restrict__ grad_scale, float max_norm,
                                                          float* __restrict__ state) {
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += partials[i];
  acc = block_sum256(acc);
  if (threadIdx.x != 0) return;
  const double inv = grad_scale != nullptr ? 1.0 / (double)*grad_scale : 1.0;
  const float norm = (float)(sqrt(acc) * inv);
  const bool bad = !(fabsf(norm) <= 3.402823466e38f);  // inf or NaN
  float coef = 1.f;                                     // max_norm <= 0: measure only
  if (max_norm > 0.f && n > 0) coef = fminf(1.f, max_norm / (norm + 1e-6f));  // clip_grad_norm_'s formula
  state[0] = norm;
  state[1] = bad ? 0.f : coef;
  state[2] = bad ? 1.f : 0.f;
  state[3] = 0.f;
}

}  // namespace

extern "C" csa_status csa_grad_sumsq(const csa_grad_sumsq_args* a, void* stream) {
  if (!a) return csa::fail(CSA_INVALID_ARG, "csa_grad_sumsq: null args");
  if (a->ntensors < 0 || a->nchunks < 0 || a->nchunks > 0x7fffffff || a->first < 0)
    return csa::fail(CSA_INVALID_ARG, "csa_grad_sumsq: bad ntensors/nchunks/first");
  if (a->nchunks == 0) return CSA_OK;
  if (!a->tensors || !a->chunk_tensor || !a->chunk_start)
    return csa::fail(CSA_INVALID_ARG, "csa_grad_sumsq: null tensor table");
  if (!a->partials) return csa::fail(CSA_INVALID_ARG, "csa_grad_sumsq: null partials");
  const csa::DeviceGuard guard((hipStream_t)stream);
  hipLaunchKernelGGL(k_grad_sumsq, dim3((unsigned)a->nchunks), dim3(256), 0, (hipStream_t)stream, a->tensors,
                     a->chunk_tensor, a->chunk_start, a->partials + a->first);
  return csa::launched("csa_grad_sumsq");
}

extern "C" csa_status csa_grad_norm_finish(const double* partials, int64_t n, const float* grad_scale, float max_norm,
                                           float* state, void* stream) {
  if (!state) return csa::fail(CSA_INVALID_ARG, "csa_grad_norm_finish: null state");
  if (n < 0 || (n > 0 && !partials)) return csa::fail(CSA_INVALID_ARG, "csa_grad_norm_finish: bad n/partials");
  if (max_norm != max_norm) return csa::fail(CSA_INVALID_ARG, "csa_grad_norm_finish: max_norm is NaN");
  const csa::DeviceGuard guard((hipStream_t)stream);
  hipLaunchKernelGGL(k_grad_norm_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n, grad_scale,
                     max_norm, state);
  return csa::launched("csa_grad_norm_finish");
}

extern "C" csa_status csa_adamw_step(const csa_adamw_args* a, void* stream) {
  return csa_adamw_step_clipped(a, nullptr, stream);
}

extern "C" csa_status csa_adamw_step_clipped(const csa_adamw_args* a, const float* clip, void* stream) {
  if (!a) return csa::fail(CSA_INVALID_ARG, "csa_adamw_step: null args");
  if (a->ntensors < 0 || a->nchunks < 0 || a->nchunks > 0x7fffffff)
    return csa::fail(CSA_INVALID_ARG, "csa_adamw_step: bad ntensors/nchunks");
  if (a->nchunks == 0) return CSA_OK;
  if (!a->tensors || !a->chunk_tensor || !a->chunk_start)
    return csa::fail(CSA_INVALID_ARG, "csa_adamw_step: null tensor table");
  if (!(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f && a->eps >= 0.f))
    return csa::fail(CSA_INVALID_ARG, "csa_adamw_step: invalid beta/eps");
  AdamElem c;
  c.b1 = a->beta1; c.b2 = a->beta2; c.om_b1 = a->one_minus_beta1; c.om_b2 = a->one_minus_beta2;
  c.eps = a->eps; c.neg_step = -a->step_size; c.neg_decay = -a->decay;
  const csa::DeviceGuard guard((hipStream_t)stream);
  if (clip != nullptr)
    hipLaunchKernelGGL(k_adamw<true>, dim3((unsigned)a->nchunks), dim3(256), 0, (hipStream_t)stream, a->tensors,
                       a->chunk_tensor, a->chunk_start, c, a->grad_scale, a->found_inf, clip);
  else
    hipLaunchKernelGGL(k_adamw<false>, dim3((unsigned)a->nchunks), dim3(256), 0, (hipStream_t)stream, a->tensors,
                       a->chunk_tensor, a->chunk_start, c, a->grad_scale, a->found_inf, clip);
  return csa::launched("csa_adamw_step");
}
