// Sampled decoding on top of the KV-cached, device-stepped decode step (csa_decode.hip): the one kernel of a sampling
// step that is neither a GEMM nor the attention.
//
//   k_sample_rows  per row r of the (R, V) last-position logits z, at the step t held in the device counter:
//                  y = fl32(z * inv_temperature); top-k (all ties at the k-th largest value stay); top-p on the softmax
//                  of the top-k set (a class of equal values stays while the mass of the strictly larger values is below
//                  top_p); one Gumbel-max draw over what is left, token = argmax fl32(y + g), lowest index first, with
//                  g = -log(-log u) from Philox4x32-7 stream RNG_SAMPLE; logp = y[token] - lse(y over the kept set).
//                  Writes ys[r, t+1], pad[r, t+1], logp[r, t] and fin[r] in place; a finished row takes PAD and logp 0.
//
// One workgroup of 256 threads per row, fp32, wave64. Thread i owns the column quads i, i + 256, ... (columns 4q .. 4q+3)
// whatever V and the base address are: 16-byte loads when V % 4 == 0, the row stride is a multiple of 4 and the base is
// 16-byte aligned, the same four columns one by one otherwise, so results do not depend on where the logits lie. One
// Philox call serves a quad. Every float reduction has a fixed order (per-thread partial, xor butterfly inside the
// wave, then the waves in index order); the only atomics are integer counts in LDS. Nothing allocates or syncs.
//
// Without a filter (top_k == 0 and top_p >= 1) the row is read once: online (max, sum exp) and the noisy arg-max.
// With a filter the row is re-read from L2 per pass (at most 128 KiB, read by the one workgroup that just missed on
// it), never staged in LDS, so LDS stays at 1.3 KiB and occupancy is set by registers alone:
//   pass 0         the maximum m and the number of candidates (entries that are neither -inf nor NaN);
//   top-k          4 passes of radix descent on the order-preserving integer image of y, 8 bits per pass: integer LDS
//                  histogram of the digit among the entries that share the prefix found so far, a suffix scan over
//                  the 256 buckets (one per thread), the bucket holding the k-th largest becomes the next digit;
//   top-p          8 passes, 4 bits per pass: per-thread register histograms of exp(y - m) by digit (16 floats, compile-
//                  time indices), reduced in the fixed order; walking the buckets downwards from the mass A of everything
//                  above the prefix, the lowest non-empty bucket whose start is still below top_p * Z holds the boundary
//                  class. Entries off the prefix cost a load and a compare, so the deeper passes are cheap;
//   draw           sum exp over the kept set and the noisy arg-max.
#include "csa_common.hpp"
#include "csa_row_select.hpp"
#include "../../include/csa_hip.h"

#include <math.h>

using namespace csa;

namespace {

constexpr int SAMPLE_THREADS = 256;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr int SAMPLE_MAX_V = 32768;
constexpr uint32_t RNG_SAMPLE = 7u;

struct SampArgs {
  const float* z; int64_t z_s; int V;
  int64_t* ys; int64_t ys_s;
  uint8_t* pad; int64_t pad_s;
  float* logp; int64_t logp_s;
  int T;
  uint8_t* fin;
  float inv, top_p;
  int top_k;
  int64_t eos_id, pad_id;
  const uint64_t* rng;
  const int32_t* t_dev;
};

__device__ __forceinline__ bool is_cand(float y) { return y > -INFINITY; }  // neither -inf nor NaN

// order-preserving integer image of a candidate: a < b <=> okey(a) < okey(b), with -0 and +0 on one key
__device__ __forceinline__ uint32_t okey(float y) {
  const uint32_t u = __float_as_uint(y + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// u = ((w >> 9) + 0.5) 2^-23 in (0, 1), exact in fp32; g = -log(-log u)
__device__ __forceinline__ float gumbel(uint32_t w) {
  const float u = ((float)(w >> 9) + 0.5f) * (1.0f / 8388608.0f);
  return -logf(-logf(u));
}

// One pass over the row: f(y, c) for each of the thread's quads, y[e] = fl32(z[c + e] * inv), columns at or past V
// reading as -inf (never candidates). The loads of QUAD_BATCH quads are issued before the first is used: a pass is a
// few round trips to L2, not one per quad. Every load is unconditional on a clamped address and only the value is
// selected (a branch around a load would make the compiler drain the loads in flight).
// __fmul_rn: the product is rounded on its own, never contracted into the add of the Gumbel noise.
constexpr int QUAD_BATCH = 8;

template <bool VEC, class F>
__device__ __forceinline__ void quad_pass(const float* __restrict__ zr, int V, float inv, int tid, F&& f) {
  for (int c0 = 4 * tid; c0 < V; c0 += 4 * SAMPLE_THREADS * QUAD_BATCH) {
    float y[QUAD_BATCH][4];
#pragma unroll
    for (int u = 0; u < QUAD_BATCH; ++u) {
      const int c = c0 + u * 4 * SAMPLE_THREADS;
      f32x4 q;
      if (VEC) {  // V % 4 == 0 and V >= 4: the row's last quad is always there
        q = *reinterpret_cast<const f32x4*>(zr + (c < V ? c : V - 4));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = zr[c + e < V ? c + e : V - 1];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) y[u][e] = (c + e < V) ? __fmul_rn(q[e], inv) : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < QUAD_BATCH; ++u) {
      const int c = c0 + u * 4 * SAMPLE_THREADS;
      if (c < V) f(y[u], c);
    }
  }
}

template <class F>
__device__ __forceinline__ void for_each_quad(const float* __restrict__ zr, int V, bool vec, float inv, int tid, F&& f) {
  if (vec) quad_pass<true>(zr, V, inv, tid, f);
  else quad_pass<false>(zr, V, inv, tid, f);
}

// No noise exceeds G_MAX: u <= 1 - 2^-24 gives g <= -log(2^-24 (1 + 2^-25 ...)) < 16.64.
constexpr float G_MAX = 16.7f;

// the noisy arg-max of one quad: (bs, bi) <- the better of itself and the kept entries' y + g. An entry with
// fl(y + G_MAX) < bs is passed over: rounding is monotone, so fl(y + g) <= fl(y + G_MAX) < bs could neither replace
// the thread's best nor tie with the row's; the result is bitwise the one without this test.
__device__ __forceinline__ void draw_quad(const float* y, bool* keep, int c, uint32_t row, uint32_t t, uint32_t c3,
                                          uint32_t k0, uint32_t k1, float& bs, int& bi) {
  if (bi != NO_IDX) {
#pragma unroll
    for (int e = 0; e < 4; ++e) keep[e] = keep[e] && !(y[e] + G_MAX < bs);
  }
  if (!(keep[0] || keep[1] || keep[2] || keep[3])) return;
  const u32x4 w = philox4x32(u32x4{(uint32_t)c >> 2, row, t, c3}, k0, k1);
  const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (keep[e]) {
      const float sc = y[e] + gumbel(ww[e]);
      if (bi == NO_IDX || sc > bs) { bs = sc; bi = c + e; }  // ascending columns: the lowest index stays on a tie
    }
  }
}

template <bool FILTER>
__global__ __launch_bounds__(SAMPLE_THREADS) void k_sample_rows(const SampArgs a) {
  const int t = *a.t_dev;
  if (t < 0 || t >= a.T - 1) return;  // one value for the whole grid, before any barrier
  __shared__ float shf[SAMPLE_WAVES * 16];
  __shared__ int shi[SAMPLE_WAVES + 4];
  __shared__ int hist[FILTER ? 256 : 1];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (a.fin[row]) {  // the workgroup's own row: uniform, before any barrier
    if (tid == 0) {
      a.ys[row * a.ys_s + t + 1] = a.pad_id;
      a.pad[row * a.pad_s + t + 1] = 1;
      if (a.logp) a.logp[row * a.logp_s + t] = 0.f;
    }
    return;
  }
  const float* zr = a.z + row * a.z_s;
  const int V = a.V;
  const bool vec = (V % 4 == 0) && (a.z_s % 4 == 0) && ((((uintptr_t)a.z) & 15) == 0);
  const float inv = a.inv;
  const uint64_t seed = a.rng[0], offset = a.rng[1];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c3 = (RNG_SAMPLE << 28) ^ (uint32_t)offset;

  float m = -INFINITY, s = 0.f, bs = -INFINITY;
  int bi = NO_IDX;
  const uint32_t urow = (uint32_t)row, ut = (uint32_t)t;

  if (!FILTER) {
    for_each_quad(zr, V, vec, inv, tid, [&](const float* y, int c) {
      bool keep[4];
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        keep[e] = is_cand(y[e]);
        if (keep[e]) mx = fmaxf(mx, y[e]);
      }
      if (mx > m) {
        s = (m > -INFINITY) ? s * expf(m - mx) : 0.f;
        m = mx;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (keep[e]) s += expf(y[e] - m);
      draw_quad(y, keep, c, urow, ut, c3, k0, k1, bs, bi);
    });
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float mo = __shfl_xor(m, o, 64);
      const float so = __shfl_xor(s, o, 64);
      lse_merge(m, s, mo, so);
    }
    if (lane == 0) { shf[wave] = m; shf[SAMPLE_WAVES + wave] = s; }
    __syncthreads();
    m = shf[0];
    s = shf[SAMPLE_WAVES];
#pragma unroll
    for (int k = 1; k < SAMPLE_WAVES; ++k) lse_merge(m, s, shf[k], shf[SAMPLE_WAVES + k]);
    __syncthreads();
  } else {
    // ---- pass 0: the maximum and the number of candidates ----
    int ncand = 0;
    for_each_quad(zr, V, vec, inv, tid, [&](const float* y, int) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (is_cand(y[e])) { m = fmaxf(m, y[e]); ++ncand; }
    });
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      m = fmaxf(m, __shfl_xor(m, o, 64));
      ncand += __shfl_xor(ncand, o, 64);
    }
    if (lane == 0) { shf[wave] = m; shi[wave] = ncand; }
    __syncthreads();
    m = fmaxf(fmaxf(shf[0], shf[1]), fmaxf(shf[2], shf[3]));
    ncand = shi[0] + shi[1] + shi[2] + shi[3];
    __syncthreads();

    uint32_t thr = 0;  // kept: candidates whose key is at least thr
    if (ncand > 0) {   // uniform over the workgroup
      // ---- top-k: the key of the k-th largest candidate, 8 bits per pass ----
      if (a.top_k > 0 && a.top_k < ncand) {
        int krem = a.top_k;
        for (int shift = 24; shift >= 0; shift -= 8) {
          hist[tid] = 0;
          __syncthreads();
          for_each_quad(zr, V, vec, inv, tid, [&](const float* y, int) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (is_cand(y[e])) {
                const uint32_t k = okey(y[e]);
                if (shift == 24 || ((k ^ thr) >> (shift + 8)) == 0) atomicAdd(&hist[(k >> shift) & 255u], 1);
              }
            }
          });
          __syncthreads();
          // thread i holds bucket 255 - i: an inclusive scan over the threads counts from the largest digit down
          const int cnt = hist[255 - tid];
          int incl = cnt;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
          }
          if (lane == 63) shi[wave] = incl;
          __syncthreads();
          for (int w = 0; w < wave; ++w) incl += shi[w];
          const int excl = incl - cnt;
          if (excl < krem && krem <= incl) {  // exactly one thread: 1 <= krem <= the entries on the prefix
            shi[SAMPLE_WAVES] = 255 - tid;
            shi[SAMPLE_WAVES + 1] = krem - excl;
          }
          __syncthreads();
          thr |= (uint32_t)shi[SAMPLE_WAVES] << shift;
          krem = shi[SAMPLE_WAVES + 1];
        }
        __syncthreads();
      }
      // ---- top-p: the key of the last class whose strictly-larger mass is below top_p, 4 bits per pass ----
      if (a.top_p < 1.f) {
        const uint32_t theta = thr;
        uint32_t pre = 0;
        float A = 0.f, P = 0.f;
        for (int shift = 28; shift >= 0; shift -= 4) {
          float h[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) h[u] = 0.f;
          uint32_t seen = 0;
          for_each_quad(zr, V, vec, inv, tid, [&](const float* y, int) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (is_cand(y[e])) {
                const uint32_t k = okey(y[e]);
                if (k >= theta && (shift == 28 || ((k ^ pre) >> (shift + 4)) == 0)) {
                  const uint32_t d = (k >> shift) & 15u;
                  const float ev = expf(y[e] - m);
                  seen |= 1u << d;
#pragma unroll
                  for (int u = 0; u < 16; ++u) h[u] += ((uint32_t)u == d) ? ev : 0.f;
                }
              }
            }
          });
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
            for (int u = 0; u < 16; ++u) h[u] += __shfl_xor(h[u], o, 64);
            seen |= __shfl_xor(seen, o, 64);
          }
          if (lane == 0) {
#pragma unroll
            for (int u = 0; u < 16; ++u) shf[wave * 16 + u] = h[u];
            shi[wave] = (int)seen;
          }
          __syncthreads();
          seen = (uint32_t)(shi[0] | shi[1] | shi[2] | shi[3]);
#pragma unroll
          for (int u = 0; u < 16; ++u) h[u] = ((shf[u] + shf[16 + u]) + shf[32 + u]) + shf[48 + u];
          if (shift == 28) {  // Z, the mass of the whole top-k set, largest bucket first
            float Z = 0.f;
#pragma unroll
            for (int u = 15; u >= 0; --u) Z += h[u];
            P = a.top_p * Z;
          }
          // every thread walks the same 16 totals: the first non-empty bucket starts at A < P (it held the boundary
          // one level up; the maximal class at the top), and the start only grows on the way down
          int sel = seen ? 31 - __clz(seen) : 0;
          float run = A, Asel = A;
#pragma unroll
          for (int u = 15; u >= 0; --u) {
            if (((seen >> u) & 1u) && run < P) { sel = u; Asel = run; }
            run += h[u];
          }
          A = Asel;
          pre |= (uint32_t)sel << shift;
          __syncthreads();  // shf / shi are rewritten by the next pass
        }
        thr = pre > theta ? pre : theta;
      }
      // ---- the draw over the kept set ----
      for_each_quad(zr, V, vec, inv, tid, [&](const float* y, int c) {
        bool keep[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          keep[e] = is_cand(y[e]) && okey(y[e]) >= thr;
          if (keep[e]) s += expf(y[e] - m);
        }
        draw_quad(y, keep, c, urow, ut, c3, k0, k1, bs, bi);
      });
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
      if (lane == 0) shf[wave] = s;
      __syncthreads();
      s = ((shf[0] + shf[1]) + shf[2]) + shf[3];
      __syncthreads();
    }
  }

  // ---- the workgroup's arg-max of the noisy scores ----
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float vo = __shfl_xor(bs, o, 64);
    const int io = __shfl_xor(bi, o, 64);
    if (io != NO_IDX && (bi == NO_IDX || ahead(vo, io, bs, bi))) { bs = vo; bi = io; }
  }
  if (lane == 0) { shf[wave] = bs; shi[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < SAMPLE_WAVES; ++k) {
      const float vo = shf[k];
      const int io = shi[k];
      if (io != NO_IDX && (bi == NO_IDX || ahead(vo, io, bs, bi))) { bs = vo; bi = io; }
    }
    int64_t tok = 0;
    float lp = -INFINITY;  // a row with no candidate: index 0, logp -inf
    if (bi != NO_IDX) {
      tok = bi;
      lp = __fmul_rn(zr[bi], inv) - (m + logf(s));
    }
    a.ys[row * a.ys_s + t + 1] = tok;
    a.pad[row * a.pad_s + t + 1] = (tok == a.pad_id) ? 1 : 0;
    if (a.logp) a.logp[row * a.logp_s + t] = lp;
    if (tok == a.eos_id) a.fin[row] = 1;
  }
}

}  // namespace

extern "C" {

int csa_sample_rows_supported(int64_t V) { return (V >= 1 && V <= SAMPLE_MAX_V) ? 1 : 0; }

csa_status csa_sample_rows(const csa_sample_rows_args* a, void* stream) {
  if (!a) return fail(CSA_INVALID_ARG, "csa_sample_rows: null args");
  if (!csa_sample_rows_supported(a->V)) return fail(CSA_UNSUPPORTED_SHAPE, "csa_sample_rows: V must be in [1, 32768]");
  if (a->rows < 0 || a->rows > 0x7fffffff || a->T < 2 || a->T > 0x7fffffff)
    return fail(CSA_INVALID_ARG, "csa_sample_rows: bad rows or T (T >= 2)");
  if (!(a->inv_temperature > 0.f) || !(a->inv_temperature < INFINITY))
    return fail(CSA_INVALID_ARG, "csa_sample_rows: the temperature must be positive (inv_temperature in (0, inf))");
  if (!(a->top_p > 0.f)) return fail(CSA_INVALID_ARG, "csa_sample_rows: top_p must be positive (>= 1 turns it off)");
  if (a->top_k < 0 || a->top_k > 0x7fffffff)
    return fail(CSA_INVALID_ARG, "csa_sample_rows: top_k must not be negative (0 turns it off)");
  if (a->logits_stride < a->V || a->ys_stride < a->T || a->pad_stride < a->T || (a->logp && a->logp_stride < a->T - 1))
    return fail(CSA_INVALID_ARG, "csa_sample_rows: a row stride below V (logits), T (ys, pad) or T - 1 (logp)");
  if (!a->logits || !a->ys || !a->pad || !a->fin || !a->rng_dev || !a->t_dev)
    return fail(CSA_INVALID_ARG, "csa_sample_rows: null pointer");
  if (!aligned(a->logits, 4) || !aligned(a->ys, 8) || !aligned(a->logp, 4) || !aligned(a->rng_dev, 8) ||
      !aligned(a->t_dev, 4))
    return fail(CSA_INVALID_ARG, "csa_sample_rows: misaligned pointer (tokens and rng 8, the fp32 / int32 arrays 4 bytes)");
  if (a->rows == 0) return CSA_OK;
  SampArgs d;
  d.z = a->logits; d.z_s = a->logits_stride; d.V = (int)a->V;
  d.ys = a->ys; d.ys_s = a->ys_stride;
  d.pad = a->pad; d.pad_s = a->pad_stride;
  d.logp = a->logp; d.logp_s = a->logp_stride;
  d.T = (int)a->T;
  d.fin = a->fin;
  d.inv = a->inv_temperature; d.top_p = a->top_p; d.top_k = (int)a->top_k;
  d.eos_id = a->eos_id < 0 ? -1 : a->eos_id;
  d.pad_id = a->pad_id;
  d.rng = a->rng_dev;
  d.t_dev = a->t_dev;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  if (a->top_k > 0 || a->top_p < 1.f)
    hipLaunchKernelGGL(k_sample_rows<true>, dim3((unsigned)a->rows), dim3(SAMPLE_THREADS), 0, st, d);
  else
    hipLaunchKernelGGL(k_sample_rows<false>, dim3((unsigned)a->rows), dim3(SAMPLE_THREADS), 0, st, d);
  return launched("csa_sample_rows");
}

}  // extern "C"
