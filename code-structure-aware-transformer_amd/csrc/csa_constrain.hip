// Decoding constraints on top of the KV-cached, device-stepped decode step (csa_decode.hip): the one kernel that says
// which tokens a step may choose. It rewrites the (R, V) last-position logits in place, after generator.linear and in
// front of whichever selection follows (k_argmax_rows_step, k_beam_row_topk, k_sample_rows), which then see a banned
// token as a plain -inf logit.
//
//   k_constrain_rows  per row r at the step t (device counter, or the host value), history h[0..L) = ys[r, 0..t],
//                     L = t + 1, the literal token columns:
//                     penalty   theta != 1: every distinct in-range token v of h, once: z_v = z_v > 0 ? z_v / theta
//                               : z_v * theta, each one correctly rounded fp32 operation;
//                     n-gram    n >= 1: every i <= L - n whose n - 1 tokens h[i ..] equal the last n - 1 tokens of h
//                               bans h[i + n - 1];
//                     length    eos_id is banned while t < min_length;
//                     list      every in-range id of the suppress list is banned.
//                     A ban stores -inf. A finished row, or a t outside [0, T - 1), is left alone.
//
// One workgroup of 256 threads per row, fp32, wave64. The history is staged once into LDS as the int64 it is (8 KiB at
// the T = 1024 limit), so an id outside [0, V) still takes part in every comparison and is only never used as a column.
// Thread i owns the positions i, i + 256, ...: a position is the first occurrence of its token when no earlier position
// holds the same one (a scan over LDS in which the lanes of a wave read one address), and only a first occurrence does
// the penalty's read-modify-write, so no two threads touch one address in that phase. The bans follow a workgroup
// barrier: __syncthreads() is a workgroup-scope release, the barrier and a workgroup-scope acquire over global memory
// too, so every penalty store happens before every ban and a ban that hits a penalised column wins (the workgroup sits
// on one CU, whose L1 takes its waves' vector memory operations in order: the fence needs no wait of its own and the
// compiler emits none). Several bans of one column store the same -inf. Nothing else in the row is read or
// written: at most L + 1 + n_suppress scattered 4-byte accesses per row, bound by latency, not bandwidth. No atomics,
// no allocation, no sync; V is not limited (columns are indexed in 64 bits).
#include "csa_common.hpp"
#include "../../include/csa_hip.h"

#include <math.h>

using namespace csa;

namespace {

constexpr int CON_THREADS = 256;
constexpr int CON_MAX_T = 1024;
constexpr int CON_MAX_SUPPRESS = 256;

struct ConArgs {
  float* z; int64_t z_s, V;
  const int64_t* ys; int64_t ys_s; int T;
  const uint8_t* fin;
  float theta;
  int64_t ngram, min_length, eos_id;
  const int32_t* suppress; int n_suppress;
  int t; const int32_t* t_dev;
};

__global__ __launch_bounds__(CON_THREADS) void k_constrain_rows(const ConArgs a) {
  const int t = a.t_dev ? *a.t_dev : a.t;
  if (t < 0 || t >= a.T - 1) return;  // one value for the whole grid, before any barrier
  const int64_t row = blockIdx.x;
  if (a.fin && a.fin[row]) return;    // the workgroup's own row: uniform, before any barrier
  __shared__ int64_t h[CON_MAX_T];
  const int tid = threadIdx.x;
  const int L = t + 1;  // <= T - 1 <= 1023
  const int64_t* yr = a.ys + row * a.ys_s;
  for (int p = tid; p < L; p += CON_THREADS) h[p] = yr[p];
  __syncthreads();
  float* zr = a.z + row * a.z_s;
  const int64_t V = a.V;

  // ---- the repetition penalty: the first occurrence of each in-range token ----
  if (a.theta != 1.f) {  // uniform
    const float theta = a.theta;
    for (int p = tid; p < L; p += CON_THREADS) {
      const int64_t v = h[p];
      if (v < 0 || v >= V) continue;
      bool first = true;
      for (int q = 0; q < p && first; ++q) first = h[q] != v;
      if (first) {
        const float x = zr[v];
        zr[v] = x > 0.f ? __fdiv_rn(x, theta) : __fmul_rn(x, theta);  // 0, -inf and NaN map to themselves
      }
    }
    __syncthreads();  // the penalty's stores precede every ban, whichever wave issues it
  }

  // ---- the bans ----
  if (a.ngram >= 1 && a.ngram <= L) {
    const int n = (int)a.ngram, s = L - (n - 1);  // h[s .. L) are the last n - 1 tokens
    for (int i = tid; i <= L - n; i += CON_THREADS) {
      bool match = true;
      for (int k = 0; k < n - 1 && match; ++k) match = h[i + k] == h[s + k];
      if (match) {
        const int64_t v = h[i + n - 1];
        if (v >= 0 && v < V) zr[v] = -INFINITY;
      }
    }
  }
  if (tid == 0 && a.eos_id >= 0 && a.eos_id < V && t < a.min_length) zr[a.eos_id] = -INFINITY;
  if (tid < a.n_suppress) {
    const int64_t v = a.suppress[tid];
    if (v >= 0 && v < V) zr[v] = -INFINITY;
  }
}

}  // namespace

extern "C" {

int csa_constrain_rows_supported(int64_t T) { return (T >= 2 && T <= CON_MAX_T) ? 1 : 0; }

csa_status csa_constrain_rows(const csa_constrain_rows_args* a, void* stream) {
  if (!a) return fail(CSA_INVALID_ARG, "csa_constrain_rows: null args");
  if (!a->logits || !a->ys) return fail(CSA_INVALID_ARG, "csa_constrain_rows: null pointer (logits, ys)");
  if (!(a->repetition_penalty > 0.f) || !(a->repetition_penalty < INFINITY))
    return fail(CSA_INVALID_ARG, "csa_constrain_rows: repetition_penalty must be in (0, inf) (1 turns it off)");
  if (a->rows < 0 || a->rows > 0x7fffffff || a->V < 0 || a->T < 0 || a->no_repeat_ngram < 0 || a->min_length < 0 ||
      a->n_suppress < 0)
    return fail(CSA_INVALID_ARG, "csa_constrain_rows: negative size (rows, V, T, no_repeat_ngram, min_length, n_suppress)");
  if (a->n_suppress > CON_MAX_SUPPRESS)
    return fail(CSA_INVALID_ARG, "csa_constrain_rows: the suppress list holds at most 256 ids");
  if (a->n_suppress > 0 && !a->suppress)
    return fail(CSA_INVALID_ARG, "csa_constrain_rows: null pointer (suppress with n_suppress > 0)");
  if (a->logits_stride < a->V || a->ys_stride < a->T)
    return fail(CSA_INVALID_ARG, "csa_constrain_rows: a row stride below V (logits) or T (ys)");
  if (!csa_constrain_rows_supported(a->T))
    return fail(CSA_UNSUPPORTED_SHAPE, "csa_constrain_rows: T must be in [2, 1024]");
  if (!aligned(a->logits, 4) || !aligned(a->ys, 8) || !aligned(a->suppress, 4) || !aligned(a->t_dev, 4))
    return fail(CSA_INVALID_ARG, "csa_constrain_rows: misaligned pointer (tokens 8, the fp32 / int32 arrays 4 bytes)");
  if (a->rows == 0 || a->V == 0) return CSA_OK;
  ConArgs d;
  d.z = a->logits; d.z_s = a->logits_stride; d.V = a->V;
  d.ys = a->ys; d.ys_s = a->ys_stride; d.T = (int)a->T;
  d.fin = a->fin;
  d.theta = a->repetition_penalty;
  d.ngram = a->no_repeat_ngram; d.min_length = a->min_length;
  d.eos_id = a->eos_id < 0 ? -1 : a->eos_id;
  d.suppress = a->suppress; d.n_suppress = (int)a->n_suppress;
  d.t = (a->t < 0 || a->t > 0x7fffffff) ? -1 : (int)a->t;  // outside every range: nothing is stored
  d.t_dev = a->t_dev;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  hipLaunchKernelGGL(k_constrain_rows, dim3((unsigned)a->rows), dim3(CON_THREADS), 0, st, d);
  return launched("csa_constrain_rows");
}

}  // extern "C"
