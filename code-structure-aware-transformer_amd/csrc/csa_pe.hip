// Structure encodings of the use_pegen ablations (module/csa_trans.py:19-64, module/base_seq2seq.py:12-36,70-84):
// the tree positional encoding (treepos) and the Laplacian eigenvectors (laplacian). fp32 in and out, wave64.
//
//   k_tree_pos_fwd       out[r, j F + f] = pos[r, j] * w[j, f],  w[j, f] = t_f^(j / width) * s_f,  t_f = tanh(p_f),
//                        s_f = sqrt((1 - t_f^2) d_model / 2); pos (rows, depth * width), out (rows, depth * width * F).
//                        Each workgroup rebuilds the depth * F distinct weights in LDS from p: t and s in fp64, the
//                        power by repeated multiplication (so p_f = 0 gives exactly s_f at depth 0 and 0 below it),
//                        rounded to fp32 once. Then one coalesced pass over its rows.
//   k_tree_pos_bwd_part  only p has a gradient. Row-block partials of S[j, f] = sum_r pos[r, j] g[r, j F + f], summed
//                        in fp64 (an fp32 product is exact there) in row order, stored plainly to the workspace.
//   k_tree_pos_bwd_fin   one workgroup: sums the partials in block order, folds the width columns of a depth, and
//                        applies dw/dp in closed form, dp_f = (1 - t^2) sum_d S_d (pow'(t, d) s + t^d ds/dt) with
//                        torch's pow gradient (pow'(t, 0) = 0, pow'(t, 1) = 1, also at t = 0) and ds/dt = -c t / s.
//                        No atomics anywhere: two runs are bitwise equal.
//
//   k_lap_pe             one workgroup per AST. A = adj[b, :n, :n] != 0 (anything outside the block is ignored),
//                        D = row sums of A clipped below at 1, M = L + I = 2 I - D^-1/2 A D^-1/2 held column-major in
//                        LDS with an odd column stride (n = 150: 90.6 KB). M is symmetric with eigenvalues in [1, 3),
//                        so its singular value decomposition is its eigendecomposition and no vector is lost at L's
//                        zero eigenvalue. One-sided (Hestenes) Jacobi on the columns: round-robin ordering, m - 1
//                        rounds of m / 2 disjoint pairs (m = n rounded up to even; the pair holding index n is the
//                        bye), 8 lanes per pair (so one pass covers a round, and the three dot products a = |x|^2,
//                        b = |y|^2, c = x.y reduce by DPP, without the LDS crossbar), one rotation when
//                        |c| > tol sqrt(a b), one barrier per round. It stops after a sweep without a
//                        rotation; at the sweep cap it sets the AST's status word instead (no assert). Then the
//                        column norms are lambda + 1 and the normalised columns the eigenvectors, in one N x N array.
//                        Each is flipped so that its largest-magnitude entry (the first on ties, judged on the fp32
//                        values that are stored) is positive, ranked by counting (ties by column index) and scattered
//                        to pe[b, :n, :n]; the rest of pe[b] and of the eigenvalue row is written as zeros, so the
//                        caller clears nothing. Reductions are symmetric butterflies, whose result is bitwise the same
//                        in every lane that takes part and from run to run.
#include "csa_common.hpp"
#include "../../include/csa_hip.h"

#include <math.h>

using namespace csa;

namespace {

constexpr int TP_MAX_DEPTH = 64;
constexpr int TP_MAX_COLS = 1024;  // depth * width * n_feat
constexpr int TP_FWD_THREADS = 256;
constexpr int TP_FWD_ROWS = 16;
constexpr int TP_BWD_ROWS = 64;

struct TpArgs {
  const float* pos; const float* p; const float* g;
  float* out; double* ws; float* dp;
  int64_t rows;
  int depth, width, F, nblk;
  float d_model;
};

__global__ __launch_bounds__(TP_FWD_THREADS) void k_tree_pos_fwd(const TpArgs a) {
  __shared__ float pw[TP_MAX_COLS];  // [depth][F]: t_f^d * s_f
  __shared__ float w[TP_MAX_COLS];   // [depth * width][F]
  const int tid = threadIdx.x, F = a.F, C = a.depth * a.width, CF = C * F;
  for (int f = tid; f < F; f += TP_FWD_THREADS) {
    const double t = tanh((double)a.p[f]);
    const double s = sqrt((1.0 - t * t) * (double)a.d_model * 0.5);
    double td = 1.0;
    for (int d = 0; d < a.depth; ++d) {
      pw[d * F + f] = (float)(td * s);
      td *= t;
    }
  }
  __syncthreads();
  for (int c = tid; c < CF; c += TP_FWD_THREADS) w[c] = pw[((c / F) / a.width) * F + c % F];
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * TP_FWD_ROWS;
  const int64_t r1 = r0 + TP_FWD_ROWS < a.rows ? r0 + TP_FWD_ROWS : a.rows;
  for (int64_t r = r0; r < r1; ++r) {
    const float* pr = a.pos + r * C;
    float* orow = a.out + r * CF;
    for (int c = tid; c < CF; c += TP_FWD_THREADS) orow[c] = pr[c / F] * w[c];
  }
}

__global__ __launch_bounds__(1024) void k_tree_pos_bwd_part(const TpArgs a) {
  const int F = a.F, C = a.depth * a.width, CF = C * F;
  const int64_t r0 = (int64_t)blockIdx.x * TP_BWD_ROWS;
  const int64_t r1 = r0 + TP_BWD_ROWS < a.rows ? r0 + TP_BWD_ROWS : a.rows;
  for (int c = threadIdx.x; c < CF; c += blockDim.x) {
    const int j = c / F;
    double acc = 0.0;
    for (int64_t r = r0; r < r1; ++r) acc += (double)a.pos[r * C + j] * (double)a.g[r * CF + c];
    a.ws[(int64_t)blockIdx.x * CF + c] = acc;
  }
}

__global__ __launch_bounds__(256) void k_tree_pos_bwd_fin(const TpArgs a) {
  __shared__ double S[TP_MAX_COLS];
  const int F = a.F, C = a.depth * a.width, CF = C * F;
  for (int c = threadIdx.x; c < CF; c += blockDim.x) {
    double s = 0.0;
    for (int b = 0; b < a.nblk; ++b) s += a.ws[(int64_t)b * CF + c];
    S[c] = s;
  }
  __syncthreads();
  for (int f = threadIdx.x; f < F; f += blockDim.x) {
    const double t = tanh((double)a.p[f]);
    const double c2 = (double)a.d_model * 0.5, one = 1.0 - t * t;
    const double s = sqrt(one * c2), dsdt = -c2 * t / s;
    double acc = 0.0, td = 1.0, tdm1 = 0.0;  // t^d and t^(d-1)
    for (int d = 0; d < a.depth; ++d) {
      double Sd = 0.0;
      for (int x = 0; x < a.width; ++x) Sd += S[(d * a.width + x) * F + f];
      const double dpow = d == 0 ? 0.0 : (double)d * tdm1;  // torch: d/dt pow(t, 0) = 0, d/dt pow(t, 1) = 1
      acc += Sd * (dpow * s + td * dsdt);
      tdm1 = td;
      td *= t;
    }
    a.dp[f] = (float)(acc * one);
  }
}

// ------------------------------------------------------------------------------------
// Laplacian eigenvectors
// ------------------------------------------------------------------------------------
constexpr int LAP_MAX_SWEEPS = 40;
constexpr float LAP_TOL = 1e-6f;
constexpr int LAP_E = 4;                 // column elements per lane of the wave-per-column passes: n <= 256
constexpr int LAP_LDS_LIMIT = 160 * 1024;

struct LapArgs {
  const uint8_t* adj; const int32_t* num_node;
  float* pe; float* eval; int32_t* status; int32_t* sweeps;
  int N, P;
};

inline size_t lap_lds_bytes(int64_t N) {
  return sizeof(float) * (size_t)(N * (N | 1) + 2 * N + LAP_MAX_SWEEPS + 1);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum over the 8 lanes of a group (lanes 8g .. 8g + 7 of a wave) by DPP: quad xor 1, quad xor 2, half-row mirror. Every
// step adds a lane's value to its partner's, so all 8 lanes end with the same bits; no lane outside the group is read.
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float group8_sum(float v) {
  v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  return dpp_add<0x141>(v);  // row_half_mirror
}

// E: column elements per lane of a pair's 8-lane group, 8 E >= N
template <int E>
__global__ __launch_bounds__(1024) void k_lap_pe(const LapArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int N = a.N, LD = N | 1, P = a.P;
  float* M = lds;                 // column-major: element (r, c) at M[c * LD + r]
  float* sig = M + N * LD;        // D^-1/2 while M is built, the column norms afterwards
  int* perm = (int*)(sig + N);    // perm[rank] = column
  int* flags = perm + N;          // flags[s] != 0: sweep s rotated a pair
  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int wave = tid >> 6, lane = tid & 63, nwaves = nthr >> 6;
  const int grp = tid >> 3, gl = tid & 7, ngrp = nthr >> 3;
  int n = a.num_node[b];
  n = n < 0 ? 0 : (n > N ? N : n);
  const uint8_t* A = a.adj + (int64_t)b * N * N;

  for (int i = tid; i <= LAP_MAX_SWEEPS; i += nthr) flags[i] = 0;
  for (int i = tid; i < N; i += nthr) perm[i] = i;  // stays a valid column whatever the norms compare as
  for (int idx = tid; idx < n * n; idx += nthr) {
    const int r = idx / n, c = idx - r * n;
    M[c * LD + r] = A[r * N + c] ? 1.f : 0.f;
  }
  __syncthreads();
  for (int r = tid; r < n; r += nthr) {
    float d = 0.f;
    for (int c = 0; c < n; ++c) d += M[c * LD + r];
    sig[r] = 1.f / sqrtf(fmaxf(d, 1.f));
  }
  __syncthreads();
  for (int idx = tid; idx < n * n; idx += nthr) {
    const int c = idx / n, r = idx - c * n;
    M[c * LD + r] = (r == c ? 2.f : 0.f) - M[c * LD + r] * sig[r] * sig[c];
  }
  __syncthreads();

  // ---- one-sided Jacobi, round-robin ----
  const int m = n + (n & 1), half = m >> 1, rounds = m - 1;
  int sweeps = 0;
  bool conv = n <= 1;
  while (!conv && sweeps < LAP_MAX_SWEEPS) {
    for (int rd = 0; rd < rounds; ++rd) {
      for (int k = grp; k < half; k += ngrp) {  // one pass: the launch has a group per pair
        int i = rd + k, j = rd - k;
        if (k == 0) j = m - 1;
        if (i >= rounds) i -= rounds;
        if (j < 0) j += rounds;
        if (i >= n || j >= n) continue;  // the bye of an odd n (uniform over the group)
        float* ci = M + i * LD;
        float* cj = M + j * LD;
        float x[E], y[E], sa = 0.f, sb = 0.f, sc = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int r = gl + 8 * e;
          x[e] = r < n ? ci[r] : 0.f;
          y[e] = r < n ? cj[r] : 0.f;
          sa = fmaf(x[e], x[e], sa);
          sb = fmaf(y[e], y[e], sb);
          sc = fmaf(x[e], y[e], sc);
        }
        sa = group8_sum(sa); sb = group8_sum(sb); sc = group8_sum(sc);
        if (fabsf(sc) > LAP_TOL * sqrtf(sa * sb)) {  // the same bits in the group's 8 lanes
          const float zeta = (sb - sa) / (2.f * sc);
          const float t = copysignf(1.f, zeta) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
          const float cs = 1.f / sqrtf(1.f + t * t), sn = cs * t;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const int r = gl + 8 * e;
            if (r < n) {
              ci[r] = fmaf(cs, x[e], -sn * y[e]);
              cj[r] = fmaf(sn, x[e], cs * y[e]);
            }
          }
          if (gl == 0) flags[sweeps] = 1;
        }
      }
      __syncthreads();
    }
    conv = flags[sweeps] == 0;  // written before the round's barrier, never written again
    ++sweeps;
  }

  // ---- norms, normalisation, sign ----
  for (int k = wave; k < n; k += nwaves) {
    float* ck = M + k * LD;
    float x[LAP_E], s = 0.f;
#pragma unroll
    for (int e = 0; e < LAP_E; ++e) {
      const int r = lane + 64 * e;
      x[e] = r < n ? ck[r] : 0.f;
      s = fmaf(x[e], x[e], s);
    }
    const float sg = sqrtf(wave_sum(s));
    float bv = 0.f;
    int bi = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < LAP_E; ++e) {
      const int r = lane + 64 * e;
      x[e] = sg > 0.f ? x[e] / sg : 0.f;
      if (r < n && (bi == 0x7fffffff || fabsf(x[e]) > fabsf(bv))) { bv = x[e]; bi = r; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (fabsf(ov) > fabsf(bv) || (fabsf(ov) == fabsf(bv) && oi < bi)) { bv = ov; bi = oi; }
    }
    const float sgn = bv < 0.f ? -1.f : 1.f;
#pragma unroll
    for (int e = 0; e < LAP_E; ++e) {
      const int r = lane + 64 * e;
      if (r < n) ck[r] = sgn * x[e];
    }
    if (lane == 0) sig[k] = sg;
  }
  __syncthreads();

  // ---- order by rank counting, scatter ----
  for (int k = tid; k < n; k += nthr) {
    const float sk = sig[k];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = sig[j];
      rank += (sj < sk || (sj == sk && j < k)) ? 1 : 0;
    }
    perm[rank] = k;
  }
  __syncthreads();
  for (int c = tid; c < N; c += nthr) a.eval[(int64_t)b * N + c] = c < n ? sig[perm[c]] - 1.f : 0.f;
  float* out = a.pe + (int64_t)b * N * P;
  for (int idx = tid; idx < N * P; idx += nthr) {
    const int r = idx / P, c = idx - r * P;
    out[idx] = (r < n && c < n) ? M[perm[c] * LD + r] : 0.f;
  }
  if (tid == 0) {
    a.status[b] = conv ? 0 : 1;
    if (a.sweeps) a.sweeps[b] = sweeps;
  }
}

bool tp_fill(TpArgs& d, const char* what, const float* pos, const float* p, int64_t rows, int64_t depth, int64_t width,
             int64_t n_feat, float d_model, csa_status* st) {
  (void)what;
  *st = CSA_OK;
  if (!pos || !p) *st = fail(CSA_INVALID_ARG, "csa_tree_pos: null pointer (pos, p)");
  else if (rows < 0 || depth < 1 || width < 1 || n_feat < 1) *st = fail(CSA_INVALID_ARG, "csa_tree_pos: rows >= 0 and depth, width, n_feat >= 1");
  else if (!csa_tree_pos_supported(depth, width, n_feat))
    *st = fail(CSA_UNSUPPORTED_SHAPE, "csa_tree_pos: depth <= 64 and depth * width * n_feat <= 1024");
  else if (!(d_model > 0.f)) *st = fail(CSA_INVALID_ARG, "csa_tree_pos: d_model must be positive");
  else if (!aligned(pos, 4) || !aligned(p, 4)) *st = fail(CSA_INVALID_ARG, "csa_tree_pos: misaligned pointer");
  if (*st != CSA_OK) return false;
  d.pos = pos; d.p = p; d.g = nullptr; d.out = nullptr; d.ws = nullptr; d.dp = nullptr;
  d.rows = rows; d.depth = (int)depth; d.width = (int)width; d.F = (int)n_feat; d.nblk = 0; d.d_model = d_model;
  return true;
}

}  // namespace

extern "C" {

int csa_tree_pos_supported(int64_t depth, int64_t width, int64_t n_feat) {
  if (depth < 1 || width < 1 || n_feat < 1 || depth > TP_MAX_DEPTH || width > TP_MAX_COLS || n_feat > TP_MAX_COLS) return 0;
  return depth * width * n_feat <= TP_MAX_COLS ? 1 : 0;
}

size_t csa_tree_pos_bwd_workspace_bytes(int64_t rows, int64_t depth, int64_t width, int64_t n_feat) {
  if (rows <= 0 || !csa_tree_pos_supported(depth, width, n_feat)) return 0;
  const int64_t nblk = (rows + TP_BWD_ROWS - 1) / TP_BWD_ROWS;
  return sizeof(double) * (size_t)(nblk * depth * width * n_feat);
}

csa_status csa_tree_pos_fwd(const float* pos, const float* p, float* out, int64_t rows, int64_t depth, int64_t width,
                            int64_t n_feat, float d_model, void* stream) {
  TpArgs d;
  csa_status s;
  if (!tp_fill(d, "csa_tree_pos_fwd", pos, p, rows, depth, width, n_feat, d_model, &s)) return s;
  if (!out || !aligned(out, 4)) return fail(CSA_INVALID_ARG, "csa_tree_pos_fwd: null or misaligned out");
  if (rows == 0) return CSA_OK;
  const int64_t nblk = (rows + TP_FWD_ROWS - 1) / TP_FWD_ROWS;
  if (nblk > 0x7fffffff) return fail(CSA_UNSUPPORTED_SHAPE, "csa_tree_pos_fwd: too many rows");
  d.out = out;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  hipLaunchKernelGGL(k_tree_pos_fwd, dim3((unsigned)nblk), dim3(TP_FWD_THREADS), 0, st, d);
  return launched("csa_tree_pos_fwd");
}

csa_status csa_tree_pos_bwd(const float* pos, const float* p, const float* dout, float* dp, int64_t rows, int64_t depth,
                            int64_t width, int64_t n_feat, float d_model, void* workspace, void* stream) {
  TpArgs d;
  csa_status s;
  if (!tp_fill(d, "csa_tree_pos_bwd", pos, p, rows, depth, width, n_feat, d_model, &s)) return s;
  if (!dp || !aligned(dp, 4)) return fail(CSA_INVALID_ARG, "csa_tree_pos_bwd: null or misaligned dp");
  if (rows > 0 && (!dout || !aligned(dout, 4) || !workspace || !aligned(workspace, 8)))
    return fail(CSA_INVALID_ARG, "csa_tree_pos_bwd: null or misaligned dout / workspace");
  const int64_t nblk = (rows + TP_BWD_ROWS - 1) / TP_BWD_ROWS;
  if (nblk > 0x7fffffff) return fail(CSA_UNSUPPORTED_SHAPE, "csa_tree_pos_bwd: too many rows");
  d.g = dout; d.dp = dp; d.ws = (double*)workspace; d.nblk = (int)nblk;
  const int CF = d.depth * d.width * d.F;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  if (nblk > 0) {
    const int thr = CF >= 1024 ? 1024 : ((CF + 63) / 64) * 64;
    hipLaunchKernelGGL(k_tree_pos_bwd_part, dim3((unsigned)nblk), dim3(thr), 0, st, d);
    const csa_status e = launched("csa_tree_pos_bwd");
    if (e != CSA_OK) return e;
  }
  hipLaunchKernelGGL(k_tree_pos_bwd_fin, dim3(1), dim3(256), 0, st, d);  // nblk = 0: dp = 0
  return launched("csa_tree_pos_bwd");
}

int csa_lap_pe_supported(int64_t N, int64_t pegen_dim) {
  if (N < 1 || N > 64 * LAP_E || pegen_dim < N || pegen_dim > 0x7fffffff / N) return 0;
  return lap_lds_bytes(N) <= (size_t)LAP_LDS_LIMIT ? 1 : 0;
}

csa_status csa_lap_pe(const csa_lap_pe_args* a, void* stream) {
  if (!a) return fail(CSA_INVALID_ARG, "csa_lap_pe: null args");
  if (a->B < 0 || a->B > 0x7fffffff || a->N < 1 || a->pegen_dim < 1)
    return fail(CSA_INVALID_ARG, "csa_lap_pe: B >= 0 and N, pegen_dim >= 1");
  if (!csa_lap_pe_supported(a->N, a->pegen_dim))
    return fail(CSA_UNSUPPORTED_SHAPE, "csa_lap_pe: needs N <= pegen_dim and an N x N fp32 matrix within the CU's LDS");
  if (a->B == 0) return CSA_OK;
  if (!a->adj || !a->num_node || !a->pe || !a->eigenvalues || !a->status)
    return fail(CSA_INVALID_ARG, "csa_lap_pe: null pointer (adj, num_node, pe, eigenvalues, status)");
  if (!aligned(a->num_node, 4) || !aligned(a->pe, 4) || !aligned(a->eigenvalues, 4) || !aligned(a->status, 4) ||
      !aligned(a->sweeps, 4))
    return fail(CSA_INVALID_ARG, "csa_lap_pe: misaligned pointer");
  LapArgs d;
  d.adj = a->adj; d.num_node = a->num_node; d.pe = a->pe; d.eval = a->eigenvalues; d.status = a->status;
  d.sweeps = a->sweeps; d.N = (int)a->N; d.P = (int)a->pegen_dim;
  const int pairs = (int)((a->N + 1) / 2);  // 8 lanes per pair: N <= 256 fits one pass of 16 waves
  const int waves = (pairs + 7) / 8 > 16 ? 16 : (pairs + 7) / 8;
  const size_t lds = lap_lds_bytes(a->N);
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  const int E = (int)((a->N + 7) / 8);
  void (*kern)(const LapArgs) = E <= 4 ? k_lap_pe<4> : E <= 8 ? k_lap_pe<8> : E <= 16 ? k_lap_pe<16>
                                : E <= 20 ? k_lap_pe<20> : k_lap_pe<32>;
  set_dyn_lds((const void*)kern, (int)lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)a->B), dim3(64 * waves), lds, st, d);
  return launched("csa_lap_pe");
}

}  // extern "C"
