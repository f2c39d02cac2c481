// Batch preparation on the device: every structural field of a batch of ASTs from their parent arrays.
//
// The hot path reads the relation planes L, T, L_mask, T_mask as uint8 (B, N, N) and the use_pegen ablations read
// adj, tree_pos and triplet; all of them are functions of parents (B, N) int32 and num_node (B). The host builds them
// in csa_ast_relations (csa_host.cpp) and the numpy loops of csa_amd/data.py and then copies 90-170 KB per AST to the
// device; here one launch builds them where they are read, from 600 bytes per AST.
//
// One AST per workgroup (S workgroups per AST when its planes are large, each with its own copy of the tables):
//   1. the parent array is range-checked (parent[0] < 0, 0 <= parent[v] < v: any topological numbering, as the host
//      builder accepts) BEFORE any value is used as an index; a malformed tree becomes the empty tree, status = 1;
//   2. per-node tables in LDS, u16 each: parent + 1, depth, child index, Euler-tour interval [tin, tout) of the DFS
//      that visits children in increasing id, and the 16 4-bit child indices of the node's path below depth 16.
//      They come from three O(n) passes by single lanes (depth / child index / path and, on another wave at the same
//      time, subtree sizes; then the interval starts), each a chain of dependent LDS accesses;
//   3. the write pass. a is a proper ancestor of c iff tin[a] < tin[c] < tout[a] (ids need not be pre-order), then
//      rawL = depth[c] - depth[a] in either direction; i, j are siblings iff their parents agree, then
//      rawT = cidx[j] - cidx[i]. Nodes >= n carry tin = 0xffff, tout = 0, parent + 1 = 0, which relates them to
//      nothing, so the element function has no bound checks of its own (adj alone has the n x n block).
//      A plane of one AST is N * N bytes at any byte alignment (N odd, or N = 150 with 150-byte rows): it is written
//      as aligned dwords, one per lane and 256 contiguous bytes per wave instruction, each dword's four elements
//      found from its linear offset; the at most three bytes in front of the first aligned dword and behind the last
//      are single byte stores. Every output byte is written exactly once: no atomics, no read-modify-write, no
//      prefill. tree_pos rows go out as float4 (32 lanes per 512-byte row), triplet as one int64 per lane.
#include "csa_common.hpp"

namespace {

using namespace csa;

constexpr int AB_THREADS = 256;
constexpr int AB_NODE_BYTES = 5 * 2 + 2 + 8;      // par1, depth, cidx, tin, tout | cnt | path
constexpr int AB_LDS_LIMIT = 64 * 1024;           // what a workgroup gets without an opt-in
constexpr int AB_FLAG_BYTES = 16;                 // the malformed-tree flag behind the tables
constexpr int AB_MAX_N = (AB_LDS_LIMIT - AB_FLAG_BYTES) / AB_NODE_BYTES;  // 3276; tin < 0xffff, N * N < 2^24 below it
constexpr int AB_SLICE_BYTES = 8192;              // plane bytes per workgroup before an AST is split
constexpr int AB_MAX_SLICES = 64;
constexpr int REL_OFFSET = 75, REL_MAX = 149;
constexpr unsigned AB_NONE = 0xffffu;

enum { F_L = 0, F_T = 1, F_LM = 2, F_TM = 3, F_ADJ = 4 };

struct AbArgs {
  const int32_t* parents; const int32_t* num_node;
  uint8_t* plane[5];
  float* tree_pos; int64_t* triplet; int32_t* status;
  int64_t plane_sb;  // batch stride of L, T and the masks in bytes
  int N, S;
};

struct AbTables {
  uint16_t* par1;   // parent + 1; 0 for the root and for nodes >= n
  uint16_t* depth;
  uint16_t* cidx;
  uint16_t* tin;    // 0xffff for nodes >= n
  uint16_t* tout;   // subtree sizes until the intervals are closed; 0 for nodes >= n
  uint16_t* cnt;    // children seen so far (pass 1), then the next free interval start (pass 3)
  uint64_t* path;   // nibble d - 1: min(child index, 7) of the ancestor-or-self at depth d <= 16, 0xf when there is none
};

struct AbRow { int tin, tout, depth, par1, cidx; };

__device__ __forceinline__ AbRow ab_row(const AbTables& t, int i) {
  return AbRow{t.tin[i], t.tout[i], t.depth[i], t.par1[i], t.cidx[i]};
}

__device__ __forceinline__ int rel_idx(int raw) {
  const int v = raw + REL_OFFSET;
  return v < 0 ? 0 : v > REL_MAX ? REL_MAX : v;
}

// element (i, j) of one plane; r holds row i's table entries
template <int F>
__device__ __forceinline__ unsigned ab_elem(const AbTables& t, const AbRow& r, int i, int j, int n) {
  if (F == F_T || F == F_TM) {
    const int pj = t.par1[j];
    const int raw = (pj == r.par1 && pj != 0) ? (int)t.cidx[j] - r.cidx : 0;  // i == j: 0 as well
    return F == F_T ? (unsigned)rel_idx(raw) : (unsigned)(raw == 0);
  }
  const int tj = t.tin[j], oj = t.tout[j];
  const bool related = (r.tin < tj && tj < r.tout) || (tj < r.tin && r.tin < oj);
  const int raw = related ? (int)t.depth[j] - r.depth : 0;
  if (F == F_L) return (unsigned)rel_idx(raw);
  if (F == F_LM) return (unsigned)(raw == 0);
  return (unsigned)(i < n && j < n && raw >= -1 && raw <= 1);
}

// One AST's plane, N * N bytes from `out` (any alignment): this workgroup's share of the aligned dwords, and for
// slice 0 the bytes outside them.
template <int F>
__device__ void ab_write_plane(uint8_t* __restrict__ out, const AbTables& t, int N, int n, int slice, int S) {
  const int NN = N * N;
  int e0 = (int)((4u - (unsigned)((uintptr_t)out & 3u)) & 3u);  // bytes in front of the first aligned dword
  if (e0 > NN) e0 = NN;
  const int K = (NN - e0) >> 2;
  const int k_lo = (int)((int64_t)K * slice / S), k_hi = (int)((int64_t)K * (slice + 1) / S);
  for (int k = k_lo + (int)threadIdx.x; k < k_hi; k += AB_THREADS) {
    const int e = e0 + 4 * k;
    int i = e / N, j = e - i * N;
    AbRow r = ab_row(t, i);
    unsigned w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      w |= ab_elem<F>(t, r, i, j, n) << (8 * b);
      if (++j == N && b < 3) {  // the dword runs into the next row (e + 3 < N * N, so there is one)
        j = 0;
        ++i;
        r = ab_row(t, i);
      }
    }
    *reinterpret_cast<uint32_t*>(out + e) = w;
  }
  if (slice == 0 && threadIdx.x < 6) {
    const int q = (int)threadIdx.x;
    const int e = q < 3 ? q : e0 + 4 * K + (q - 3);
    if (q < 3 ? e < e0 : e < NN) {
      const int i = e / N, j = e - i * N;
      out[e] = (uint8_t)ab_elem<F>(t, ab_row(t, i), i, j, n);
    }
  }
}

__global__ __launch_bounds__(AB_THREADS) void k_ast_batch(const AbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ab_lds[];
  const int N = a.N, S = a.S;
  const int b = (int)(blockIdx.x / (unsigned)S), slice = (int)(blockIdx.x % (unsigned)S);
  const int tid = (int)threadIdx.x;
  const int NP = (N + 3) & ~3;  // keeps every table 8-byte aligned
  AbTables t;
  t.path = reinterpret_cast<uint64_t*>(ab_lds);
  t.par1 = reinterpret_cast<uint16_t*>(ab_lds + 8 * (size_t)NP);
  t.depth = t.par1 + NP;
  t.cidx = t.depth + NP;
  t.tin = t.cidx + NP;
  t.tout = t.tin + NP;
  t.cnt = t.tout + NP;
  int* flag = reinterpret_cast<int*>(ab_lds + (size_t)AB_NODE_BYTES * NP);

  const int32_t* __restrict__ par = a.parents + (int64_t)b * N;
  int n = a.num_node[b];
  n = n < 0 ? 0 : n > N ? N : n;

  // 1. range check, before anything is used as an index
  int bad = 0;
  for (int v = tid; v < n; v += AB_THREADS) {
    const int p = par[v];
    bad |= v == 0 ? p >= 0 : (p < 0 || p >= v);
  }
  if (tid == 0) *flag = 0;
  __syncthreads();
  if (bad) *flag = 1;  // plain stores of one value: no atomic
  __syncthreads();
  bad = *flag;
  if (bad) n = 0;
  if (tid == 0 && slice == 0) a.status[b] = bad ? 1 : 0;

  // 2. tables
  for (int v = tid; v < N; v += AB_THREADS) {
    t.par1[v] = (uint16_t)((v > 0 && v < n) ? par[v] + 1 : 0);
    t.depth[v] = 0;
    t.cidx[v] = 0;
    t.cnt[v] = 0;
    t.tin[v] = (uint16_t)(v == 0 && n > 0 ? 0 : AB_NONE);
    t.tout[v] = (uint16_t)(v < n ? 1 : 0);
    t.path[v] = ~0ull;
  }
  __syncthreads();
  if (tid == 0) {  // depth, child index and path, top down
    int pn = n > 1 ? t.par1[1] : 0;  // the next parent is read a step ahead: one LDS round trip per node, not two
    for (int v = 1; v < n; ++v) {
      const int p = pn - 1;
      pn = t.par1[v + 1 < n ? v + 1 : v];
      const int d = t.depth[p] + 1, c = t.cnt[p];
      uint64_t ph = t.path[p];
      t.cnt[p] = (uint16_t)(c + 1);
      t.depth[v] = (uint16_t)d;
      t.cidx[v] = (uint16_t)c;
      if (d <= 16) ph = (ph & ~(0xfull << (4 * (d - 1)))) | ((uint64_t)(c < 7 ? c : 7) << (4 * (d - 1)));
      t.path[v] = ph;
    }
  } else if (tid == 64) {  // subtree sizes, bottom up (children have larger ids), on another wave
    int pn = n > 1 ? t.par1[n - 1] : 0;
    for (int v = n - 1; v >= 1; --v) {
      const int p = pn - 1;
      pn = t.par1[v > 1 ? v - 1 : v];
      t.tout[p] = (uint16_t)(t.tout[p] + t.tout[v]);
    }
  }
  __syncthreads();
  if (tid == 0 && n > 0) {  // interval starts: a node's children follow it in increasing id
    t.cnt[0] = 1;
    int pn = n > 1 ? t.par1[1] : 0;
    for (int v = 1; v < n; ++v) {
      const int p = pn - 1;
      pn = t.par1[v + 1 < n ? v + 1 : v];
      const int s = t.cnt[p];
      t.tin[v] = (uint16_t)s;
      t.cnt[p] = (uint16_t)(s + t.tout[v]);
      t.cnt[v] = (uint16_t)(s + 1);
    }
  }
  __syncthreads();
  for (int v = tid; v < n; v += AB_THREADS) t.tout[v] = (uint16_t)(t.tin[v] + t.tout[v]);
  __syncthreads();

  // 3. outputs
  const int64_t sb = a.plane_sb;
  if (a.plane[F_L]) ab_write_plane<F_L>(a.plane[F_L] + b * sb, t, N, n, slice, S);
  if (a.plane[F_T]) ab_write_plane<F_T>(a.plane[F_T] + b * sb, t, N, n, slice, S);
  if (a.plane[F_LM]) ab_write_plane<F_LM>(a.plane[F_LM] + b * sb, t, N, n, slice, S);
  if (a.plane[F_TM]) ab_write_plane<F_TM>(a.plane[F_TM] + b * sb, t, N, n, slice, S);
  if (a.plane[F_ADJ]) ab_write_plane<F_ADJ>(a.plane[F_ADJ] + b * ((int64_t)N * N), t, N, n, slice, S);

  const int v_lo = (int)((int64_t)N * slice / S), v_hi = (int)((int64_t)N * (slice + 1) / S);
  if (a.tree_pos) {  // lane q of a row's 32 writes floats 4 q .. 4 q + 3: the depth-(16 - q / 2) step, half q & 1
    f32x4* __restrict__ tp = reinterpret_cast<f32x4*>(a.tree_pos + ((int64_t)b * N + v_lo) * 128);
    const int items = (v_hi - v_lo) * 32;
    for (int w = tid; w < items; w += AB_THREADS) {
      const int v = v_lo + (w >> 5), q = w & 31;
      const unsigned nib = (unsigned)(t.path[v] >> (4 * (15 - (q >> 1)))) & 0xfu;
      f32x4 z = {0.f, 0.f, 0.f, 0.f};
      if (nib != 0xfu && (int)(nib >> 2) == (q & 1)) {
        const unsigned c = nib & 3u;
        z[0] = c == 0 ? 1.f : 0.f; z[1] = c == 1 ? 1.f : 0.f; z[2] = c == 2 ? 1.f : 0.f; z[3] = c == 3 ? 1.f : 0.f;
      }
      tp[w] = z;
    }
  }
  if (a.triplet) {
    int64_t* __restrict__ tr = a.triplet + (int64_t)b * N;
    for (int v = v_lo + tid; v < v_hi; v += AB_THREADS) {
      int64_t id = 0;  // PAD
      if (v < n) {
        const int d = t.depth[v], c = t.cidx[v];
        const int pc = v > 0 ? (int)t.cidx[t.par1[v] - 1] : 0;
        id = 2 + (d < 15 ? d : 15) * 64 + (pc < 7 ? pc : 7) * 8 + (c < 7 ? c : 7);
      }
      tr[v] = id;
    }
  }
}

size_t ab_lds_bytes(int64_t N) { return (size_t)AB_NODE_BYTES * (size_t)((N + 3) & ~(int64_t)3) + AB_FLAG_BYTES; }

}  // namespace

extern "C" {

int csa_ast_batch_supported(int64_t N) {
  return N >= 1 && N <= AB_MAX_N && ab_lds_bytes(N) <= (size_t)AB_LDS_LIMIT ? 1 : 0;
}

csa_status csa_ast_batch(const csa_ast_batch_args* a, void* stream) {
  if (!a) return fail(CSA_INVALID_ARG, "csa_ast_batch: null args");
  if (a->B < 0 || a->N < 1) return fail(CSA_INVALID_ARG, "csa_ast_batch: B >= 0 and N >= 1");
  if (!csa_ast_batch_supported(a->N))
    return fail(CSA_UNSUPPORTED_SHAPE, "csa_ast_batch: the per-node tables (20 bytes a node) must fit 64 KiB of LDS: N <= 3276");
  if (a->B == 0) return CSA_OK;
  if (!a->parents || !a->num_node || !a->status)
    return fail(CSA_INVALID_ARG, "csa_ast_batch: null pointer (parents, num_node, status)");
  if (!aligned(a->parents, 4) || !aligned(a->num_node, 4) || !aligned(a->status, 4) || !aligned(a->tree_pos, 16) ||
      !aligned(a->triplet, 8))
    return fail(CSA_INVALID_ARG, "csa_ast_batch: misaligned pointer (int32 inputs 4, tree_pos 16, triplet 8 bytes)");
  if (a->plane_sb != 0 && a->plane_sb < a->N * a->N)
    return fail(CSA_INVALID_ARG, "csa_ast_batch: plane_sb is 0 or at least N * N");
  int64_t S = a->N * a->N / AB_SLICE_BYTES;
  S = S < 1 ? 1 : S > AB_MAX_SLICES ? AB_MAX_SLICES : S;
  if (a->B > 0x7fffffff / S) return fail(CSA_UNSUPPORTED_SHAPE, "csa_ast_batch: too many ASTs");
  AbArgs d;
  d.parents = a->parents; d.num_node = a->num_node;
  d.plane[F_L] = a->L; d.plane[F_T] = a->T; d.plane[F_LM] = a->L_mask; d.plane[F_TM] = a->T_mask; d.plane[F_ADJ] = a->adj;
  d.tree_pos = a->tree_pos; d.triplet = a->triplet; d.status = a->status;
  d.plane_sb = a->plane_sb ? a->plane_sb : a->N * a->N;
  d.N = (int)a->N; d.S = (int)S;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  hipLaunchKernelGGL(k_ast_batch, dim3((unsigned)(a->B * S)), dim3(AB_THREADS), ab_lds_bytes(a->N), st, d);
  return launched("csa_ast_batch");
}

}  // extern "C"
