// Validation metrics of decoded ids on the device: smoothed sentence BLEU-4 (valid_metrices/google_bleu.py
// compute_bleu(smooth=True) behind bleu_output_transform) and ROUGE-L (valid_metrices/rouge/rouge.py calc_score), restated
// on token ids, so that a validation pass scores what the generators leave on the device without a copy to the host.
//
//   k_seq_metrics<NW>  one launch scores R = B * G hypothesis rows against B reference rows; hypothesis row r belongs to
//                      reference r / G. A row's length is the index of its first eos_id (none: the full width); every
//                      other id is an ordinary token. An empty hypothesis is the reference's one-token placeholder that
//                      matches nothing (length 1, possible counts 1,0,0,0, no match, LCS 0); a row whose reference is
//                      empty is invalid (valid = 0 and every other output 0).
//
// One wave64 per hypothesis row, one wave per workgroup, NW = ceil(max(Th, Tr) / 64) in {1, 2, 4} words of 64 positions
// (the launch classes). Both rows are staged once into LDS as the int64 they are (ids above 2^31 compare as any other).
//   clipped matches  lane l of word w owns hypothesis position i = 64 w + l and holds its four tokens h[i .. i + 3]. One
//                    pass over the hypothesis positions j < i and one over the reference positions k, every lane reading
//                    the same four LDS words (a broadcast), count for n = 1..4 at once the earlier hypothesis positions
//                    and the reference positions that carry position i's n-gram; i is a clipped match exactly when fewer
//                    earlier positions carry it than the reference has, and m_n is the popcount of that ballot: this is
//                    sum_g min(count_hyp(g), count_ref(g)) with no hashing and no sorting.
//                    sum_w min(len_h, 64 (w + 1)) + NW len_r vector steps per row for the four orders together.
//   LCS              the bit-parallel recurrence over the reference tokens on ballot masks, wave-uniform: M = ballot(h ==
//                    r[k]), U = V & M, V = (V + U) | (V & ~M) with the carry run across the NW words; the LCS is the count
//                    of zero bits of V below len_h. len_r NW steps per row.
// The scores are fp64 in the reference's order of operations, written by lane 0 with the int32 record. A row's result
// depends on that row and its reference alone: no atomics, no cross-row state, no allocation, no sync; deterministic.
#include "csa_common.hpp"
#include "../../include/csa_hip.h"

#include <math.h>

using namespace csa;

namespace {

constexpr int MET_MAX_T = 256;
constexpr int MET_FIELDS = 12;  // m1..m4, poss1..poss4, len_h, len_r, lcs, valid

struct MetArgs {
  const int64_t* hyp; int64_t hyp_s; int Th;
  const int64_t* ref; int64_t ref_s; int Tr;
  int64_t G, eos;
  int32_t* stats; double* bleu; double* rouge;
};

template <int NW>
__global__ __launch_bounds__(64) void k_seq_metrics(const MetArgs a) {
  constexpr int CAP = NW * 64;
  __shared__ int64_t hs[CAP + 4], rs[CAP + 4];  // 3 words of slack: position i reads i .. i + 3
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t* hp = a.hyp + row * a.hyp_s;
  const int64_t* rp = a.ref + (row / a.G) * a.ref_s;

  // ---- stage both rows, find the first EOS of each (words in descending order: the lowest one wins) ----
  int lh = a.Th, lr = a.Tr;
  int64_t hreg[NW];
#pragma unroll
  for (int w = NW - 1; w >= 0; --w) {
    const int p = w * 64 + lane;
    const int64_t hv = p < a.Th ? hp[p] : 0;
    const int64_t rv = p < a.Tr ? rp[p] : 0;
    hreg[w] = hv;
    hs[p] = hv;
    rs[p] = rv;
    const unsigned long long eh = __ballot(p < a.Th && hv == a.eos);
    const unsigned long long er = __ballot(p < a.Tr && rv == a.eos);
    if (eh) lh = w * 64 + __builtin_ctzll(eh);
    if (er) lr = w * 64 + __builtin_ctzll(er);
  }
  if (lane < 4) {
    hs[CAP + lane] = 0;
    rs[CAP + lane] = 0;
  }
  __syncthreads();

  int m[4] = {0, 0, 0, 0};
  int lcs = 0;
  const bool valid = lr > 0;        // wave-uniform, as is everything derived from lh and lr
  if (valid && lh > 0) {
    // ---- clipped n-gram matches, n = 1..4 in one pass ----
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      if (w * 64 < lh) {
        const int i = w * 64 + lane;
        const int64_t a0 = hs[i], a1 = hs[i + 1], a2 = hs[i + 2], a3 = hs[i + 3];
        int cb[4] = {0, 0, 0, 0}, cr[4] = {0, 0, 0, 0};
        const int jend = lh < w * 64 + 64 ? lh : w * 64 + 64;
        // an n-gram that starts before a valid start i ends before i's does, so it lies inside the hypothesis
        for (int j = 0; j < jend; ++j) {
          const bool e1 = j < i && hs[j] == a0;
          const bool e2 = e1 && hs[j + 1] == a1;
          const bool e3 = e2 && hs[j + 2] == a2;
          const bool e4 = e3 && hs[j + 3] == a3;
          cb[0] += e1; cb[1] += e2; cb[2] += e3; cb[3] += e4;
        }
        for (int k = 0; k < lr; ++k) {
          const bool e1 = rs[k] == a0;
          const bool e2 = e1 && k + 2 <= lr && rs[k + 1] == a1;
          const bool e3 = e2 && k + 3 <= lr && rs[k + 2] == a2;
          const bool e4 = e3 && k + 4 <= lr && rs[k + 3] == a3;
          cr[0] += e1; cr[1] += e2; cr[2] += e3; cr[3] += e4;
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) m[n] += __popcll(__ballot(i + n + 1 <= lh && cb[n] < cr[n]));
      }
    }
    // ---- LCS: V = (V + (V & M)) | (V & ~M) per reference token, carry across the words ----
    unsigned long long V[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) V[w] = ~0ull;
    for (int k = 0; k < lr; ++k) {
      const int64_t t = rs[k];
      unsigned long long carry = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const unsigned long long M = __ballot(w * 64 + lane < lh && hreg[w] == t);
        const unsigned long long v = V[w], s = v + (v & M), s2 = s + carry;
        carry = (unsigned long long)(s < v) | (unsigned long long)(s2 < s);
        V[w] = s2 | (v & ~M);
      }
    }
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int nb = lh - w * 64;
      const unsigned long long low = nb <= 0 ? 0ull : nb >= 64 ? ~0ull : ((1ull << nb) - 1ull);
      lcs += __popcll(~V[w] & low);
    }
  }

  if (lane != 0) return;
  int32_t* st = a.stats + row * MET_FIELDS;
  if (!valid) {
#pragma unroll
    for (int f = 0; f < MET_FIELDS; ++f) st[f] = 0;
    a.bleu[row] = 0.0;
    a.rouge[row] = 0.0;
    return;
  }
  const int len_h = lh > 0 ? lh : 1;  // the placeholder token of an empty hypothesis
  double log_sum = 0.0;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int poss = len_h - n > 0 ? len_h - n : 0;
    st[n] = m[n];
    st[4 + n] = poss;
    log_sum += 0.25 * log(((double)m[n] + 1.0) / ((double)poss + 1.0));
  }
  st[8] = len_h; st[9] = lr; st[10] = lcs; st[11] = 1;
  const double ratio = (double)len_h / (double)lr;
  const double bp = ratio > 1.0 ? 1.0 : exp(1.0 - 1.0 / ratio);
  a.bleu[row] = exp(log_sum) * bp;
  double rouge = 0.0;
  if (lcs > 0) {
    const double beta2 = 1.2 * 1.2;
    const double prec = (double)lcs / (double)len_h, rec = (double)lcs / (double)lr;
    rouge = ((1.0 + beta2) * prec * rec) / (rec + beta2 * prec);
  }
  a.rouge[row] = rouge;
}

}  // namespace

extern "C" {

int csa_seq_metrics_supported(int64_t Th, int64_t Tr) {
  return (Th >= 1 && Th <= MET_MAX_T && Tr >= 1 && Tr <= MET_MAX_T) ? 1 : 0;
}

csa_status csa_seq_metrics(const csa_seq_metrics_args* a, void* stream) {
  if (!a) return fail(CSA_INVALID_ARG, "csa_seq_metrics: null args");
  if (!a->hyp || !a->ref || !a->stats || !a->bleu || !a->rouge)
    return fail(CSA_INVALID_ARG, "csa_seq_metrics: null pointer (hyp, ref, stats, bleu, rouge)");
  if (a->rows < 0 || a->rows > 0x7fffffff || a->Th < 0 || a->Tr < 0)
    return fail(CSA_INVALID_ARG, "csa_seq_metrics: negative size (rows, Th, Tr) or more than 2^31 - 1 rows");
  if (a->group < 1 || a->rows % a->group != 0)
    return fail(CSA_INVALID_ARG, "csa_seq_metrics: group must be at least 1 and divide rows");
  if (a->hyp_stride < a->Th || a->ref_stride < a->Tr)
    return fail(CSA_INVALID_ARG, "csa_seq_metrics: a row stride below Th (hyp) or Tr (ref)");
  if (!csa_seq_metrics_supported(a->Th, a->Tr))
    return fail(CSA_UNSUPPORTED_SHAPE, "csa_seq_metrics: Th and Tr must be in [1, 256]");
  if (!aligned(a->hyp, 8) || !aligned(a->ref, 8) || !aligned(a->stats, 4) || !aligned(a->bleu, 8) || !aligned(a->rouge, 8))
    return fail(CSA_INVALID_ARG, "csa_seq_metrics: misaligned pointer (ids and scores 8, the int32 record 4 bytes)");
  if (a->rows == 0) return CSA_OK;
  MetArgs d;
  d.hyp = a->hyp; d.hyp_s = a->hyp_stride; d.Th = (int)a->Th;
  d.ref = a->ref; d.ref_s = a->ref_stride; d.Tr = (int)a->Tr;
  d.G = a->group; d.eos = a->eos_id;
  d.stats = a->stats; d.bleu = a->bleu; d.rouge = a->rouge;
  const hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(st);
  const int64_t T = a->Th > a->Tr ? a->Th : a->Tr;
  const dim3 grid((unsigned)a->rows), block(64);
  if (T <= 64) hipLaunchKernelGGL(k_seq_metrics<1>, grid, block, 0, st, d);
  else if (T <= 128) hipLaunchKernelGGL(k_seq_metrics<2>, grid, block, 0, st, d);
  else hipLaunchKernelGGL(k_seq_metrics<4>, grid, block, 0, st, d);
  return launched("csa_seq_metrics");
}

}  // extern "C"
