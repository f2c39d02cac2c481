"""Loop oracle of the validation metrics on id lists, and the cases the CPU and GPU tests share.

The oracle restates three reference functions on ids, in plain Python with Counter and the DP LCS:
bleu_output_transform (valid_metrices/bleu_metrice.py: cut at the first EOS, the "<???>" placeholder for an empty
hypothesis, rows with an empty reference dropped), google_bleu.compute_bleu(smooth=True) for one reference, and
rouge.Rouge.calc_score (beta = 1.2). tools/gen_metric_golden.py pins it to the reference's own code run on words
(tests/golden/seq_metrics_*.npz).

Cases are built with numpy's legacy RandomState, whose streams are frozen, so the golden files hold results only."""
import functools
import math
from collections import Counter

import numpy as np

EOS_ID = 3
FIELDS = ("m1", "m2", "m3", "m4", "poss1", "poss2", "poss3", "poss4", "len_h", "len_r", "lcs", "valid")
PLACEHOLDER = ("<???>",)  # equal to no id
BETA = 1.2
LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256)
BIG = 1 << 40  # ids above 2^31


def trim(ids, eos):
    ids = [int(v) for v in ids]
    return ids[:ids.index(eos)] if eos in ids else ids


def ngram_counts(tokens, n):
    """How often each run of n consecutive tokens occurs."""
    return Counter(zip(*(tokens[k:] for k in range(n))))


def lcs_len(a, b):
    """Length of the longest common subsequence of two lists: the textbook DP, one rolling row."""
    row = [0] * (len(b) + 1)
    for x in a:
        nxt = [0]
        for j, y in enumerate(b):
            nxt.append(row[j] + 1 if x == y else max(row[j + 1], nxt[j]))
        row = nxt
    return row[-1]


def bleu_from_counts(m, poss, len_h, len_r):
    """Smoothed BLEU-4 from the four match counts, the four possible counts and the two lengths, in the fp64 operation
    order of the reference's compute_bleu(smooth=True): a quarter of each log added in turn from 0, one exp, then the
    brevity penalty exp(1 - 1 / (len_h / len_r)) unless the hypothesis is the longer."""
    log_sum = 0.0
    for hit, total in zip(m, poss):
        log_sum += 0.25 * math.log((hit + 1.0) / (total + 1.0))
    length_ratio = len_h / len_r
    brevity = 1.0 if length_ratio > 1.0 else math.exp(1.0 - 1.0 / length_ratio)
    return math.exp(log_sum) * brevity


def rouge_from_lcs(lcs, len_h, len_r):
    """ROUGE-L F-measure with beta = 1.2 from the LCS length, in the reference's operation order; 0 without an LCS."""
    if lcs == 0:
        return 0.0
    b2 = BETA ** 2
    p, r = lcs / len_h, lcs / len_r
    return (1 + b2) * p * r / (r + b2 * p)


def score_row(hyp_ids, ref_ids, eos=EOS_ID):
    """-> (the 12 integer fields, bleu, rouge) of one hypothesis row against its reference row."""
    hyp, ref = trim(hyp_ids, eos), trim(ref_ids, eos)
    if not ref:  # an invalid row
        return [0] * 12, 0.0, 0.0
    if not hyp:
        hyp = [PLACEHOLDER]
    m = [sum((ngram_counts(hyp, n) & ngram_counts(ref, n)).values()) for n in range(1, 5)]  # clipped at the reference's
    poss = [max(len(hyp) - n + 1, 0) for n in range(1, 5)]
    lcs = lcs_len(ref, hyp)
    fields = m + poss + [len(hyp), len(ref), lcs, 1]
    return fields, bleu_from_counts(m, poss, len(hyp), len(ref)), rouge_from_lcs(lcs, len(hyp), len(ref))


def score(hyp, ref, eos=EOS_ID, group=1):
    """hyp (R, Th), ref (R / group, Tr) id arrays -> stats (R, 12) int32, bleu (R,) and rouge (R,) float64."""
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    R = hyp.shape[0]
    assert R == ref.shape[0] * group
    stats = np.zeros((R, 12), np.int32)
    bleu, rouge = np.zeros(R), np.zeros(R)
    for r in range(R):
        stats[r], bleu[r], rouge[r] = score_row(hyp[r], ref[r // group], eos)
    return stats, bleu, rouge


def aggregate(stats, bleu, rouge):
    """What SummaryMetrics.compute returns, from per-row results: BLEU4's mean over valid rows, compute_bleu over the
    summed counts (the first value of google_bleu.corpus_bleu), the mean ROUGE-L and the number of valid rows."""
    stats = np.asarray(stats, np.int64)
    ok = stats[:, 11] == 1
    n = int(ok.sum())
    s = stats[ok].sum(0)
    return {"bleu": float(np.sum(bleu[ok])) / n, "rouge_l": float(np.sum(rouge[ok])) / n, "n": n,
            "corpus_bleu": bleu_from_counts([int(v) for v in s[0:4]], [int(v) for v in s[4:8]], int(s[8]), int(s[9]))}


# ---- cases ----

def _row(rng, length, width, vocab, eos=EOS_ID):
    """`length` tokens from `vocab` (never eos), then eos and a tail of anything (more eos included) up to `width`;
    length == width: no eos at all."""
    row = rng.choice(vocab, size=width).astype(np.int64)
    if length < width:
        row[length] = eos
        tail = width - length - 1
        if tail:
            row[length + 1:] = rng.choice(list(vocab) + [eos], size=tail)
    return row


VOCABS = ((5, 6, 7), tuple(range(4, 16)), tuple(range(4, 1000)), (5, 6, BIG + 5, BIG + 6, -9))


@functools.lru_cache(maxsize=None)
def length_case(width):
    """Every (hypothesis length, reference length) pair of LENGTHS that fits `width`, one row each (group 1); the
    length `width` itself is a row without EOS. Vocabularies rotate between 3 tokens (heavy repetition), 12, ~1000 and
    one with ids above 2^31 and a negative id; every third hypothesis is its reference with a few edits, so that long
    n-grams match."""
    rng = np.random.RandomState(1000 + width)
    lens = [n for n in LENGTHS if n <= width]
    hyp, ref = [], []
    for q, (lh, lr) in enumerate((a, b) for a in lens for b in lens):
        vocab = VOCABS[q % len(VOCABS)]
        r = _row(rng, lr, width, vocab)
        h = _row(rng, lh, width, vocab)
        if q % 3 == 0 and min(lh, lr) > 0:
            n = min(lh, lr)
            h[:n] = r[:n]
            for _ in range(1 + n // 16):
                h[rng.randint(n)] = vocab[rng.randint(len(vocab))]
        hyp.append(h)
        ref.append(r)
    return np.stack(hyp), np.stack(ref)


SPECIAL_TH, SPECIAL_TR = 9, 7
SPECIAL_NAMES = ("clip_aaaa_vs_aa", "identical", "disjoint", "hyp_eos_at_0", "empty_reference", "both_empty", "no_eos",
                 "above_2_31", "above_2_31_low_words_equal", "pad_and_unk_are_tokens", "shorter_than_order", "second_eos_ignored")


@functools.lru_cache(maxsize=None)
def special_case():
    """Hand-written rows (group 1), widths 9 and 7, named by SPECIAL_NAMES."""
    E = EOS_ID

    def h(*v):
        return list(v) + [E] * (SPECIAL_TH - len(v))

    def r(*v):
        return list(v) + [E] * (SPECIAL_TR - len(v))

    rows = [
        (h(5, 5, 5, 5), r(5, 5)),
        (h(5, 6, 7, 8, 9, 10), r(5, 6, 7, 8, 9, 10)),
        (h(5, 6, 7, 8, 9), r(10, 11, 12, 13, 14)),
        (h(), r(5, 6, 7)),
        (h(5, 6, 7), r()),
        (h(), r()),
        ([5, 6, 7, 5, 6, 7, 5, 6, 7], [5, 6, 7, 5, 6, 8, 9]),
        (h(BIG + 1, BIG + 2, 7, BIG + 1), r(BIG + 1, BIG + 2, 7)),
        (h((1 << 32) + 5, 5, (2 << 32) + 5), r(5, 5, 5)),
        (h(0, 0, 1, 1, 0), r(0, 1, 1, 0)),
        (h(5, 6), r(5, 6, 7, 8)),
        ([5, 6, E, 7, 8, E, 5, 6, 7], [5, 6, 7, 8, E, 5, E]),
    ]
    assert len(rows) == len(SPECIAL_NAMES)
    return np.array([a for a, _ in rows], np.int64), np.array([b for _, b in rows], np.int64)


GROUP_B, GROUP_TH, GROUP_TR = 257, 12, 11
ROW_COUNTS = (1, 63, 64, 65, 257)
GROUPS = (1, 3, 4)


@functools.lru_cache(maxsize=None)
def group_case(group):
    """257 references and 257 * group hypotheses of widths 12 and 11 over a 5-token vocabulary, lengths uniform in
    [0, width]. A row's result depends on that row and its reference alone, so the first B * group rows are the case of
    B references."""
    rng = np.random.RandomState(2000 + group)
    vocab = (5, 6, 7, 8, 9)
    ref = np.stack([_row(rng, rng.randint(GROUP_TR + 1), GROUP_TR, vocab) for _ in range(GROUP_B)])
    hyp = np.stack([_row(rng, rng.randint(GROUP_TH + 1), GROUP_TH, vocab) for _ in range(GROUP_B * group)])
    return hyp, ref


WIDE_TH, WIDE_TR = 257, 300


@functools.lru_cache(maxsize=None)
def wide_case():
    """Rows wider than the device limit (group 2): they take the host fallback."""
    rng = np.random.RandomState(3000)
    vocab = VOCABS[1]
    ref = np.stack([_row(rng, n, WIDE_TR, vocab) for n in (300, 257, 64, 0)])
    hyp = np.stack([_row(rng, n, WIDE_TH, vocab) for n in (257, 256, 200, 0, 65, 1, 5, 257)])
    hyp[0, :257] = ref[0, :257]
    return hyp, ref


# name -> (builder, group); the golden files cover exactly these
CASES = {
    "special": (special_case, 1),
    "len64": (functools.partial(length_case, 64), 1),
    "len128": (functools.partial(length_case, 128), 1),
    "len256": (functools.partial(length_case, 256), 1),
    "group3": (lambda: tuple(a[:65 * g] for a, g in zip(group_case(3), (3, 1))), 3),
    "wide": (wide_case, 2),
}


@functools.lru_cache(maxsize=None)
def oracle(name):
    """-> (stats, bleu, rouge) of a case of CASES, computed once."""
    build, group = CASES[name]
    hyp, ref = build()
    return score(hyp, ref, EOS_ID, group)


@functools.lru_cache(maxsize=None)
def group_oracle(group):
    hyp, ref = group_case(group)
    return score(hyp, ref, EOS_ID, group)
