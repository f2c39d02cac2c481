"""Generate tests/golden/seq_metrics_*.npz by running the REFERENCE's own metric code on words (where a checkout of the
reference is at hand only; the fixtures travel, the reference does not).

usage: PYTHONDONTWRITEBYTECODE=1 python tools/gen_metric_golden.py --reference <checkout of the reference>

valid_metrices/google_bleu.py and valid_metrices/rouge/rouge.py are loaded BY FILE PATH and run as they are. The package's
bleu_metrice.py cannot be imported (it needs ignite, and valid_metrices/__init__ pulls in the METEOR jar wrapper), so
two small pieces of it are RESTATED here, not run: bleu_output_transform (ids -> words, cut at the first EOS word, the
"<???>" placeholder for an empty hypothesis, rows with an empty reference dropped) and BLEU4's averaging (sum of the
sentence scores / their number). Ids become words through a synthetic injective i2w (id -> "w<id>", the EOS id ->
"<eos>"); no word contains whitespace and none is "<???>".

Per case of tests/metric_ref.py CASES and per row the file holds the reference's sentence BLEU, ROUGE-L, smoothed
precisions, lengths and my_lcs value, the match counts read back from the precisions, and a valid flag; and the
aggregates over the valid rows: BLEU4's mean, corpus_bleu's corpus and average values, Rouge.compute_score's mean.
Results only: the ids are rebuilt by metric_ref's builders (a crc of them is stored to catch a drift)."""
import argparse
import importlib.util
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metric_ref  # noqa: E402

EOS_WORD = "<eos>"


def load(path, name):
    s = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(s)
    s.loader.exec_module(m)
    return m


def i2w(i):
    return EOS_WORD if i == metric_ref.EOS_ID else f"w{i}"


def output_transform(hyp_row, ref_row):
    """The rule of bleu_output_transform for one row, written from its description: both id rows are cut in front of
    their first EOS and become words; a pair with no reference words is dropped (None); no hypothesis words become the
    single word "<???>". -> (hypothesis words, reference words) or None."""
    ref_words = [i2w(i) for i in metric_ref.trim(ref_row, metric_ref.EOS_ID)]
    if not ref_words:
        return None
    hyp_words = [i2w(i) for i in metric_ref.trim(hyp_row, metric_ref.EOS_ID)]
    return hyp_words or ["<???>"], ref_words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    gb = load(os.path.join(a.reference, "valid_metrices", "google_bleu.py"), "ref_google_bleu")
    rg = load(os.path.join(a.reference, "valid_metrices", "rouge", "rouge.py"), "ref_rouge")
    rouge = rg.Rouge()
    out_dir = os.path.join(ROOT, "tests", "golden")
    for name, (build, group) in metric_ref.CASES.items():
        hyp, ref = build()
        R = hyp.shape[0]
        bleu, rl = np.zeros(R), np.zeros(R)
        prec = np.zeros((R, 4))
        m = np.zeros((R, 4), np.int32)
        len_h, len_r, lcs, valid = (np.zeros(R, np.int32) for _ in range(4))
        hyps, refs = {}, {}
        for r in range(R):
            pair = output_transform(hyp[r], ref[r // group])
            if pair is None:
                continue
            h, g = pair
            b, p, _, _, tl, rlen = gb.compute_bleu([[g]], [h], smooth=True)
            bleu[r], prec[r], len_h[r], len_r[r], valid[r] = b, p, tl, rlen, 1
            poss = [max(len(h) - n + 1, 0) for n in range(1, 5)]
            m[r] = [int(round(p[n] * (poss[n] + 1.) - 1.)) for n in range(4)]
            rl[r] = rouge.calc_score([" ".join(h)], [" ".join(g)])
            lcs[r] = rg.my_lcs(g, h)
            hyps[r], refs[r] = [" ".join(h)], [" ".join(g)]
        corpus, avg, _ = gb.corpus_bleu(hyps, refs)
        rouge_mean, _ = rouge.compute_score(refs, hyps)
        bleu4 = np.sum(bleu[valid == 1]) / int(valid.sum())  # BLEU4.update / compute, restated
        crc = zlib.crc32(hyp.tobytes() + ref.tobytes())
        path = os.path.join(out_dir, f"seq_metrics_{name}.npz")
        np.savez_compressed(path, bleu=bleu, rouge=rl, precisions=prec, m=m, len_h=len_h, len_r=len_r, lcs=lcs,
                            valid=valid, agg=np.array([bleu4, corpus, avg, rouge_mean, valid.sum()], np.float64),
                            ids_crc=np.array([crc], np.uint32), group=np.array([group], np.int32))
        print(name, R, "rows", int(valid.sum()), "valid", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
