"""Validation metrics over decoded ids, accumulated on the device (csa_amd.metric_ops.seq_metrics, csrc/csa_metric.hip).

SummaryMetrics replaces the reference's BLEU4 metric (valid_metrices/bleu_metrice.py: the mean smoothed sentence BLEU-4
that picks the best checkpoint) and the BLEU / ROUGE-L half of eval_accuracies (valid_metrices/compute_scores.py) without
a vocabulary, a host copy per batch or a sync per batch: update() launches one kernel on the ids as the generators
leave them and adds into two device tensors; compute() is the only place that reads them. METEOR is out of scope (the
reference shells out to a Java jar and WordNet data).

evaluate() runs a generator over (data, target) batches and returns compute()'s result: one host sync per call."""
from types import SimpleNamespace

import torch

from .metric_ops import bleu_from_counts, seq_metrics

__all__ = ["SummaryMetrics", "evaluate"]


class NotComputableError(RuntimeError):
    """compute() before any valid row was seen (the reference raises ignite's error of this name)."""


class SummaryMetrics:
    """Running BLEU-4 / ROUGE-L state on the device: counts (12,) int64 = the sums of the eleven count fields of
    seq_metrics' stats (m1..m4, poss1..poss4, len_h, len_r, lcs) and the number of valid rows; scores (2,) fp64 = the
    sums of the sentence BLEU and ROUGE-L. Rows whose reference is empty are left out of everything, as
    bleu_output_transform drops them. The state is created on the device of the first update."""

    def __init__(self, eos_id=3):
        self.eos_id = int(eos_id)
        self.counts = None
        self.scores = None

    def reset(self):
        if self.counts is not None:
            self.counts.zero_()
            self.scores.zero_()

    def update(self, hyp, ref, group=1):
        """Scores hyp (R, Th) or (B, group, Th) against ref (B, Tr) and adds the rows into the state; no .item(), no
        sync. -> the per-row namespace(stats, bleu, rouge) of seq_metrics, e.g. to re-rank an n-best list or take its
        oracle BLEU."""
        out = seq_metrics(hyp, ref, eos_id=self.eos_id, group=group)
        if self.counts is None:
            self.counts = torch.zeros(12, dtype=torch.int64, device=out.stats.device)
            self.scores = torch.zeros(2, dtype=torch.float64, device=out.stats.device)
        elif self.counts.device != out.stats.device:
            raise ValueError("SummaryMetrics.update: the state lives on another device than these ids")
        self.counts += out.stats.sum(0, dtype=torch.int64)  # invalid rows are all zeros
        self.scores += torch.stack([out.bleu.sum(), out.rouge.sum()])
        return out

    def compute(self, process_group=None):
        """-> namespace(bleu, corpus_bleu, rouge_l, n) of Python numbers: the mean sentence BLEU-4 over valid rows (the
        reference's validation BLEU4), compute_bleu(smooth=True) over the summed counts (the first value of
        google_bleu.corpus_bleu), the mean ROUGE-L, and the number of valid rows. With a process group the two state
        tensors are SUM-reduced first, on copies: the local state is left as it is. The only method that
        synchronises."""
        if self.counts is None:
            raise NotComputableError("SummaryMetrics must have at least one example before it can be computed.")
        counts, scores = self.counts, self.scores
        if process_group is not None:
            import torch.distributed as dist
            counts, scores = counts.clone(), scores.clone()
            dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=process_group)
            dist.all_reduce(scores, op=dist.ReduceOp.SUM, group=process_group)
        corpus = bleu_from_counts(counts[0:4], counts[4:8], counts[8], counts[9].clamp(min=1))
        host = torch.cat([counts.double(), scores, corpus.reshape(1)]).cpu()  # one copy: the sync
        n = int(host[11])
        if n == 0:
            raise NotComputableError("SummaryMetrics must have at least one example before it can be computed.")
        return SimpleNamespace(bleu=float(host[12]) / n, corpus_bleu=float(host[14]), rouge_l=float(host[13]) / n, n=n)


def _ids(out):
    """The ids of a generator's result: the tensor itself, or the first element of a tuple (a beam's best row with
    return_all, a generator's ids with return_logp)."""
    return out[0] if isinstance(out, (tuple, list)) else out


def evaluate(generator, batches, metrics=None, group=None, **gen_kw):
    """Decodes every (data, target) batch with `generator` and scores the ids against target (B, Tr): the ids are
    generator(data, **gen_kw), or the first element when that is a tuple. A (B, S, T-1) result (a sampler with
    num_samples = S, a beam's n-best ids) is scored on its first row per AST unless group=S is passed, which scores all
    S rows against the same reference. -> metrics.compute(); `metrics` (a fresh SummaryMetrics of the generator's eos_id
    by default) keeps the state afterwards. One host sync per call, in compute()."""
    if metrics is None:
        eos = getattr(generator, "eos_id", None)
        metrics = SummaryMetrics(3 if eos is None else eos)
    with torch.no_grad():
        for data, target in batches:
            ids = _ids(generator(data, **gen_kw))
            if ids.dim() == 3 and group is None:
                ids = ids[:, 0]
            metrics.update(ids, target, group=1 if group is None else group)
    return metrics.compute()
