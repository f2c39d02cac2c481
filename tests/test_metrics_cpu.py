"""Validation metrics without a GPU: the loop oracle (tests/metric_ref.py) against the reference's own numbers
(tests/golden/seq_metrics_*.npz, tools/gen_metric_golden.py), the torch fallback of seq_metrics against the oracle,
SummaryMetrics against the golden aggregates (one process, and two gloo ranks), and the entry point's validation.

Rule everywhere: every integer field is exact; the scores agree to 1e-12 absolute (each is about twenty fp64 roundings
and two library log / exp calls on values <= 1, about 1e-14)."""
import ctypes
import os
import socket
import zlib

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import metric_ref as mr
from conftest import GOLDEN

TOL = 1e-12


def gold(name):
    with np.load(os.path.join(GOLDEN, f"seq_metrics_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def case_tensors(name):
    build, group = mr.CASES[name]
    hyp, ref = build()
    return torch.from_numpy(hyp), torch.from_numpy(ref), group


def assert_rows(got, name, what):
    """got: namespace(stats, bleu, rouge) of tensors; against the oracle of case `name`."""
    st, bleu, rouge = mr.oracle(name)
    assert got.stats.dtype == torch.int32 and got.bleu.dtype == torch.float64 and got.rouge.dtype == torch.float64
    np.testing.assert_array_equal(got.stats.cpu().numpy(), st, err_msg=what)
    assert np.abs(got.bleu.cpu().numpy() - bleu).max() <= TOL, what
    assert np.abs(got.rouge.cpu().numpy() - rouge).max() <= TOL, what


@pytest.mark.parametrize("name", list(mr.CASES))
def test_oracle_reproduces_the_reference(name):
    g = gold(name)
    build, group = mr.CASES[name]
    hyp, ref = build()
    assert zlib.crc32(hyp.tobytes() + ref.tobytes()) == int(g["ids_crc"][0]), "the case builder drifted from the golden"
    assert int(g["group"][0]) == group
    st, bleu, rouge = mr.oracle(name)
    ok = g["valid"] == 1
    np.testing.assert_array_equal(st[:, 11], g["valid"])
    np.testing.assert_array_equal(st[:, 0:4], g["m"])
    np.testing.assert_array_equal(st[:, 8], g["len_h"])
    np.testing.assert_array_equal(st[:, 9], g["len_r"])
    np.testing.assert_array_equal(st[:, 10], g["lcs"])
    prec = (st[:, 0:4] + 1.) / (st[:, 4:8] + 1.)
    np.testing.assert_array_equal(prec[ok], g["precisions"][ok])  # one fp64 division of the same integers
    assert not st[~ok].any() and not bleu[~ok].any() and not rouge[~ok].any()
    assert np.abs(bleu - g["bleu"]).max() <= TOL and np.abs(rouge - g["rouge"]).max() <= TOL
    agg = mr.aggregate(st, bleu, rouge)
    bleu4, corpus, avg, rouge_mean, n = g["agg"]
    assert agg["n"] == int(n)
    assert abs(agg["bleu"] - bleu4) <= TOL and abs(agg["bleu"] - avg) <= TOL
    assert abs(agg["corpus_bleu"] - corpus) <= TOL and abs(agg["rouge_l"] - rouge_mean) <= TOL


def test_special_rows_have_the_values_worked_out_by_hand():
    """The oracle and seq_metrics' fallback on the hand-written rows: the same record, and the values below."""
    from csa_amd.metric_ops import FIELDS, seq_metrics
    assert FIELDS == mr.FIELDS
    st, bleu, rouge = mr.oracle("special")
    got = seq_metrics(*(torch.from_numpy(a) for a in mr.special_case()), eos_id=mr.EOS_ID)
    np.testing.assert_array_equal(got.stats.numpy(), st)
    row = {n: (dict(zip(mr.FIELDS, st[i])), bleu[i], rouge[i]) for i, n in enumerate(mr.SPECIAL_NAMES)}
    f, b, r = row["clip_aaaa_vs_aa"]  # a a a a against a a: unigrams clip at 2, the bigram (a a) at 1
    assert [f[k] for k in mr.FIELDS] == [2, 1, 0, 0, 4, 3, 2, 1, 4, 2, 2, 1]
    f, b, r = row["identical"]
    assert b == 1.0 and r == 1.0 and f["m4"] == 3 and f["lcs"] == 6
    f, b, r = row["disjoint"]
    assert r == 0.0 and f["lcs"] == 0 and f["m1"] == 0 and abs(b - (1 / 360) ** 0.25) < TOL  # smoothing alone
    f, b, r = row["hyp_eos_at_0"]  # the placeholder token
    assert [f[k] for k in mr.FIELDS] == [0, 0, 0, 0, 1, 0, 0, 0, 1, 3, 0, 1] and r == 0.0
    for name in ("empty_reference", "both_empty"):
        f, b, r = row[name]
        assert not any(f.values()) and b == 0.0 and r == 0.0
    f, b, r = row["no_eos"]
    assert f["len_h"] == mr.SPECIAL_TH and f["len_r"] == mr.SPECIAL_TR
    f, b, r = row["above_2_31"]
    assert [f["m1"], f["m2"], f["m3"], f["lcs"]] == [3, 2, 1, 3]
    f, b, r = row["above_2_31_low_words_equal"]  # ids that differ only above bit 32 are different tokens
    assert f["m1"] == 1 and f["lcs"] == 1
    f, b, r = row["pad_and_unk_are_tokens"]
    assert f["len_h"] == 5 and f["m1"] == 4
    f, b, r = row["shorter_than_order"]
    assert [f["poss1"], f["poss2"], f["poss3"], f["poss4"]] == [2, 1, 0, 0] and [f["m3"], f["m4"]] == [0, 0]
    f, b, r = row["second_eos_ignored"]
    assert f["len_h"] == 2 and f["len_r"] == 4


def test_one_changed_id_changes_the_record():
    """The cases decide something: they are neither all-zero nor all-match, and one id moves the record."""
    for name in mr.CASES:
        st, bleu, rouge = mr.oracle(name)
        ok = st[:, 11] == 1
        assert ok.any() and (~ok).any(), name  # valid rows, and rows with an empty reference
        assert (st[ok, 0] > 0).any() and (st[ok, 0] < st[ok, 4]).any(), name  # some unigram matches, not all
        assert (bleu[ok] < 1).any() and (rouge[ok] > 0).any() and (rouge[ok] < 1).any(), name
    hyp, ref = (a.copy() for a in mr.special_case())
    i = mr.SPECIAL_NAMES.index("identical")
    base = mr.score_row(hyp[i], ref[i])
    hyp[i, 2] = 99
    moved = mr.score_row(hyp[i], ref[i])
    assert moved[0] != base[0] and moved[1] < base[1] and moved[2] < base[2]
    assert moved[0][:4] == [5, 3, 1, 0] and moved[0][10] == 5
    # and the op sees the same move
    from csa_amd.metric_ops import seq_metrics
    got = seq_metrics(torch.from_numpy(hyp[i:i + 1]), torch.from_numpy(ref[i:i + 1]), eos_id=mr.EOS_ID)
    assert got.stats[0].tolist() == moved[0]
    assert abs(float(got.bleu[0]) - moved[1]) <= TOL and abs(float(got.rouge[0]) - moved[2]) <= TOL


def test_rows_with_overlapping_or_strided_storage_are_copied_not_rejected():
    """An expanded reference (row stride 0) and a column-strided hypothesis are not views the kernel can take:
    _rows hands back rows with a unit last stride and a row stride of at least the width, and the result is that of
    the materialised rows."""
    from csa_amd import metric_ops
    hyp, ref = (torch.from_numpy(a) for a in mr.group_case(3))
    one = ref[4:5].expand(6, -1)
    assert one.stride(0) == 0
    r = metric_ops._rows(one, "ref")
    assert r.stride(0) >= r.shape[1] and r.stride(1) == 1 and torch.equal(r, one)
    wide = torch.stack([hyp[:6], hyp[6:12]], 2).reshape(6, -1)[:, ::2]  # hyp[:6] with a column stride of 2
    h = metric_ops._rows(wide, "hyp")
    assert h.stride(1) == 1 and torch.equal(h, hyp[:6])
    kept = metric_ops._rows(hyp[:, 1:], "hyp")  # a plain column slice stays a view
    assert kept.data_ptr() == hyp.data_ptr() + 8 and kept.stride(0) == hyp.shape[1]
    got = metric_ops.seq_metrics(wide, one, eos_id=mr.EOS_ID)
    want = mr.score(hyp[:6].numpy(), ref[4:5].numpy().repeat(6, 0), mr.EOS_ID, 1)
    np.testing.assert_array_equal(got.stats.numpy(), want[0])
    assert np.abs(got.bleu.numpy() - want[1]).max() <= TOL and np.abs(got.rouge.numpy() - want[2]).max() <= TOL


@pytest.mark.parametrize("name", list(mr.CASES))
def test_host_fallback_is_the_oracle(name):
    from csa_amd.metric_ops import seq_metrics
    hyp, ref, group = case_tensors(name)
    assert_rows(seq_metrics(hyp, ref, eos_id=mr.EOS_ID, group=group), name, name)
    assert_rows(seq_metrics(hyp, ref, eos_id=mr.EOS_ID, group=group, backend="host"), name, name + " host")


def test_host_fallback_takes_views_and_three_dims():
    from csa_amd.metric_ops import seq_metrics
    hyp, ref = (torch.from_numpy(a) for a in mr.group_case(3))
    st, bleu, rouge = mr.group_oracle(3)
    B, S, Th = 7, 3, mr.GROUP_TH
    ys = torch.full((B, S, Th + 1), 2, dtype=torch.int64)
    ys[:, :, 1:] = hyp[:B * S].view(B, S, Th)
    got = seq_metrics(ys[:, :, 1:], ref[:B], group=S)
    np.testing.assert_array_equal(got.stats.numpy(), st[:B * S])
    assert np.abs(got.bleu.numpy() - bleu[:B * S]).max() <= TOL
    with pytest.raises(ValueError):
        seq_metrics(ys[:, :, 1:], ref[:B], group=1)
    with pytest.raises(ValueError):
        seq_metrics(hyp[:6], ref[:4], group=3)
    with pytest.raises(ValueError):
        seq_metrics(hyp[:6].int(), ref[:2], group=3)
    with pytest.raises(ValueError):
        seq_metrics(hyp[:6], ref[:2], group=3, backend="gpu")
    from csa_amd._lib import CsaError
    with pytest.raises(CsaError):
        seq_metrics(hyp[:6], ref[:2], group=3, backend="device")  # CPU tensors


def _expect(names):
    """The aggregate over the rows of several cases, from the golden per-row numbers."""
    st = np.concatenate([mr.oracle(n)[0] for n in names])
    return mr.aggregate(st, np.concatenate([gold(n)["bleu"] for n in names]),
                        np.concatenate([gold(n)["rouge"] for n in names]))


def assert_summary(got, want):
    assert got.n == want["n"]
    for k in ("bleu", "corpus_bleu", "rouge_l"):
        assert abs(getattr(got, k) - want[k]) <= TOL, k


def test_summary_metrics_accumulates_to_the_golden_aggregates():
    from csa_amd.metrics import NotComputableError, SummaryMetrics
    from csa_amd.model import SummaryMetrics as beside_the_generators, evaluate  # noqa: F401 (the re-export)
    assert beside_the_generators is SummaryMetrics
    sm = SummaryMetrics(eos_id=mr.EOS_ID)
    with pytest.raises(NotComputableError):
        sm.compute()
    for name in mr.CASES:  # one case alone: the golden file's own aggregates
        sm.reset()
        hyp, ref, group = case_tensors(name)
        out = sm.update(hyp, ref, group=group)
        assert out.stats.shape == (hyp.shape[0], 12)
        bleu4, corpus, avg, rouge_mean, n = gold(name)["agg"]
        assert_summary(sm.compute(), {"bleu": bleu4, "corpus_bleu": corpus, "rouge_l": rouge_mean, "n": int(n)})
    sm.reset()
    assert sm.counts.dtype == torch.int64 and sm.counts.shape == (12,) and not sm.counts.any()
    assert sm.scores.dtype == torch.float64 and sm.scores.shape == (2,) and not sm.scores.any()
    names = ["special", "len64", "group3", "wide"]
    for name in names:  # several updates of different widths and groups
        hyp, ref, group = case_tensors(name)
        sm.update(hyp, ref, group=group)
    assert_summary(sm.compute(), _expect(names))
    assert_summary(sm.compute(), _expect(names))  # compute changes nothing
    # only invalid rows: nothing to compute
    sm.reset()
    sm.update(torch.tensor([[5, 6, 3]]), torch.tensor([[3, 5, 6]]))
    with pytest.raises(NotComputableError):
        sm.compute()


class _FixedGenerator:
    """Stands in for a generator: returns prepared ids per batch (a tuple when `extras`)."""
    eos_id = mr.EOS_ID

    def __init__(self, outs, extras=False):
        self.outs, self.extras, self.calls = list(outs), extras, 0

    def __call__(self, data, **kw):
        ids = self.outs[data]
        self.calls += 1
        return (ids, None) if self.extras else ids


def test_evaluate_takes_the_first_row_or_the_whole_group():
    from csa_amd.metrics import SummaryMetrics, evaluate
    hyp, ref = (torch.from_numpy(a) for a in mr.group_case(3))
    st, bleu, rouge = mr.group_oracle(3)
    B, S = 10, 3
    h3 = hyp.view(-1, S, mr.GROUP_TH)
    batches = [(i, ref[i * B:(i + 1) * B]) for i in range(3)]
    outs = [h3[i * B:(i + 1) * B] for i in range(3)]
    n = 3 * B
    first = np.arange(n) * S
    want_first = mr.aggregate(st[first], bleu[first], rouge[first])
    want_all = mr.aggregate(st[:n * S], bleu[:n * S], rouge[:n * S])
    assert_summary(evaluate(_FixedGenerator(outs), batches), want_first)
    assert_summary(evaluate(_FixedGenerator(outs, extras=True), batches), want_first)
    assert_summary(evaluate(_FixedGenerator([o[:, 0] for o in outs]), batches), want_first)
    sm = SummaryMetrics(mr.EOS_ID)
    assert_summary(evaluate(_FixedGenerator(outs), batches, metrics=sm, group=S), want_all)
    assert int(sm.counts[11]) == want_all["n"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    import torch.distributed as dist

    from csa_amd.metrics import SummaryMetrics
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sm = SummaryMetrics(mr.EOS_ID)
    for name in (("len64", "special") if rank == 0 else ("group3",)):  # unequal shards, different groups
        build, group = mr.CASES[name]
        hyp, ref = build()
        sm.update(torch.from_numpy(hyp), torch.from_numpy(ref), group=group)
    local = sm.compute()
    both = sm.compute(process_group=dist.group.WORLD)
    again = sm.compute()  # the reduction ran on copies
    q.put((rank, (vars(local), vars(both), vars(again))))
    dist.barrier()
    dist.destroy_process_group()


def test_compute_on_two_gloo_ranks_equals_one_rank_with_all_rows():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    from types import SimpleNamespace
    want = _expect(["len64", "special", "group3"])
    for rank, shard in ((0, ["len64", "special"]), (1, ["group3"])):
        local, both, again = (SimpleNamespace(**d) for d in res[rank])
        assert_summary(local, _expect(shard))
        assert_summary(both, want)
        assert vars(again) == vars(local)
    assert res[0][1] == res[1][1]  # the same fp64 sums on both ranks


def test_seq_metrics_entry_point_validates_without_gpu():
    from csa_amd import _lib
    L = _lib.lib()
    err = L.csa_last_error_str
    assert L.csa_abi_version() == 10
    assert "csa_seq_metrics" in _lib.EXPORTED_SYMBOLS and "csa_seq_metrics_supported" in _lib.EXPORTED_SYMBOLS
    for ok in ((1, 1), (49, 49), (256, 256), (1, 256), (256, 1)):
        assert L.csa_seq_metrics_supported(*ok), ok
    for bad in ((0, 5), (5, 0), (257, 5), (5, 257), (-1, 5)):
        assert not L.csa_seq_metrics_supported(*bad), bad
    assert L.csa_seq_metrics(None, None) == 1 and b"csa_seq_metrics" in err() and b"null args" in err()

    def call(**kw):
        base = dict(hyp=16, rows=6, Th=9, hyp_stride=10, ref=16, Tr=7, ref_stride=7, group=3, eos_id=3, stats=16, bleu=16,
                    rouge=16)
        base.update(kw)
        a = _lib.CsaSeqMetricsArgs(**base)
        return L.csa_seq_metrics(ctypes.byref(a), None)
    for name in ("hyp", "ref", "stats", "bleu", "rouge"):
        assert call(**{name: None}) == 1 and b"csa_seq_metrics" in err() and b"null pointer" in err(), name
    for name in ("rows", "Th", "Tr"):
        assert call(**{name: -1}) == 1 and b"negative" in err(), name
    assert call(rows=1 << 31, group=1) == 1 and b"rows" in err()
    for g in (0, -1, 4):
        assert call(group=g) == 1 and b"group" in err(), g
    assert call(hyp_stride=8) == 1 and b"stride" in err()
    assert call(ref_stride=6) == 1 and b"stride" in err()
    for kw in (dict(Th=0), dict(Tr=0), dict(Th=257, hyp_stride=300), dict(Tr=257, ref_stride=300)):
        assert call(**kw) == 2 and b"Th and Tr must be in [1, 256]" in err(), kw
    for name, bad in (("hyp", 20), ("ref", 12), ("stats", 18), ("bleu", 20), ("rouge", 12)):
        assert call(**{name: bad}) == 1 and b"misaligned" in err(), name
    assert call(rows=0) == 0  # nothing to do, no launch
