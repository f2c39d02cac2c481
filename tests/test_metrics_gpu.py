"""Validation metrics on the GPU: k_seq_metrics<1 | 2 | 4> (csrc/csa_metric.hip) against the loop oracle
(tests/metric_ref.py), which tests/test_metrics_cpu.py pins to the reference's numbers. Every integer field is exact
and both scores agree to 1e-12 absolute: each score is about twenty fp64 roundings and two library log / exp calls on
values <= 1, about 1e-14; the margin covers library ulp differences.

The launch classes are the word counts NW = ceil(max(Th, Tr) / 64) in {1, 2, 4}, named nw1 / nw2 / nw4 in the ids."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import metric_ref as mr
from conftest import has_gpu
from golden_inputs import fill_params_deterministic

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]

TOL = 1e-12
SENT_I, SENT_F = -777, -777.25
PAD_ROWS = 5  # sentinel rows in front of and behind each output


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_rows(got, want, what, rows=slice(None)):
    st, bleu, rouge = (w[rows] for w in want)
    assert got.stats.dtype == torch.int32 and got.bleu.dtype == torch.float64 and got.rouge.dtype == torch.float64
    assert got.stats.is_cuda
    g = got.stats.cpu().numpy()
    assert g.shape == st.shape, what
    bad = np.argwhere(g != st)
    assert not len(bad), f"{what}: row {bad[0][0]} got {g[bad[0][0]]} want {st[bad[0][0]]}"
    eb = np.abs(got.bleu.cpu().numpy() - bleu).max()
    er = np.abs(got.rouge.cpu().numpy() - rouge).max()
    print(f"{what}: max |bleu err| {eb:.3e}, max |rouge err| {er:.3e}")
    assert eb <= TOL and er <= TOL, what


def launch_raw(hyp, ref, group, eos=mr.EOS_ID):
    """csa_seq_metrics through the C ABI into caller buffers with sentinel rows on both sides of every output.
    -> (namespace of the result views, the three whole buffers)."""
    from csa_amd import _lib
    R, B = hyp.shape[0], ref.shape[0]
    stats = torch.full((R + 2 * PAD_ROWS, 12), SENT_I, dtype=torch.int32, device="cuda")
    bleu = torch.full((R + 2 * PAD_ROWS,), SENT_F, dtype=torch.float64, device="cuda")
    rouge = bleu.clone()
    a = _lib.CsaSeqMetricsArgs(hyp=hyp.data_ptr(), rows=R, Th=hyp.shape[1], hyp_stride=hyp.stride(0), ref=ref.data_ptr(),
                               Tr=ref.shape[1], ref_stride=ref.stride(0), group=group, eos_id=eos,
                               stats=stats[PAD_ROWS:].data_ptr(), bleu=bleu[PAD_ROWS:].data_ptr(),
                               rouge=rouge[PAD_ROWS:].data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().csa_seq_metrics(ctypes.byref(a), stream), "csa_seq_metrics")
    view = SimpleNamespace(stats=stats[PAD_ROWS:PAD_ROWS + R], bleu=bleu[PAD_ROWS:PAD_ROWS + R],
                           rouge=rouge[PAD_ROWS:PAD_ROWS + R])
    return view, (stats, bleu, rouge)


def assert_sentinels(bufs, R, what):
    for buf, s in zip(bufs, (SENT_I, SENT_F, SENT_F)):
        assert bool((buf[:PAD_ROWS] == s).all()) and bool((buf[PAD_ROWS + R:] == s).all()), what
        assert not bool((buf[PAD_ROWS:PAD_ROWS + R] == s).any()), what  # every row was written


LAUNCH_CLASSES = [("nw1", "len64"), ("nw2", "len128"), ("nw4", "len256")]


@pytest.mark.parametrize("cls,name", LAUNCH_CLASSES, ids=[c for c, _ in LAUNCH_CLASSES])
def test_kernel_is_the_oracle_over_the_length_grid(cls, name):
    """Every (len_h, len_r) pair of {0..5, 63, 64, 65, 127, 128, 129, 255, 256} that fits the class's width: the empty
    placeholder, fewer tokens than the order, the word boundaries and the width limit (a row without EOS); 3-token,
    12-token and ~1000-token vocabularies and ids above 2^31."""
    from csa_amd.metric_ops import seq_metrics
    build, group = mr.CASES[name]
    hyp, ref = (cuda(a) for a in build())
    assert (max(hyp.shape[1], ref.shape[1]) + 63) // 64 == int(cls[2:])
    want = mr.oracle(name)
    assert_rows(seq_metrics(hyp, ref, eos_id=mr.EOS_ID, group=group, backend="device"), want, f"{cls} op")
    got, bufs = launch_raw(hyp, ref, group)
    assert_rows(got, want, f"{cls} raw")
    assert_sentinels(bufs, hyp.shape[0], cls)


def test_special_rows():
    """a a a a against a a, identical and disjoint rows, EOS at column 0, an empty reference, no EOS, ids above 2^31,
    PAD / UNK as tokens, a second EOS; widths 9 and 7 (nw1, Th != Tr)."""
    hyp, ref = (cuda(a) for a in mr.special_case())
    got, bufs = launch_raw(hyp, ref, 1)
    assert_rows(got, mr.oracle("special"), "special")
    assert_sentinels(bufs, hyp.shape[0], "special")
    i = mr.SPECIAL_NAMES.index("identical")
    assert float(got.bleu[i]) == 1.0 and float(got.rouge[i]) == 1.0
    i = mr.SPECIAL_NAMES.index("clip_aaaa_vs_aa")
    assert got.stats[i].tolist() == [2, 1, 0, 0, 4, 3, 2, 1, 4, 2, 2, 1]
    i = mr.SPECIAL_NAMES.index("empty_reference")
    assert not got.stats[i].any() and float(got.bleu[i]) == 0.0 and float(got.rouge[i]) == 0.0


@pytest.mark.parametrize("cls,wide_side", [("nw4", "ref"), ("nw4", "hyp"), ("nw2", "ref")],
                         ids=["nw4_short_hyp", "nw4_short_ref", "nw2_short_hyp"])
def test_unequal_widths_take_the_class_of_the_wider_side(cls, wide_side):
    """The class follows max(Th, Tr): 9-wide rows against 256- or 128-wide ones, on either side, and an eos_id that
    is not 3."""
    from csa_amd.metric_ops import seq_metrics
    small_h, small_r = mr.special_case()
    big_h, big_r = mr.length_case(256 if cls == "nw4" else 128)
    n = len(small_h)
    pick = np.linspace(0, len(big_h) - 1, n).astype(int)
    hyp, ref = (small_h, big_r[pick]) if wide_side == "ref" else (big_h[pick], small_r)
    for eos in (mr.EOS_ID, 6):
        want = mr.score(hyp, ref, eos, 1)
        assert_rows(seq_metrics(cuda(hyp), cuda(ref), eos_id=eos, backend="device"), want, f"{cls} {wide_side} eos={eos}")


@pytest.mark.parametrize("group", mr.GROUPS)
def test_row_counts_and_groups(group):
    """B in {1, 63, 64, 65, 257} references with `group` hypotheses each: hypothesis row r reads reference r // group."""
    from csa_amd.metric_ops import seq_metrics
    hyp, ref = (cuda(a) for a in mr.group_case(group))
    want = mr.group_oracle(group)
    for B in mr.ROW_COUNTS:
        R = B * group
        got, bufs = launch_raw(hyp[:R], ref[:B], group)
        assert_rows(got, want, f"G={group} B={B}", slice(0, R))
        assert_sentinels(bufs, R, f"G={group} B={B}")
    assert_rows(seq_metrics(hyp, ref, eos_id=mr.EOS_ID, group=group, backend="device"), want, f"G={group} op")


def test_strided_views_are_read_in_place():
    """A sampler's (B, S, T-1) result and ys[:, 1:] are views of a wider buffer: the op takes them without a copy and
    reads the right columns."""
    from csa_amd import metric_ops
    hyp, ref = mr.group_case(3)
    want = mr.group_oracle(3)
    B, S, Th = 65, 3, mr.GROUP_TH
    ys = torch.full((B, S, Th + 1), mr.EOS_ID, dtype=torch.int64, device="cuda")  # column 0 would end every row
    ys[:, :, 1:] = cuda(hyp[:B * S]).view(B, S, Th)
    view = ys[:, :, 1:]
    rows = metric_ops._rows(view, "hyp")
    assert rows.data_ptr() == ys.data_ptr() + 8 and rows.stride(0) == Th + 1
    rbuf = torch.full((B, mr.GROUP_TR + 3), mr.EOS_ID, dtype=torch.int64, device="cuda")
    rbuf[:, 2:-1] = cuda(ref[:B])
    got = metric_ops.seq_metrics(view, rbuf[:, 2:-1], eos_id=mr.EOS_ID, group=S, backend="device")
    assert_rows(got, want, "(B, S, T-1) view", slice(0, B * S))
    ys2 = ys.view(B * S, Th + 1)
    got = metric_ops.seq_metrics(ys2[:, 1:], cuda(ref[:B]), eos_id=mr.EOS_ID, group=S, backend="device")
    assert_rows(got, want, "ys[:, 1:] view", slice(0, B * S))
    raw, bufs = launch_raw(ys2[:, 1:], rbuf[:, 2:-1], S)
    assert_rows(raw, want, "raw views", slice(0, B * S))
    assert_sentinels(bufs, B * S, "raw views")
    # an expanded reference (row stride 0) is no such view: the op copies it and still runs the kernel
    one = cuda(ref[4:5]).expand(6, -1)
    got = metric_ops.seq_metrics(cuda(hyp[:6]), one, eos_id=mr.EOS_ID, backend="device")
    assert_rows(got, mr.score(hyp[:6], ref[4:5].repeat(6, 0), mr.EOS_ID, 1), "expanded reference")


def test_wider_rows_take_the_fallback_on_the_device():
    from csa_amd._lib import CsaError
    from csa_amd.metric_ops import seq_metrics
    hyp, ref = (cuda(a) for a in mr.wide_case())
    got = seq_metrics(hyp, ref, eos_id=mr.EOS_ID, group=2)
    assert_rows(got, mr.oracle("wide"), "wide")
    with pytest.raises(CsaError):
        seq_metrics(hyp, ref, eos_id=mr.EOS_ID, group=2, backend="device")
    # the fallback and the kernel agree where both run
    h2, r2 = (cuda(a) for a in mr.length_case(128))
    assert_rows(seq_metrics(h2, r2, eos_id=mr.EOS_ID, backend="host"), mr.oracle("len128"), "len128 host on cuda")


def test_summary_metrics_on_the_device():
    from csa_amd.metrics import SummaryMetrics
    sm = SummaryMetrics(mr.EOS_ID)
    names = ["special", "len64", "len256", "group3", "wide"]
    for name in names:
        build, group = mr.CASES[name]
        hyp, ref = (cuda(a) for a in build())
        sm.update(hyp, ref, group=group)
    assert sm.counts.is_cuda and sm.scores.is_cuda
    parts = [mr.oracle(n) for n in names]
    want = mr.aggregate(*(np.concatenate([p[i] for p in parts]) for i in range(3)))
    got = sm.compute()
    assert got.n == want["n"]
    for k in ("bleu", "corpus_bleu", "rouge_l"):
        assert abs(getattr(got, k) - want[k]) <= TOL, k


# ---- end to end on a tiny model ----

TINY = dict(src_vocab_size=50, tgt_vocab_size=60, hidden_size=64, num_heads=8, num_layers=1, sbm_layers=2,
            use_pegen="pegen", dim_feed_forward=128, dropout=0.2, pe_dim=32, pegen_dim=128, sbm_enc_dim=512,
            clusters=[10, 12], full_att=False)
E2E_B, E2E_N, E2E_T = 4, 16, 12


def _tiny():
    from csa_amd.data import synthetic_batch
    from csa_amd.model import CSATrans, batch_to_device
    m = CSATrans(**TINY)
    fill_params_deterministic(m, 5)
    with torch.no_grad():
        m.generator.linear.weight.mul_(8.0)
    m = m.cuda().eval()
    batches = []
    for seed in (11, 12):
        data, target = batch_to_device(synthetic_batch(E2E_B, max_size=E2E_N, seed=seed, min_nodes=9, src_vocab=50,
                                                       tgt_vocab=12, max_tgt_len=E2E_T), torch.device("cuda"))
        data.tgt_seq = None
        batches.append((data, target))
    return m, batches


class _Recording:
    """A generator that keeps what it returned, so the oracle can score the same ids."""

    def __init__(self, gen):
        self.gen, self.eos_id, self.ids = gen, getattr(gen, "eos_id", None), []

    def __call__(self, data, **kw):
        torch.manual_seed(0)  # the encoder's graph sampling key
        out = self.gen(data, **kw)
        self.ids.append(out)
        return out


def test_evaluate_with_the_graph_generator_is_the_oracle_on_the_same_ids():
    from csa_amd.model import CachedGreedyGenerator, evaluate
    m, batches = _tiny()
    gen = _Recording(CachedGreedyGenerator(m, E2E_T, graph=True))
    got = evaluate(gen, batches)
    assert len(gen.ids) == 2 and gen.ids[0].shape == (E2E_B, E2E_T - 1)
    hyp = np.concatenate([i.cpu().numpy() for i in gen.ids])
    ref = np.concatenate([t.cpu().numpy() for _, t in batches])
    want = mr.aggregate(*mr.score(hyp, ref, mr.EOS_ID, 1))
    assert got.n == want["n"] == 2 * E2E_B
    for k in ("bleu", "corpus_bleu", "rouge_l"):
        assert abs(getattr(got, k) - want[k]) <= TOL, k


def test_update_on_a_beams_n_best_list_equals_one_call_per_rank():
    from csa_amd.model import BeamSearchGenerator, SummaryMetrics
    m, batches = _tiny()
    W = 3
    data, target = batches[0]
    torch.manual_seed(0)
    best, ids, scores = BeamSearchGenerator(m, E2E_T, W)(data, return_all=True)
    assert ids.shape == (E2E_B, W, E2E_T - 1)
    whole, parts = SummaryMetrics(), SummaryMetrics()
    out = whole.update(ids, target, group=W)
    assert_rows(out, mr.score(ids.reshape(-1, E2E_T - 1).cpu().numpy(), target.cpu().numpy(), mr.EOS_ID, W), "beam")
    for w in range(W):
        o = parts.update(ids[:, w], target)
        assert torch.equal(o.stats, out.stats[w::W]) and torch.equal(o.bleu, out.bleu[w::W])
        assert torch.equal(o.rouge, out.rouge[w::W])
    assert torch.equal(whole.counts, parts.counts)
    a, b = whole.compute(), parts.compute()
    assert a.n == b.n == E2E_B * W and a.corpus_bleu == b.corpus_bleu
    assert abs(a.bleu - b.bleu) <= TOL and abs(a.rouge_l - b.rouge_l) <= TOL  # fp64 sums in another order
