"""Beam search on the GPU: k_beam_row_topk and k_beam_select (csrc/csa_beam.hip) and the BEAM form of k_decode_attn
(csrc/csa_decode.hip) against torch / numpy, and BeamSearchGenerator against the greedy fixture
(tests/golden/greedy_tiny.npz), the uncached oracle (tests/beam_ref.py), its own captured graph, and at the production
head dim with the HIP and fallback calls counted."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import beam_ref
from beam_ref import (EOS_ID, STEP_TOL, assert_oracle_is_decisive, assert_run_is_interesting, assert_select_equal,
                      expected_select, greedy_ids_ref, run_select, search_case)
from conftest import has_gpu
from golden_inputs import fill_params_deterministic

# the model of tests/golden/greedy_tiny.npz (the same dims as test_decode_gpu.TINY)
TINY = dict(src_vocab_size=50, tgt_vocab_size=60, hidden_size=64, num_heads=8, num_layers=1, sbm_layers=2,
            use_pegen="pegen", dim_feed_forward=128, dropout=0.2, pe_dim=32, pegen_dim=128, sbm_enc_dim=512,
            clusters=[10, 12], full_att=False)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]

SENTINEL = 777.0


# ---- row top-W ----

def _check_topk(x, W, what):
    from csa_amd.decode_ops import beam_row_topk
    lse, tv, ti = beam_row_topk(x.cuda(), W)
    rl, rv, ri = beam_ref.row_topk_np(x.numpy(), W)
    np.testing.assert_array_equal(ti.cpu().numpy(), ri, err_msg=what)
    np.testing.assert_allclose(tv.cpu().numpy(), rv, rtol=1e-4, atol=1e-5, err_msg=what)
    np.testing.assert_allclose(lse.cpu().numpy(), rl, rtol=1e-4, atol=1e-5, err_msg=what)
    return ti.cpu()


@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("V", ["W", 60, 1023, 20000])
def test_beam_row_topk(rows, V):
    for W in (1, 4, 8):
        v = W if V == "W" else V
        g = torch.Generator().manual_seed(rows * 100003 + v)
        x = (torch.randperm(rows * v, generator=g).float() - rows * v / 2).view(rows, v)  # distinct values
        _check_topk(x, W, f"W={W} plain")
        _check_topk(x / (rows * v) * 8, W, f"W={W} small range")  # a row whose sum of exponentials has many terms
        for at in (0, v - 1):  # the maximum planted at either end
            y = x.clone()
            y[:, at] = 1e9
            assert bool((_check_topk(y, W, f"W={W} max at {at}")[:, 0] == at).all())
        if v >= 60:  # duplicated maxima: the lowest index first, wherever the copies sit
            y = x.clone()
            y[:, torch.tensor([v - 1, v // 2, 7, 41])] = 1e9
            want = sorted([v - 1, v // 2, 7, 41])[:W]
            assert _check_topk(y, W, f"W={W} duplicates")[0, :len(want)].tolist() == want[:W]
        y = x.clone()
        y[rows // 2] = float("-inf")  # an all -inf row gives 0 .. W-1
        assert _check_topk(y, W, f"W={W} all -inf row")[rows // 2].tolist() == list(range(W))
        y = x.clone()
        y[:, ::2] = float("-inf")     # a row with -inf entries (fewer than W finite ones when V = W)
        _check_topk(y, W, f"W={W} -inf entries")


def test_beam_row_topk_obeys_the_device_counter():
    from csa_amd.decode_ops import beam_row_topk
    x = torch.randn(3, 60, generator=torch.Generator().manual_seed(1)).cuda()
    want = beam_row_topk(x, 4)
    for t, stores in ((0, True), (4, True), (5, False), (-1, False), (1 << 30, False)):
        out = (torch.full((3,), SENTINEL, device="cuda"), torch.full((3, 4), SENTINEL, device="cuda"),
               torch.full((3, 4), -9, dtype=torch.int32, device="cuda"))
        beam_row_topk(x, 4, *out, t_dev=torch.tensor([t], dtype=torch.int32, device="cuda"), t_end=5)
        if stores:
            assert all(torch.equal(a, b) for a, b in zip(out, want)), t
        else:
            assert bool((out[0] == SENTINEL).all() and (out[1] == SENTINEL).all() and (out[2] == -9).all()), t


# ---- select ----

@pytest.mark.parametrize("name,state,claim", beam_ref.select_states(), ids=[s[0] for s in beam_ref.select_states()])
def test_beam_select_on_hand_built_states(name, state, claim):
    want = expected_select(state)
    assert claim(want[5], want[1], want[2], want[3]), f"{name}: the state does not show what it is built for"
    assert_select_equal(run_select(state, device="cuda"), want, name)


def test_beam_select_stores_nothing_for_a_counter_outside_its_range():
    _, state, _ = beam_ref.select_states()[3]
    before = (state["cum"], state["fin"], state["tokens"], state["pad"], state["anc"],
              np.full(state["cum"].shape, -1, dtype=np.int32))
    for t in (-1, state["T"] - 1, state["T"], 1 << 30):
        assert_select_equal(run_select(state, device="cuda", t=t), before, f"t={t}")


# ---- attention through the ancestry table / a shared memory ----

def _ref_attention(q, k, v, mask, n):
    """fp64 on the CPU: q (R,H,hd), k / v (R,H,n,hd), mask (R,>=n) uint8 or None -> (R, H*hd)."""
    q, k, v = q.double(), k.double(), v.double()
    s = torch.einsum("bhd,bhjd->bhj", q, k) * q.shape[-1] ** -0.5
    if mask is not None:
        s = s.masked_fill(mask[:, None, :n].bool(), float("-inf"))
    return torch.einsum("bhj,bhjd->bhd", s.softmax(-1), v).reshape(q.shape[0], -1)


# (hd, keys); the last four: hd / 4 = 1, 3, 24 and 5 (3, 24 and 5 do not divide the wave), see test_decode_gpu.CASES
ATTN_CASES = [(8, 1), (8, 7), (64, 64), (64, 65), (128, 130), (4, 70), (12, 65), (96, 150), (20, 130)]


@pytest.mark.parametrize("W", [1, 3, 4])
@pytest.mark.parametrize("hd,n", ATTN_CASES)
def test_decode_attention_follows_the_ancestry_table(hd, n, W):
    """Self form: a random ancestry table inside each AST's W rows against the existing kernel on a cache gathered
    physically with torch (bitwise), and against fp64; only row (r, t) of the physical cache is written."""
    from csa_amd.decode_ops import decode_attention
    g = torch.Generator().manual_seed(1000 * n + hd + W)
    B, H, t, cap = 2, 2, n - 1, n + 3
    R = B * W
    q, kn, vn = torch.randn(R, 3, H, hd, generator=g).unbind(1)
    cache = torch.full((2, R, H, cap, hd), SENTINEL)
    cache[:, :, :, :t] = torch.randn(2, R, H, t, hd, generator=g)
    anc = torch.full((R, cap + 2), 1 << 20, dtype=torch.int32)[:, :cap]  # row stride above the capacity
    anc[:, :t] = (torch.arange(R)[:, None] // W) * W + torch.randint(0, W, (R, t), generator=g)
    gathered = cache.clone()
    for j in range(t):
        gathered[:, :, :, j] = cache[:, anc[:, j].long(), :, j]
    mask = (torch.rand(R, cap + 5, generator=g) < 0.4).to(torch.uint8)
    mask[:, 0] = 0
    for name, m in (("none", None), ("random", mask)):
        dm = None if m is None else m.cuda()
        for step in (t, torch.tensor([t], dtype=torch.int32, device="cuda")):
            dg, dc = gathered.cuda(), cache.cuda()
            want = decode_attention(q.cuda(), dg[0], dg[1], key_mask=dm, k_new=kn.cuda(), v_new=vn.cuda(), t=step)
            got = decode_attention(q.cuda(), dc[0], dc[1], key_mask=dm, k_new=kn.cuda(), v_new=vn.cuda(), t=step,
                                   anc=anc.cuda())
            assert torch.equal(got, want), name
            after = dc.cpu()
            assert torch.equal(after[0, :, :, t], kn) and torch.equal(after[1, :, :, t], vn), name
            assert torch.equal(after[:, :, :, :t], cache[:, :, :, :t]), name
            assert bool((after[:, :, :, t + 1:] == SENTINEL).all()), name
        ref = _ref_attention(q, torch.cat([gathered[0, :, :, :t], kn[:, :, None]], 2),
                             torch.cat([gathered[1, :, :, :t], vn[:, :, None]], 2), m, n)
        np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-5, err_msg=name)


@pytest.mark.parametrize("W", [1, 3, 4])
@pytest.mark.parametrize("hd,n", ATTN_CASES)
def test_decode_attention_shares_one_memory_per_group(hd, n, W):
    """Cross form: kv_group = W against the memory repeated W times (bitwise) and fp64, without a mask and with a
    mask whose row stride exceeds n."""
    from csa_amd.decode_ops import decode_attention
    g = torch.Generator().manual_seed(2000 * n + hd + W)
    B, H = 2, 3
    R = B * W
    q = torch.randn(R, H, hd, generator=g)
    kv = torch.randn(B, n, 2, H, hd, generator=g)
    mask = (torch.rand(B, n + 5, generator=g) < 0.4).to(torch.uint8)
    mask[:, 0] = 0
    dk, dv = (u.transpose(1, 2) for u in kv.cuda().unbind(2))
    rk, rv = (u.transpose(1, 2) for u in kv.repeat_interleave(W, 0).cuda().unbind(2))
    for name, m in (("none", None), ("random", mask)):
        got = decode_attention(q.cuda(), dk, dv, key_mask=None if m is None else m.cuda(), kv_group=W)
        rm = None if m is None else m.repeat_interleave(W, 0)
        want = decode_attention(q.cuda(), rk, rv, key_mask=None if rm is None else rm.cuda())
        assert got.shape == (R, H * hd) and torch.equal(got, want), name
        ref = _ref_attention(q, rk.cpu(), rv.cpu(), rm, n)
        np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-5, err_msg=name)


# ---- the generator ----

def _tiny_model(seed, gen_scale, eos_bias=0.0):
    from csa_amd.model import CSATrans
    m = CSATrans(**TINY)
    fill_params_deterministic(m, seed)
    with torch.no_grad():
        m.generator.linear.weight.mul_(gen_scale)
        m.generator.linear.bias[EOS_ID] += eos_bias
    return m.eval()


def _fixture_model_and_data(z):
    seed, max_len = (int(v) for v in z["meta"])
    m = _tiny_model(seed, 8.0).cuda()
    c = lambda k, dt: torch.from_numpy(z[k]).to(dt).cuda()

    def data():
        """A fresh batch, and the fixture's uniforms armed for the next encode (SBMAttention consumes them)."""
        for i in range(2):
            getattr(m.SBM, f"transformer_{i}").mha.attn.uniforms = torch.from_numpy(z[f"u{i}"]).cuda()
        return SimpleNamespace(src_seq=c("src_seq", torch.int64), tgt_seq=None, L=c("L", torch.uint8),
                               T=c("T", torch.uint8), L_mask=c("L_mask", torch.uint8), T_mask=c("T_mask", torch.uint8))
    return m, data, max_len


def test_beam_of_one_is_greedy_on_the_reference_fixture(golden):
    """W = 1, eos_id None on the reference's GreedyGenerator fixture, whose ys hold neither PAD nor EOS, so masks and
    freezing do not enter: the fixture's ids, CachedGreedyGenerator's ids, and as score the sum of the fixture's
    per-step maxima of step_logp within 1e-4 per step."""
    from csa_amd.model import BeamSearchGenerator, CachedGreedyGenerator
    z = golden("greedy_tiny")
    assert not np.isin(z["ys"], (beam_ref.PAD, EOS_ID)).any()
    m, data, max_len = _fixture_model_and_data(z)
    best, ids, scores = BeamSearchGenerator(m, max_len, 1, eos_id=None)(data(), return_all=True)
    np.testing.assert_array_equal(best.cpu().numpy(), z["ys"])
    assert torch.equal(best, CachedGreedyGenerator(m, max_len)(data()))
    assert torch.equal(ids[:, 0], best) and scores.shape == (best.shape[0], 1)
    steps = z["step_logp"].shape[0]
    want = z["step_logp"].max(-1).astype(np.float64).sum(0)
    print("beam-of-one score error", np.abs(scores[:, 0].cpu().numpy() - want).max())
    np.testing.assert_allclose(scores[:, 0].cpu().numpy(), want, rtol=0, atol=STEP_TOL * steps)


# fill_params_deterministic seed, generator scale and EOS bias of the tiny model, and the seed of its random memory:
# chosen on the CPU oracle alone (seeds 1..15 x three scales), the one run that finishes hypotheses early, reorders
# its beam and beats greedy; its smallest decisive gap is 0.0212 log-probability for W = 3 and W = 4.
TINY_BEAM = dict(seed=6, gen_scale=24.0, eos_bias=2.0)


def _tiny_beam_case():
    m = _tiny_model(**TINY_BEAM)
    g = torch.Generator().manual_seed(TINY_BEAM["seed"])
    enc = torch.randn(3, 20, 64, generator=g)
    src_mask = torch.zeros(3, 20, dtype=torch.bool)
    src_mask[1, 17:] = True
    src_mask[2, 12:] = True
    return m, enc, src_mask


_ORACLE = {}


def _tiny_oracle(W, T=8):
    """The CPU oracle of the tiny case, computed once per W and shared (never modified)."""
    if W not in _ORACLE:
        m, enc, src_mask = _tiny_beam_case()
        _ORACLE[W] = (beam_ref.beam_search_ref(m, enc, src_mask, T, W, EOS_ID), greedy_ids_ref(m, enc, src_mask, T))
    return _ORACLE[W]


@pytest.mark.parametrize("W", [3, 4])
def test_beam_search_matches_the_oracle_on_the_tiny_model(W):
    from csa_amd.model import BeamSearchGenerator
    T = 8
    ref, greedy = _tiny_oracle(W)
    assert_oracle_is_decisive(ref, T - 1)
    assert_run_is_interesting(ref, greedy)
    m, enc, src_mask = _tiny_beam_case()
    best, ids, scores = BeamSearchGenerator(m.cuda(), T, W).search(enc.cuda(), src_mask.cuda(), return_all=True)
    print(f"W={W} min_gap={ref.min_gap:.6f} score error", (scores.cpu() - ref.scores).abs().max().item())
    assert torch.equal(ids.cpu(), ref.ids) and torch.equal(best.cpu(), ref.best)
    np.testing.assert_allclose(scores.cpu().numpy(), ref.scores.numpy(), rtol=0, atol=STEP_TOL * (T - 1))


def test_beam_graph_mode_is_bitwise_eager_and_resets_its_state():
    """graph=True equals eager bitwise in ids and scores, two calls capture once, and a second batch through the same
    graph is right: the stale cum, fin, anc and pad of the first batch are reset."""
    from csa_amd.model import BeamSearchGenerator
    T, W = 8, 4
    m, enc, src_mask = _tiny_beam_case()
    m, enc, src_mask = m.cuda(), enc.cuda(), src_mask.cuda()
    eager = BeamSearchGenerator(m, T, W)
    gen = BeamSearchGenerator(m, T, W, graph=True)
    want = eager.search(enc, src_mask, return_all=True)
    got = gen.search(enc, src_mask, return_all=True)
    again = gen.search(enc, src_mask, return_all=True)
    assert gen.captures == 1 and eager.captures == 0
    ref, _ = _tiny_oracle(W)
    assert torch.equal(want[1].cpu(), ref.ids) and bool(ref.fin.any())  # the first batch leaves finished rows behind
    for a, b, c in zip(want, got, again):
        assert torch.equal(a, b) and torch.equal(a, c)
    enc2 = torch.randn(enc.shape, generator=torch.Generator().manual_seed(77)).cuda()
    mask2 = torch.zeros_like(src_mask)
    mask2[0, 9:] = True
    want2 = eager.search(enc2, mask2, return_all=True)
    got2 = gen.search(enc2, mask2, return_all=True)
    assert gen.captures == 1
    assert not torch.equal(want2[1], want[1])
    for a, b in zip(want2, got2):
        assert torch.equal(a, b)


def test_beam_graph_generator_keeps_at_most_four_graphs():
    """Five (B, S) shapes through one generator: the fifth capture evicts the oldest entry, which is then captured
    again and still gives the eager result."""
    from csa_amd.model import BeamSearchGenerator
    m = beam_ref.stub_model().cuda()
    gen = BeamSearchGenerator(m, 3, 2, graph=True)
    shapes = [(3, 7), (2, 7), (1, 7), (3, 5), (2, 5)]
    g = torch.Generator().manual_seed(11)
    encs = [torch.randn(B, S, 32, generator=g).cuda() for B, S in shapes]
    for enc in encs:
        gen.search(enc)
    assert gen.captures == 5 and len(gen._graphs) == gen.MAX_GRAPHS
    first = gen.search(encs[0], return_all=True)  # evicted as the oldest: captured again
    assert gen.captures == 6 and len(gen._graphs) == gen.MAX_GRAPHS
    want = BeamSearchGenerator(m, 3, 2).search(encs[0], return_all=True)
    for a, b in zip(first, want):
        assert torch.equal(a, b)


def test_beam_graph_without_a_mask_clears_the_static_mask():
    """src_mask=None through a captured entry whose static mask still holds the previous call's padding: bitwise the
    eager result without a mask, which is not the masked one."""
    from csa_amd.model import BeamSearchGenerator
    T, W = 8, 3
    m, enc, src_mask = search_case(device="cuda")
    eager = BeamSearchGenerator(m, T, W)
    gen = BeamSearchGenerator(m, T, W, graph=True)
    masked = gen.search(enc, src_mask, return_all=True)
    got = gen.search(enc, None, return_all=True)
    assert gen.captures == 1 and bool(src_mask.any())
    want = eager.search(enc, None, return_all=True)
    want_masked = eager.search(enc, src_mask, return_all=True)
    assert not torch.equal(want_masked[2], want[2])  # the mask matters: a stale one would show in the scores
    for a, b, c, d in zip(got, want, masked, want_masked):
        assert torch.equal(a, b) and torch.equal(c, d)


# seed / generator scale of the production-dim decoder, chosen on the CPU oracle alone (seeds 1..8 x two scales): the
# run that finishes a hypothesis early, reorders its beam and beats greedy; smallest decisive gap 0.0346
PROD_BEAM = dict(seed=5, gen_scale=4.0, eos_bias=1.0)


def test_beam_search_at_production_head_dim(monkeypatch):
    """hd = 64, S = 150, E = 512, two layers, padded source: search against the oracle, every attention through the
    HIP kernel (counted) and neither it nor the selection through a fallback."""
    from csa_amd import decode_ops
    from csa_amd.model import BeamSearchGenerator
    calls = {"hip": 0, "ref": 0, "topk_ref": 0, "select_ref": 0}

    def count(name, fn):
        def wrapped(*a):
            calls[name] += 1
            return fn(*a)
        return wrapped
    for name, attr in (("hip", "_decode_attention_hip"), ("ref", "_decode_attention_ref"),
                       ("topk_ref", "_beam_row_topk_ref"), ("select_ref", "_beam_select_ref")):
        monkeypatch.setattr(decode_ops, attr, count(name, getattr(decode_ops, attr)))
    T, W, B, S, E = 6, 3, 2, 150, 512
    m, enc, _ = search_case(B=B, S=S, E=E, H=8, V=120, **PROD_BEAM)
    src_mask = torch.zeros(B, S, dtype=torch.bool)
    src_mask[0, 120:] = True
    src_mask[1, 37:] = True
    ref = beam_ref.beam_search_ref(m, enc, src_mask, T, W, EOS_ID)
    assert_oracle_is_decisive(ref, T - 1)
    assert_run_is_interesting(ref, greedy_ids_ref(m, enc, src_mask, T))
    best, ids, scores = BeamSearchGenerator(m.cuda(), T, W).search(enc.cuda(), src_mask.cuda(), return_all=True)
    print(f"min_gap={ref.min_gap:.6f} score error", (scores.cpu() - ref.scores).abs().max().item())
    assert calls == {"hip": 2 * 2 * (T - 1), "ref": 0, "topk_ref": 0, "select_ref": 0}
    assert torch.equal(ids.cpu(), ref.ids) and torch.equal(best.cpu(), ref.best)
    np.testing.assert_allclose(scores.cpu().numpy(), ref.scores.numpy(), rtol=0, atol=STEP_TOL * (T - 1))
