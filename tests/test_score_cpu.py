"""Scoring given summaries, without a GPU: the torch fallback of score_ops.token_logp against the fp64 oracle,
SequenceScorer.score on CPU tensors against the position-by-position loop oracle in both head-mask modes, rerank,
validation_nll on a stub, and the C ABI's declarations and host-side validation (tests/score_ref.py)."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import score_ref
from conftest import ROOT
from score_ref import ATOL, EOS_ID, PAD, RTOL, assert_same_kind_and_close, outside

SYMBOLS = ("csa_token_logp_supported", "csa_token_logp_fwd", "csa_token_logp_bwd")


# ---- the fallback op ----

@pytest.mark.parametrize("V", [1, 2, 3, 61, 1003])
def test_fallback_op_matches_the_oracle_and_its_gradient(V):
    from csa_amd.score_ops import token_logp
    ig = score_ref.kernel_ignore_id(V)
    z, t, g = score_ref.kernel_case(9, V)
    zz = z.clone().requires_grad_()
    out = token_logp(zz, t, ignore_id=ig)
    assert out.dtype == torch.float32 and out.shape == (9,)
    assert_same_kind_and_close(out, score_ref.token_logp_ref(z, t, ig), f"V={V} logp")
    out.backward(g)
    assert_same_kind_and_close(zz.grad, score_ref.token_logp_grad_ref(z, t, g, ig), f"V={V} grad")
    ignored = ~score_ref.scored_rows(t, V, ig)
    assert bool(ignored.any()) and bool((out[ignored] == 0).all()) and bool((zz.grad[ignored] == 0).all())


def test_fallback_op_shapes_dtypes_and_argument_checks():
    from csa_amd.score_ops import token_logp
    z, t, _ = score_ref.kernel_case(12, 17, kinds=("plain", "ignored"))
    want = score_ref.token_logp_ref(z, t)
    assert torch.equal(token_logp(z.view(3, 4, 17), t.view(3, 4)), token_logp(z, t).view(3, 4))
    wide = torch.zeros(12, 40)
    wide[:, 3:20] = z
    assert torch.equal(token_logp(wide[:, 3:20], t), token_logp(z, t))  # a strided view
    np.testing.assert_allclose(token_logp(z.double(), t).numpy(), want.numpy(), rtol=1e-12, atol=1e-12)
    assert token_logp(z.to(torch.bfloat16), t).dtype == torch.float32
    assert token_logp(torch.zeros(4, 0), torch.zeros(4, dtype=torch.int64)).tolist() == [0.0] * 4  # V = 0: all ignored
    assert token_logp(torch.zeros(0, 5), torch.zeros(0, dtype=torch.int64)).shape == (0,)
    with pytest.raises(ValueError):
        token_logp(z, t.int())
    with pytest.raises(ValueError):
        token_logp(z, t[:-1])


def test_fallback_does_not_underflow_where_log_of_softmax_does():
    """The Generator's log(softmax(z)) gives -inf once the probability underflows fp32; the scorer's log-softmax keeps
    the finite value."""
    from csa_amd.score_ops import token_logp
    z = torch.tensor([[0.0, -200.0, 3.0]])
    t = torch.tensor([1])
    assert torch.log(torch.softmax(z, -1))[0, 1] == float("-inf")
    np.testing.assert_allclose(token_logp(z, t).item(), score_ref.token_logp_ref(z, t).item(), rtol=RTOL)


# ---- the scorer against the loop oracle ----

_CASE = {}


def _case():
    """Model, inputs and the loop oracle in both modes, computed once and never modified."""
    if not _CASE:
        m = score_ref.decoder_stub()
        enc, src_mask, cand = score_ref.scorer_case()
        _CASE.update(m=m, enc=enc, src_mask=src_mask, cand=cand,
                     own=score_ref.score_loop_ref(m, enc, src_mask, cand, EOS_ID, "own"),
                     reference=score_ref.score_loop_ref(m, enc, src_mask, cand, EOS_ID, "reference"))
    return SimpleNamespace(**_CASE)


@pytest.mark.parametrize("mode", ["own", "reference"])
def test_scorer_on_cpu_matches_the_loop_oracle(mode):
    from csa_amd.model import SequenceScorer
    c = _case()
    B, G, T = c.cand.shape
    tokens, logp, length = getattr(c, mode)
    with torch.no_grad():
        out = SequenceScorer(c.m, eos_id=EOS_ID, head_mask=mode).score(c.enc, c.src_mask, c.cand, return_tokens=True)
    assert out.logp.shape == (B, G) and out.logp.dtype == torch.float32
    assert out.length.shape == (B, G) and out.length.dtype == torch.int32 and out.tokens.shape == (B, G, T)
    np.testing.assert_allclose(out.tokens.reshape(B * G, T).numpy(), tokens.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out.logp.reshape(-1).numpy(), logp.numpy(), rtol=RTOL, atol=ATOL)
    assert out.length.reshape(-1).tolist() == length.tolist() == [2, 7, 4, 7, 5, 3]
    assert torch.equal(out.logp, out.tokens.sum(-1))  # the plain sum of the per-token vector
    unscored = ~score_ref.scored_positions(c.cand.view(B * G, T), EOS_ID)
    assert bool((out.tokens.reshape(B * G, T)[unscored] == 0).all())
    # (B, T') input: G is squeezed away and the numbers are those of G = 1
    with torch.no_grad():
        flat = SequenceScorer(c.m, eos_id=EOS_ID, head_mask=mode).score(c.enc, c.src_mask, c.cand[:, 0])
    assert flat.logp.shape == (B,) and flat.length.shape == (B,) and flat.tokens is None
    if mode == "own":  # a row's score does not depend on its neighbours in the batch
        np.testing.assert_allclose(flat.logp.numpy(), out.logp[:, 0].numpy(), rtol=RTOL, atol=ATOL)


def test_scorer_fixture_is_decisive():
    """Each wrong reading of the definition leaves the tolerance on these inputs."""
    from csa_amd.model import SequenceScorer
    c = _case()
    B, G, T = c.cand.shape
    cand = c.cand.view(B * G, T)
    scored = score_ref.scored_positions(cand, EOS_ID)
    s = SequenceScorer(c.m, eos_id=EOS_ID, head_mask="own")
    bos = torch.full((B * G, 1), score_ref.BOS, dtype=torch.int64)
    dec_in = torch.cat([bos, cand[:, :-1]], 1)
    want = c.own[0]
    with torch.no_grad():
        right = s.token_logps(c.enc, c.src_mask, dec_in, cand, scored, G)
        shifted = s.token_logps(c.enc, c.src_mask, dec_in, torch.roll(cand, -1, 1), scored, G)
        no_bos = s.token_logps(c.enc, c.src_mask, cand, cand, scored, G)
        past_eos = SequenceScorer(c.m, eos_id=None).score(c.enc, c.src_mask, c.cand, return_tokens=True)
        other = SequenceScorer(c.m, eos_id=EOS_ID, head_mask="reference").score(c.enc, c.src_mask, c.cand,
                                                                                 return_tokens=True)
    assert not outside(right, want)
    assert outside(shifted, want), "a target shifted by one goes unnoticed"
    assert outside(no_bos, want), "a missing BOS shift goes unnoticed"
    assert outside(past_eos.tokens.view(B * G, T), want) and outside(past_eos.logp.view(-1), c.own[1]), \
        "scoring past the first EOS goes unnoticed"
    assert past_eos.length.view(-1)[4] == 7 and past_eos.length.view(-1)[1] == 6  # ids after EOS; a PAD before it
    assert outside(other.tokens.view(B * G, T), want), "the head-mask modes do not differ on this batch"
    assert outside(c.reference[0], c.own[0])


def test_scorer_is_differentiable_on_cpu():
    from csa_amd.model import SequenceScorer
    c = _case()
    enc = c.enc.clone().requires_grad_()
    out = SequenceScorer(c.m, eos_id=EOS_ID).score(enc, c.src_mask, c.cand)
    out.logp.sum().backward()
    try:
        assert enc.grad is not None and bool(torch.isfinite(enc.grad).all()) and float(enc.grad.abs().max()) > 0
        for p in (c.m.generator.linear.weight, c.m.decoder.layers[0].self_attn.in_proj_weight):
            assert p.grad is not None and float(p.grad.abs().max()) > 0
    finally:
        c.m.zero_grad(set_to_none=True)


def test_scorer_argument_checks():
    from csa_amd.model import SequenceScorer
    c = _case()
    with pytest.raises(ValueError):
        SequenceScorer(c.m, head_mask="mine")
    with pytest.raises(ValueError):
        SequenceScorer(c.m, eos_id=-1)
    with pytest.raises(ValueError):
        SequenceScorer(c.m).score(c.enc, c.src_mask, c.cand.int())
    with pytest.raises(ValueError):
        SequenceScorer(c.m).score(c.enc, c.src_mask, c.cand[:2])


# ---- rerank and validation_nll ----

def test_rerank_orders_by_score_and_breaks_ties_by_index():
    from csa_amd.model import rerank
    ids = torch.arange(2 * 4 * 3).view(2, 4, 3)
    out = SimpleNamespace(logp=torch.tensor([[-3.0, -1.0, -1.0, -2.0], [-4.0, -4.0, -6.0, -0.5]]),
                          length=torch.tensor([[3, 1, 1, 2], [1, 2, 3, 1]], dtype=torch.int32))
    best, order = rerank(ids, out)
    assert order.tolist() == [[1, 2, 3, 0], [3, 0, 1, 2]]
    assert torch.equal(best, torch.stack([ids[0, 1], ids[1, 3]]))
    best, order = rerank(ids, out, length_penalty=1.0)  # -1, -1, -1, -1 | -4, -2, -2, -0.5
    assert order.tolist() == [[0, 1, 2, 3], [3, 1, 2, 0]]
    assert torch.equal(best, torch.stack([ids[0, 0], ids[1, 3]]))
    out.length[0, 0] = 0  # an empty candidate is ranked on its sum
    assert rerank(ids, out, length_penalty=1.0)[1][0].tolist() == [1, 2, 3, 0]
    with pytest.raises(ValueError):
        rerank(ids[:, 0], out)


def test_validation_nll_pools_tokens_over_batches():
    """On a stub whose encoder is the identity: the pooled NLL of two batches is the oracle's token-weighted mean."""
    from csa_amd.model import validation_nll
    c = _case()

    class WithEncoder(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.tgt_embedding, self.decoder, self.generator = m.tgt_embedding, m.decoder, m.generator

        def process_data(self, data):
            pass

        def encode(self, data):
            return (data.enc,)

    B, G, T = c.cand.shape
    batches, tot, n = [], 0.0, 0
    for k in range(G):
        target = c.cand[:, k].clone()
        target[target == EOS_ID] = 5  # no EOS rule here: every non-PAD target counts
        tgt_seq = torch.cat([torch.full((B, 1), score_ref.BOS), target[:, :-1]], 1)
        batches.append((SimpleNamespace(enc=c.enc, src_mask=c.src_mask, tgt_seq=tgt_seq), target))
        _, logp, length = score_ref.score_loop_ref(c.m, c.enc, c.src_mask, target, None, "reference")
        tot, n = tot + float(logp.sum()), n + int(length.sum())
    out = validation_nll(WithEncoder(c.m), batches)
    assert out.tokens == n and isinstance(out.nll, float)
    np.testing.assert_allclose(out.nll, -tot / n, rtol=1e-5)
    np.testing.assert_allclose(out.ppl, math.exp(-tot / n), rtol=1e-4)
    assert validation_nll(WithEncoder(c.m), []).tokens == 0


# ---- the C ABI ----

def test_new_symbols_are_declared_exported_and_listed():
    from csa_amd import _lib
    src = open(os.path.join(ROOT, "include", "csa_hip.h")).read()
    L = _lib.lib()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", src), s
        assert hasattr(L, s), s
        assert s in _lib.EXPORTED_SYMBOLS, s
    from csa_amd import model
    for name in ("SequenceScorer", "rerank", "validation_nll"):
        assert callable(getattr(model, name))
    from csa_amd.build import SOURCES
    assert "csa_score.hip" in SOURCES


def test_entry_points_validate_without_a_gpu():
    from csa_amd import _lib
    L = _lib.lib()
    assert L.csa_token_logp_supported(1) == 1 and L.csa_token_logp_supported(50021) == 1
    assert L.csa_token_logp_supported(1 << 24) == 1 and L.csa_token_logp_supported((1 << 24) + 1) == 0
    assert L.csa_token_logp_supported(0) == 0 and L.csa_token_logp_supported(-1) == 0
    assert L.csa_token_logp_fwd(None, 8, None, 2, 8, 0, None, None, None) == 1
    assert b"null pointer" in L.csa_last_error_str()
    assert L.csa_token_logp_bwd(None, None, 8, None, None, None, 8, 2, 8, 0, None) == 1
    assert b"null pointer" in L.csa_last_error_str()
    buf = (ctypes.c_float * 64)()
    tgt = (ctypes.c_int64 * 4)()
    p, t = ctypes.addressof(buf), ctypes.addressof(tgt)
    assert L.csa_token_logp_fwd(p, 4, t, 2, 8, 0, p, p, None) == 1   # ld < V
    assert L.csa_token_logp_fwd(p, 8, t, -1, 8, 0, p, p, None) == 1
    assert L.csa_token_logp_bwd(p, p, 8, t, p, p, 12, 2, 8, 0, None) == 1  # in place with another stride
    assert b"in place" in L.csa_last_error_str()
    assert L.csa_token_logp_fwd(p, (1 << 24) + 1, t, 1, (1 << 24) + 1, 0, p, p, None) == 2  # CSA_UNSUPPORTED_SHAPE
    # nothing to do: CSA_OK before any pointer is looked at, no launch
    assert L.csa_token_logp_fwd(None, 8, None, 0, 8, 0, None, None, None) == 0
    assert L.csa_token_logp_fwd(None, 0, None, 3, 0, 0, None, None, None) == 0
    assert L.csa_token_logp_bwd(None, None, 8, None, None, None, 8, 0, 8, 0, None) == 0


def test_score_ops_calls_the_library_on_the_tensors_device():
    """As tests/test_abi_cpu.py demands of the other ctypes-bound ops files: every library call sits in on_device."""
    path = os.path.join(ROOT, "code-structure-aware-transformer_amd", "csa_amd", "score_ops.py")
    lines = open(path).read().split("\n")
    calls = [i for i, ln in enumerate(lines) if re.match(r"\s*check\((L|lib\(\))\.csa_", ln)]
    assert len(calls) == 2
    for i in calls:
        assert "with on_device(" in lines[i - 1], f"score_ops.py:{i + 1} library call outside on_device"
