"""The full-sequence decoder attention without a GPU (tests/seq_attn_ref.py): the torch fallback of
seq_attn_ops.seq_attention against the fp64 oracle, forward and gradients; wrong variants of the rule leave the bound on
the chosen cases; SequenceScorer(attention="fused") on CPU tensors against the loop oracle and against "sdpa", values and
gradients; which path a call reports; argument checks; the C ABI's host-side validation."""
import ctypes

import numpy as np
import pytest
import torch

import score_ref
import seq_attn_ref as ref
from score_ref import ATOL, EOS_ID, RTOL


def _run(c, inputs):
    from csa_amd.seq_attn_ops import seq_attention
    q, k, v, mask, dout = inputs
    qq, kk, vv = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = seq_attention(qq, kk, vv, mask, causal=c["causal"], mask_mode=c["mode"], kv_group=c["G"])
    assert out.shape == (c["R"], c["T"], c["H"] * c["hd"]) and out.dtype == torch.float32
    return (out.detach(),) + torch.autograd.grad(out, (qq, kk, vv), dout)


@pytest.mark.parametrize("name", ref.CPU_CASES)
def test_fallback_matches_the_oracle_forward_and_gradients(name):
    c = ref.CASES[name]
    inputs = ref.build(c)
    ref.check(c, _run(c, inputs), inputs, what="fallback ")


@pytest.mark.parametrize("name, wrong, tensors", [
    ("group_hd8_G2", "group_mod", ("out", "dq", "dk", "dv")),
    ("causal_own_hd8_T17", "no_causal", ("out", "dq", "dk", "dv")),
    ("causal_own_hd8_T17", "other_mode", ("out", "dq", "dk", "dv")),
    ("causal_reference_hd8_T17", "other_mode", ("out", "dq", "dk", "dv")),
    ("group_hd8_G3", "one_member", ("dk", "dv")),
])
def test_wrong_variants_leave_the_bound(name, wrong, tensors):
    """A fixture is decisive when an answer computed by a plausible wrong rule lies outside the case's bound."""
    c = ref.CASES[name]
    inputs = ref.build(c)
    good, bad = ref.oracle(c, *inputs), ref.oracle(c, *inputs, wrong=wrong)
    for tname, x, x64, base in zip(("out", "dq", "dk", "dv"), bad, good, ref.BASELINE[name]):
        if tname in tensors:
            assert ref.rel_err(x, x64) > 1000 * ref.FACTOR * base, (name, wrong, tname)


def test_scorer_case_separates_the_two_mask_modes():
    own, reference = (score_ref.score_loop_ref(score_ref.decoder_stub(layers=1), *score_ref.scorer_case(), EOS_ID, hm)[0]
                      for hm in ("own", "reference"))
    assert score_ref.outside(own, reference)


# ---- the scorer ----

_CASE = {}


def _case():
    """Model, inputs and the loop oracle in both modes, computed once and never modified."""
    if not _CASE:
        m = score_ref.decoder_stub()
        enc, src_mask, cand = score_ref.scorer_case()
        _CASE.update(m=m, enc=enc, src_mask=src_mask, cand=cand,
                     own=score_ref.score_loop_ref(m, enc, src_mask, cand, EOS_ID, "own"),
                     reference=score_ref.score_loop_ref(m, enc, src_mask, cand, EOS_ID, "reference"))
    return _CASE


@pytest.mark.parametrize("head_mask", ["own", "reference"])
def test_fused_scorer_matches_the_loop_oracle_and_sdpa(head_mask):
    from csa_amd.model import SequenceScorer
    c = _case()
    tokens, logp, length = c[head_mask]
    other = c["reference" if head_mask == "own" else "own"][0]
    scorer = SequenceScorer(c["m"], EOS_ID, head_mask, attention="fused")
    with torch.no_grad():
        out = scorer.score(c["enc"], c["src_mask"], c["cand"], return_tokens=True)
        sdpa = SequenceScorer(c["m"], EOS_ID, head_mask).score(c["enc"], c["src_mask"], c["cand"], return_tokens=True)
    assert scorer.last_attention == "fused"
    got = out.tokens.view(6, -1)
    print("fused vs fp64", (got.double() - tokens).abs().max().item(),
          "fused vs sdpa", (out.tokens - sdpa.tokens).abs().max().item())
    np.testing.assert_allclose(got.numpy(), tokens.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out.logp.view(-1).numpy(), logp.numpy(), rtol=RTOL, atol=ATOL)
    assert out.length.view(-1).tolist() == length.tolist()
    np.testing.assert_allclose(out.tokens.numpy(), sdpa.tokens.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out.logp.numpy(), sdpa.logp.numpy(), rtol=RTOL, atol=ATOL)
    assert score_ref.outside(got, other)  # the other mode's numbers would not pass
    # (B, T') candidates: kv_group = 1
    with torch.no_grad():
        one = scorer.score(c["enc"], c["src_mask"], c["cand"][:, 0])
    if head_mask == "own":  # a row's score does not depend on its neighbours
        np.testing.assert_allclose(one.logp.numpy(), logp.view(3, 2)[:, 0].numpy(), rtol=RTOL, atol=ATOL)


def test_fused_scorer_gradients_match_sdpa():
    from csa_amd.model import SequenceScorer
    c = _case()
    m = c["m"]
    w_dec = m.decoder.layers[1].multihead_attn.in_proj_weight

    def grads(attention):
        m.zero_grad(set_to_none=True)
        e = c["enc"].clone().requires_grad_()
        SequenceScorer(m, EOS_ID, "own", attention=attention).score(e, c["src_mask"], c["cand"]).logp.sum().backward()
        return [g.detach().clone() for g in (m.generator.linear.weight.grad, w_dec.grad,
                                             m.decoder.layers[0].self_attn.in_proj_weight.grad, e.grad)]
    try:
        got, want = grads("fused"), grads("sdpa")
    finally:
        m.zero_grad(set_to_none=True)
    for name, a, b in zip(("generator", "cross in_proj", "self in_proj", "enc"), got, want):
        scale = b.abs().max().item()
        print(name, "max|fused - sdpa| / max|sdpa|", (a - b).abs().max().item() / scale)
        assert scale > 0
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-3, atol=1e-5 * scale, err_msg=name)


def test_last_attention_reports_the_path_taken():
    from csa_amd.model import SequenceScorer, validation_nll
    c = _case()
    m = score_ref.decoder_stub(layers=1)
    scorer = SequenceScorer(m, EOS_ID, attention="fused")
    assert scorer.last_attention is None
    with torch.no_grad():
        scorer.score(c["enc"], c["src_mask"], c["cand"])
        assert scorer.last_attention == "fused"
        m.train()  # dropout 0.2 > 0: the kernel has no attention dropout
        scorer.score(c["enc"], c["src_mask"], c["cand"])
        assert scorer.last_attention == "sdpa"
        for mod in m.decoder.layers:
            mod.self_attn.dropout = mod.multihead_attn.dropout = 0.0
        scorer.score(c["enc"], c["src_mask"], c["cand"])
        assert scorer.last_attention == "fused"
    plain = SequenceScorer(m.eval(), EOS_ID)
    with torch.no_grad():
        plain.score(c["enc"], c["src_mask"], c["cand"])
    assert plain.last_attention == "sdpa"
    with pytest.raises(ValueError):
        SequenceScorer(m, EOS_ID, attention="flash")
    # validation_nll takes the keyword and gives the same number
    data = type("D", (), {})()
    data.tgt_seq = torch.cat([torch.full((3, 1), score_ref.BOS), c["cand"][:, 0, :-1]], 1)
    data.src_mask = c["src_mask"]
    m.process_data, m.encode = (lambda d: None), (lambda d: (c["enc"],))
    a = validation_nll(m, [(data, c["cand"][:, 0])], attention="fused")
    b = validation_nll(m, [(data, c["cand"][:, 0])])
    assert a.tokens == b.tokens and abs(a.nll - b.nll) <= 1e-5 * abs(b.nll)


def test_bad_arguments_raise():
    from csa_amd import model
    from csa_amd.seq_attn_ops import seq_attention
    assert model.seq_attention is seq_attention and model.ATTENTIONS == ("sdpa", "fused")
    q, k = torch.randn(6, 2, 5, 8), torch.randn(6, 2, 7, 8)
    with pytest.raises(ValueError):
        seq_attention(q, k, k, causal=True)  # S != T
    with pytest.raises(ValueError):
        seq_attention(q, k[:3, :, :5], k[:3, :, :5], causal=True, kv_group=2)  # causal with a group
    with pytest.raises(ValueError):
        seq_attention(q, k[:4], k[:4], kv_group=4)  # R not divisible by kv_group
    with pytest.raises(ValueError):
        seq_attention(q, k[:2], k[:2], kv_group=2)  # k holds the wrong number of rows
    with pytest.raises(ValueError):
        seq_attention(q, k, k, key_mask=torch.zeros(6, 6, dtype=torch.uint8))  # fewer than S columns
    with pytest.raises(ValueError):
        seq_attention(q, k, k, key_mask=torch.zeros(6, 7))  # not bytes
    with pytest.raises(ValueError):
        seq_attention(q, k, k, mask_mode="heads")
    assert seq_attention(q, k[:3], k[:3], key_mask=torch.zeros(3, 9, dtype=torch.bool), kv_group=2).shape == (6, 5, 16)


def test_abi_validates_on_the_host():
    """The entry points reject bad arguments before any HIP call, and report the supported shapes."""
    from csa_amd import _lib
    L = _lib.lib()
    assert L.csa_seq_attn_supported(64, 49, 150) and L.csa_seq_attn_supported(8, 1, 1) and L.csa_seq_attn_supported(64, 256, 9)
    assert not L.csa_seq_attn_supported(64, 257, 9) and not L.csa_seq_attn_supported(32, 8, 8)
    assert not L.csa_seq_attn_supported(64, 0, 8) and not L.csa_seq_attn_supported(64, 8, 0)
    assert L.csa_seq_attn_bwd_workspace_bytes(6, 8, 7) == 6 * 8 * 7 * 4
    assert L.csa_seq_attn_fwd(None, None) == 1 and L.csa_seq_attn_bwd(None, None) == 1
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(R=4, H=2, T=5, S=5, hd=8, kv_group=1, q=p, q_sr=80, q_sh=40, q_st=8, k=p, k_sb=80, k_sh=40, k_sn=8,
              v=p, v_sb=80, v_sh=40, v_sn=8, scale=1.0, out=p, lse=p)
    for change, status, text in ((dict(kv_group=3), 1, b"kv_group must divide R"),
                                 (dict(causal=1, kv_group=2), 1, b"causal needs"),
                                 (dict(causal=1, S=6), 1, b"causal needs"),
                                 (dict(hd=32), 2, b"hd in"),
                                 (dict(T=300), 2, b"T <= 256"),
                                 (dict(q_st=6), 1, b"multiples of 4"),
                                 (dict(mask=p, mask_ld=4), 1, b"mask_ld"),
                                 (dict(mask_mode=2), 1, b"mask_mode"),
                                 (dict(out=None), 1, b"null pointer"),
                                 (dict(R=1 << 30, H=1 << 10), 2, b"grid limit")):
        a = _lib.SeqAttnArgs(**{**ok, **change})
        assert L.csa_seq_attn_fwd(ctypes.byref(a), None) == status, change
        assert text in L.csa_last_error_str(), (change, L.csa_last_error_str())
    a = _lib.SeqAttnArgs(**ok)
    b = _lib.SeqAttnBwdArgs(fwd=ctypes.pointer(a), dout=p, dq=p, dk=p, dv=p)  # no workspace
    assert L.csa_seq_attn_bwd(ctypes.byref(b), None) == 1 and b"null pointer" in L.csa_last_error_str()
