"""The full-sequence decoder attention without a GPU (tests/seq_attn_ref.py): the torch fallback of
seq_attn_ops.seq_attention against the fp64 oracle, forward and gradients; wrong variants of the rule leave the bound on
the chosen cases, and so does an operand read with its neighbour's strides; build() is bit for bit stable for the old
cases; the wide-logit and one-visible-key cases are what the GPU tests take them for; SequenceScorer(attention="fused") on CPU tensors against the loop oracle and against "sdpa", values and
gradients; which path a call reports; argument checks; the C ABI's host-side validation."""
import ctypes
import hashlib

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
    ("group4_own_hd8", "group_mod", ("out", "dq", "dk", "dv")),
    ("group4_own_hd8", "other_mode", ("out", "dq", "dk", "dv")),
    ("group4_own_hd64", "one_member", ("dk", "dv")),
    ("group4_reference_hd8", "group_mod", ("out", "dq", "dk", "dv")),
    ("group4_reference_hd8", "other_mode", ("out", "dq", "dk", "dv")),
    ("group4_reference_hd64", "other_mode", ("out", "dq", "dk", "dv")),
    ("group2_reference_hd8", "group_mod", ("out", "dq", "dk", "dv")),
    ("group2_reference_hd8", "other_mode", ("out", "dq", "dk", "dv")),
    ("group2_reference_hd64", "other_mode", ("out", "dq", "dk", "dv")),
    ("heads3_hd8", "other_mode", ("out", "dq", "dk", "dv")),
    ("mask_prefix_hd8", "mask_row0", ("out", "dq", "dk", "dv")),
    ("mask_prefix_hd64", "mask_row0", ("out", "dq", "dk", "dv")),
    ("mask_alternate_hd8", "mask_row0", ("out", "dq", "dk", "dv")),
    ("long_causal_reference_hd64_T256", "other_mode", ("out", "dq", "dk", "dv")),
])
def test_wrong_variants_leave_the_bound(name, wrong, tensors):
    """A fixture is decisive when an answer computed by a plausible wrong rule lies outside the case's bound."""
    c = ref.CASES[name]
    inputs = ref.build(c)
    good, bad = ref.oracle(c, *inputs), ref.oracle(c, *inputs, wrong=wrong)
    for tname, x, x64, base in zip(("out", "dq", "dk", "dv"), bad, good, ref.BASELINE[name]):
        if tname in tensors:
            assert ref.rel_err(x, x64) > 1000 * ref.FACTOR * base, (name, wrong, tname)


@pytest.mark.parametrize("name", ["layout_cross_hd8", "layout_causal_hd64"])
@pytest.mark.parametrize("which", ["k", "v", "q"])
def test_reading_one_operand_with_anothers_strides_leaves_the_bound(name, which):
    """The mixed-layout GPU tests are decisive: with one operand stored as (N, L, H, hd) and read with the contiguous
    (N, H, L, hd) strides of its neighbour, as a kernel that took k's strides for v would, every tensor leaves the bound
    (dv = P^T dO does not depend on V's values: it is exempt when V is the misread one)."""
    c = ref.CASES[name]
    inputs = ref.build(c)
    i = "qkv".index(which)
    stored = inputs[i].transpose(1, 2).contiguous().transpose(1, 2)  # the same values, the other layout
    assert torch.equal(stored, inputs[i])
    misread = stored.as_strided(stored.shape, inputs[i].stride())
    bad = ref.oracle(c, *(misread if j == i else t for j, t in enumerate(inputs)))
    for tname, x, x64, base in zip(("out", "dq", "dk", "dv"), bad, ref.oracle(c, *inputs), ref.BASELINE[name]):
        if (which, tname) != ("v", "dv"):
            assert ref.rel_err(x, x64) > 1000 * ref.FACTOR * base, (name, which, tname)


def test_build_is_unchanged_for_the_old_cases():
    """The keys build() gained default to off: the old cases' tensors are bit for bit what they were (sha256 over
    q, k, v, mask, dout, taken before the keys existed), and their BASELINE rows are the old ones."""
    want = {"group_hd8_G2": "60aea848df2961e94820fc410a5e3ebce349609acfca0f9df97769675b8784c5",
            "packed_self_hd64": "f0d178a8c9d4b8a6a3abeb8a94efe3097e114e38565b3dc5ca15de8792e0237b",
            "causal_reference_hd8_T17": "3b2b66ccce88ac6e17700db57aa02f5b8c00d4dfc46d277ce46aeda6c51f7293",
            "packed_cross_hd8": "a35e8a7ee0cfc4bacb92f1ebc8f5643b95cf7c0ddf2aa51e4a5eb1a0a0145abb"}
    for name, digest in want.items():
        h = hashlib.sha256()
        for t in ref.build(ref.CASES[name]):
            h.update(t.contiguous().numpy().tobytes())
        assert h.hexdigest() == digest, name
    assert len(ref.OLD_CASES) == 38 and list(ref.CASES)[:38] == [c["name"] for c in ref.OLD_CASES]
    assert all(c["qscale"] is None and c["key_order"] is None and c["dout"] is None for c in ref.OLD_CASES)
    assert set(ref.BASELINE) == set(ref.CASES)
    assert ref.BASELINE["cross_hd8_T1_S17"] == (1.941e-07, 1.772e-07, 7.696e-08, 1.890e-07)
    assert ref.BASELINE["packed_cross_hd64"] == (4.917e-07, 5.454e-07, 5.951e-07, 4.400e-07)


@pytest.mark.parametrize("name", [n for n, c in ref.CASES.items() if c["qscale"] is not None])
def test_wide_logit_cases_are_wide_ordered_and_finite(name):
    c = ref.CASES[name]
    q, k, v, mask, dout = inputs = ref.build(c)
    s = (q.double() @ k.double().transpose(-1, -2)) * float(c["hd"]) ** -0.5
    assert 6.0 < s.std().item() < 10.0  # scale * s: a standard deviation of about 8
    step = s[:, :, 0, 1:] - s[:, :, 0, :-1]  # query 0 against the sorted keys
    assert bool((step >= 0).all() if c["key_order"] == "ascending" else (step <= 0).all())
    gap = (s[:, :, 0, -1] - s[:, :, 0, 0]).abs()  # first to last key: exp(-gap) lies below fp32's resolution
    assert gap.min().item() > -np.log(ref.EPS32), gap
    assert not bool(ref.mask_entries(c, mask).all(-1).any())  # no query row is fully masked
    for x in ref.oracle(c, *inputs):
        assert bool(torch.isfinite(x).all()), name
    for n, e in ref.lse_bound(c, *inputs).items():
        assert 0.0 < e < 1e-4, (name, n, e)


@pytest.mark.parametrize("name", ["mask_last_only_hd8", "mask_last_only_hd64"])
def test_one_visible_last_key_gives_that_v_row_and_zero_dq_dk(name):
    """What the GPU test relies on: in fp64 out is exactly the last V row for every query, dq and dk are identically
    zero (the zero_bound branch of check()), dv is non-zero in that row only."""
    c = ref.CASES[name]
    q, k, v, mask, dout = inputs = ref.build(c)
    out, dq, dk, dv = ref.oracle(c, *inputs)
    want = v[:, :, c["S"] - 1].double().reshape(c["R"], 1, -1).expand(-1, c["T"], -1)
    assert torch.equal(out, want)
    assert not bool(dq.any()) and not bool(dk.any())
    assert bool(dv[:, :, c["S"] - 1].any()) and not bool(dv[:, :, :c["S"] - 1].any())
    assert ref.BASELINE[name][1] is None and ref.BASELINE[name][2] is None and ref.BASELINE[name][0] == 0.0
    assert ref.zero_bound(c, q, k, v, dout) > 0.0


def test_new_mask_kinds_are_what_their_names_say():
    for name, rows in (("mask_prefix_hd8", {0: range(32), 1: range(16)}), ("mask_alternate_hd8", {0: range(0, 33, 2), 1: range(1, 33, 2)}),
                       ("mask_last_only_hd8", {0: range(32), 1: range(32)})):
        mask = ref.build(ref.CASES[name])[3]
        for b, dead in rows.items():
            assert mask[b].nonzero().flatten().tolist() == list(dead), (name, b)
    for name in ("group4_reference_hd8", "group2_reference_hd64"):  # (R, S), the rows all different
        c = ref.CASES[name]
        mask = ref.build(c)[3]
        assert mask.shape == (c["R"], c["S"]) and len({tuple(r.tolist()) for r in mask}) == c["R"]


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
                                 (dict(mask=p, mask_ld=5, S=6, causal=0), 1, b"mask_ld"),
                                 (dict(k_sn=10), 1, b"multiples of 4"),
                                 (dict(v_sh=42), 1, b"multiples of 4"),
                                 (dict(q_sr=-80), 1, b"multiples of 4"),
                                 (dict(q=ctypes.c_void_p(p.value + 4)), 1, b"16-byte aligned"),
                                 (dict(v=ctypes.c_void_p(p.value + 8)), 1, b"16-byte aligned"),
                                 (dict(R=6, kv_group=4), 1, b"kv_group must divide R"),
                                 (dict(out=None), 1, b"null pointer"),
                                 (dict(R=1 << 30, H=1 << 10), 2, b"grid limit")):
        a = _lib.SeqAttnArgs(**{**ok, **change})
        assert L.csa_seq_attn_fwd(ctypes.byref(a), None) == status, change
        assert text in L.csa_last_error_str(), (change, L.csa_last_error_str())
    a = _lib.SeqAttnArgs(**ok)
    b = _lib.SeqAttnBwdArgs(fwd=ctypes.pointer(a), dout=p, dq=p, dk=p, dv=p)  # no workspace
    assert L.csa_seq_attn_bwd(ctypes.byref(b), None) == 1 and b"null pointer" in L.csa_last_error_str()
    for change, text in ((dict(dq=ctypes.c_void_p(p.value + 4)), b"16-byte aligned"), (dict(dv_sn=6), b"multiples of 4"),
                         (dict(dk_sh=-40), b"multiples of 4")):
        b = _lib.SeqAttnBwdArgs(**{**dict(fwd=ctypes.pointer(a), dout=p, dq=p, dk=p, dv=p, workspace=p, dq_sr=80, dq_sh=40,
                                          dq_st=8, dk_sb=80, dk_sh=40, dk_sn=8, dv_sb=80, dv_sh=40, dv_sn=8), **change})
        assert L.csa_seq_attn_bwd(ctypes.byref(b), None) == 1 and text in L.csa_last_error_str(), change
