"""The full-sequence decoder attention on the GPU (csrc/csa_seqattn.hip through seq_attn_ops.seq_attention): every case
of tests/seq_attn_ref.py against the fp64 oracle within four times the parent's error, forward and the three gradients;
packed operands and packed gradients; exact zeros at masked keys; bitwise determinism; a fully masked query row;
SequenceScorer(attention="fused") on the tiny model against the loop oracle, "sdpa" and the beam's scores; peak memory."""
import functools

import numpy as np
import pytest
import torch

import score_ref
import seq_attn_ref as ref
from conftest import has_gpu
from golden_inputs import fill_params_deterministic
from score_ref import ATOL, EOS_ID, RTOL, TINY

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]


def _to_gpu(c, inputs):
    """The case's tensors on the GPU with the same layout: packed views stay views of one packed buffer."""
    q, k, v, mask, dout = inputs
    if c["packed"] and c["causal"]:
        buf = torch.stack([t.transpose(1, 2) for t in (q, k, v)], 2).cuda()
        q, k, v = (buf[:, :, i].transpose(1, 2) for i in range(3))
    elif c["packed"]:
        q = q.transpose(1, 2).contiguous().cuda().transpose(1, 2)
        buf = torch.stack([t.transpose(1, 2) for t in (k, v)], 2).cuda()
        k, v = (buf[:, :, i].transpose(1, 2) for i in range(2))
    else:
        q, k, v = q.cuda(), k.cuda(), v.cuda()
    return q, k, v, None if mask is None else mask.cuda(), dout.cuda()


def _run(c, gpu):
    from csa_amd.seq_attn_ops import seq_attention
    q, k, v, mask, dout = gpu
    qq, kk, vv = (t.detach().requires_grad_() for t in (q, k, v))  # the same memory, strides kept
    out = seq_attention(qq, kk, vv, mask, causal=c["causal"], mask_mode=c["mode"], kv_group=c["G"])
    assert out.shape == (c["R"], c["T"], c["H"] * c["hd"]) and out.is_contiguous()
    return (out.detach(),) + torch.autograd.grad(out, (qq, kk, vv), dout)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_kernels_match_the_oracle_forward_and_gradients(name):
    from csa_amd._lib import lib
    from csa_amd.ops import packed_qkv
    from csa_amd.seq_attn_ops import _packed_kv
    c = ref.CASES[name]
    assert lib().csa_seq_attn_supported(c["hd"], c["T"], c["S"])
    inputs = ref.build(c)
    got = _run(c, _to_gpu(c, inputs))
    ref.check(c, got, inputs)
    out, dq, dk, dv = got
    mask = inputs[3]
    if mask is not None and c["mode"] == "own":  # a key masked for every query that reads it: exact zeros
        dead = (mask[:, :c["S"]] != 0).cuda()
        assert bool(dead.any()) or c["T"] == 1  # one position: BOS, never PAD
        for g in (dk, dv):
            assert bool((g.transpose(1, 2)[dead] == 0).all()), name
    if c["packed"] and c["causal"]:
        assert packed_qkv(dq, dk, dv), "dq, dk, dv are not the views of one packed gradient"
    elif c["packed"]:
        assert _packed_kv(dk, dv), "dk, dv are not the views of one packed gradient"


@pytest.mark.parametrize("name", ["packed_self_hd64", "packed_cross_hd8"])
def test_packed_projection_receives_one_packed_gradient(name):
    """Through glue.split_heads3 / split_heads_kv the leaf behind the views gets the kernels' packed buffer as it is."""
    from csa_amd.glue import split_heads3
    from csa_amd.seq_attn_ops import seq_attention, split_heads_kv
    c = ref.CASES[name]
    inputs = ref.build(c)
    q, k, v, mask, dout = _to_gpu(c, inputs)
    R, H, T, hd, S = (c[n] for n in ("R", "H", "T", "hd", "S"))
    want = ref.oracle(c, *inputs)
    if c["causal"]:
        leaf = torch.stack([t.transpose(1, 2) for t in (q, k, v)], 2).reshape(R, T, 3 * H * hd).requires_grad_()
        out = seq_attention(*split_heads3(leaf, H), mask, causal=True, mask_mode=c["mode"])
        out.backward(dout)
        g = leaf.grad.view(R, T, 3, H, hd)
        got = [g[:, :, i].transpose(1, 2) for i in range(3)]
    else:
        ql = q.detach().requires_grad_()
        leaf = torch.stack([t.transpose(1, 2) for t in (k, v)], 2).contiguous().requires_grad_()
        out = seq_attention(ql, *split_heads_kv(leaf), mask, kv_group=c["G"])
        out.backward(dout)
        got = [ql.grad] + [leaf.grad[:, :, i].transpose(1, 2) for i in range(2)]
    ref.check(c, [out.detach()] + got, inputs, want, what="leaf ")


@pytest.mark.parametrize("name", ["causal_reference_hd64_T17", "group_hd8_G3", "cross_hd64_T50_S150"])
def test_two_runs_are_bitwise_equal(name):
    c = ref.CASES[name]
    gpu = _to_gpu(c, ref.build(c))
    a, b = _run(c, gpu), _run(c, gpu)
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), name


@pytest.mark.parametrize("hd, T", [(16, 5), (8, 257)])
def test_unsupported_shapes_take_the_torch_path_on_the_device(hd, T):
    """A head dim other than 8 / 64 and T > 256 report unsupported; the op then runs its torch definition where the
    tensors are, with the same result as on the CPU."""
    from csa_amd._lib import lib
    from csa_amd.seq_attn_ops import seq_attention
    assert not lib().csa_seq_attn_supported(hd, T, T)
    c = ref.case("unsupported", 2, 2, hd, T, T, causal=True, mask="pad", seed=9)
    q, k, v, mask, dout = ref.build(c)
    want = seq_attention(q, k, v, mask, causal=True)
    got = seq_attention(q.cuda(), k.cuda(), v.cuda(), mask.cuda(), causal=True)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-5)


def test_fully_masked_query_row_gives_nan_in_that_row_only():
    c, inputs = ref.fully_masked_case()
    got = _run(c, _to_gpu(c, inputs))
    torch.cuda.synchronize()  # both passes returned
    want = ref.oracle(c, *inputs)[0]
    assert bool(torch.isnan(want[2, 0]).all()) and int(torch.isnan(want).sum()) == want.shape[2]
    e = ref.finite_err(got[0], want)  # NaN exactly where the oracle's softmax of an all -inf row is
    print(f"fully masked row: out err {e:.3e} bound {ref.FACTOR * ref.BASELINE_FULLY_MASKED_OUT:.3e}")
    assert e <= ref.FACTOR * ref.BASELINE_FULLY_MASKED_OUT
    other = [r for r in range(c["R"]) if r != 2]
    for g in got[1:]:  # the rows that do not read row 2's keys are untouched by it
        assert bool(torch.isfinite(g[other]).all())


# ---- the scorer on the tiny model ----

def _tiny(seed, gen_scale=1.0, eos_bias=0.0):
    from csa_amd.model import CSATrans
    m = CSATrans(**TINY)
    fill_params_deterministic(m, seed)
    with torch.no_grad():
        m.generator.linear.weight.mul_(gen_scale)
        m.generator.linear.bias[EOS_ID] += eos_bias
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _model_case():
    """The tiny model, three synthetic ASTs and their encoder output, computed once on the GPU."""
    from csa_amd.data import synthetic_batch
    from csa_amd.model import batch_to_device
    m = _tiny(6, 8.0, 2.0)
    sb = synthetic_batch(3, max_size=20, seed=4, min_nodes=12, max_nodes=20, src_vocab=50, tgt_vocab=60, max_tgt_len=9)
    data, _ = batch_to_device(sb, torch.device("cuda"))
    torch.manual_seed(3)
    with torch.no_grad():
        m.process_data(data)
        enc = m.encode(data)[0]
    return m, enc, data.src_mask


@pytest.mark.parametrize("head_mask", ["own", "reference"])
def test_fused_scorer_matches_the_loop_oracle_and_sdpa(head_mask):
    from csa_amd.model import SequenceScorer
    m, enc, src_mask = _model_case()
    cand = score_ref.scorer_case()[2].cuda()  # (B = 3, G = 2, T = 7)
    scorer = SequenceScorer(m, EOS_ID, head_mask, attention="fused")
    with torch.no_grad():
        out = scorer.score(enc, src_mask, cand, return_tokens=True)
        sdpa = SequenceScorer(m, EOS_ID, head_mask).score(enc, src_mask, cand, return_tokens=True)
    assert scorer.last_attention == "fused"
    tokens, logp, length = score_ref.score_loop_ref(m, enc, src_mask, cand.cpu(), EOS_ID, head_mask)
    got = out.tokens.view(6, -1).cpu()
    print("fused vs fp64", (got.double() - tokens).abs().max().item(),
          "fused vs sdpa", (out.tokens - sdpa.tokens).abs().max().item())
    np.testing.assert_allclose(got.numpy(), tokens.numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out.logp.view(-1).cpu().numpy(), logp.numpy(), rtol=RTOL, atol=ATOL)
    assert out.length.view(-1).tolist() == length.tolist()
    np.testing.assert_allclose(out.tokens.cpu().numpy(), sdpa.tokens.cpu().numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(out.logp.cpu().numpy(), sdpa.logp.cpu().numpy(), rtol=RTOL, atol=ATOL)


def test_fused_scorer_equals_the_beams_scores():
    from csa_amd.model import BeamSearchGenerator, SequenceScorer
    m, enc, src_mask = _model_case()
    _, ids, scores = BeamSearchGenerator(m, 8, 3, length_penalty=0.0).search(enc, src_mask, return_all=True)
    scorer = SequenceScorer(m, attention="fused")
    with torch.no_grad():
        out = scorer.score(enc, src_mask, ids)
    assert scorer.last_attention == "fused"
    print("fused scorer vs beam", (out.logp - scores).abs().max().item())
    np.testing.assert_allclose(out.logp.cpu().numpy(), scores.cpu().numpy(), rtol=2 * RTOL, atol=2 * ATOL)


def test_fused_scorer_gradients_match_sdpa_on_the_gpu():
    from csa_amd.model import SequenceScorer
    m, enc, src_mask = _model_case()
    cand = score_ref.scorer_case()[2].cuda()
    params = {k: p for k, p in m.named_parameters() if k.startswith(("decoder.", "generator.", "tgt_embedding."))}

    def grads(attention):
        m.zero_grad(set_to_none=True)
        e = enc.clone().requires_grad_()
        SequenceScorer(m, EOS_ID, attention=attention).score(e, src_mask, cand).logp.sum().backward()
        out = {k: p.grad.detach().clone() for k, p in params.items() if p.grad is not None}
        out["enc"] = e.grad.detach().clone()
        return out
    try:
        got, want = grads("fused"), grads("sdpa")
    finally:
        m.zero_grad(set_to_none=True)
    assert got.keys() == want.keys() and len(got) > 20
    for k in want:
        np.testing.assert_allclose(got[k].cpu().numpy(), want[k].cpu().numpy(), rtol=1e-3, atol=2e-5, err_msg=k)


def test_fused_scorer_never_holds_the_repeated_memory_projection():
    """One decoder layer, E = 512, H = 8, B = 8, G = 4, S = 150, T = 8, V = 60, no_grad: "sdpa" projects B * G * S memory
    rows to 2 E columns, "fused" B * S, so its peak above the inputs is lower by at least the B * (G - 1) * S * 2 E fp32
    values it never computes. T and V are small so that nothing else sets the peak."""
    from csa_amd.model import SequenceScorer
    B, G, S, T, E, V = 8, 4, 150, 8, 512, 60
    m = score_ref.decoder_stub(E=E, H=8, V=V, ffn=128, layers=1).cuda()
    g = torch.Generator().manual_seed(4)
    enc = torch.randn(B, S, E, generator=g).cuda()
    src_mask = torch.zeros(B, S, dtype=torch.bool)
    src_mask[1, S - 7:] = True
    src_mask = src_mask.cuda()
    cand = torch.randint(4, V, (B, G, T), generator=g).cuda()

    def peak(attention):
        scorer = SequenceScorer(m, None, attention=attention)
        with torch.no_grad():
            scorer.score(enc, src_mask, cand)  # warm: workspaces of the GEMM library are allocated once
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = scorer.score(enc, src_mask, cand)
            torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out.logp

    p_fused, a = peak("fused")
    p_sdpa, b = peak("sdpa")
    need = B * (G - 1) * S * 2 * E * 4
    print(f"peak bytes above the inputs: fused {p_fused}, sdpa {p_sdpa}, difference {p_sdpa - p_fused}, required {need}")
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=1e-4)
    assert p_sdpa - p_fused >= need
