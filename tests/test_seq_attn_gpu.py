"""The full-sequence decoder attention on the GPU (csrc/csa_seqattn.hip through seq_attn_ops.seq_attention): every case
of tests/seq_attn_ref.py against the fp64 oracle within four times the parent's error, forward and the three gradients
(16 and 19 key tiles, G = 4, odd head counts, masked leading tiles, wide logits among them); packed operands and packed
gradients; exact zeros at masked keys; operands, masks and upstream gradients handed over in other layouts; no store
outside the addressed output elements; bitwise determinism; a fully masked query row;
SequenceScorer(attention="fused") on the tiny model against the loop oracle, "sdpa" and the beam's scores; peak memory."""
import ctypes
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
    if c["mask"] == "last_only":  # p = 1, l = 1: out is the last V row of the AST and head, bit for bit
        v = inputs[2]
        want = v[:, :, c["S"] - 1].repeat_interleave(c["G"], 0).reshape(c["R"], 1, -1).expand(-1, c["T"], -1)
        assert torch.equal(out.cpu().view(torch.int32), want.contiguous().view(torch.int32)), name
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


# ---- the same values in other layouts ----

LAYOUT_CASES = [n for n in ref.CASES if n.startswith("layout_") and not n.endswith("_doutrow")]


@functools.lru_cache(maxsize=None)
def _layout_case(name):
    """Case, CPU inputs, fp64 oracle and the plain tensors on the GPU: computed once, never modified."""
    c = ref.CASES[name]
    inputs = ref.build(c)
    return c, inputs, ref.oracle(c, *inputs), _to_gpu(c, inputs)


def _transposed(t):
    """The same (N, H, L, hd) values stored as (N, L, H, hd): a head-major view with other strides."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _offset1(t):
    """The same values as a view of a flat buffer that starts at element 1: 4 bytes off every alignment."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:].copy_(t.reshape(-1))
    return flat[1:].view(t.shape)


def _padded(t):
    """The same values as the slice [..., :hd] of a tensor whose last dimension is hd + 2: row stride hd + 2."""
    wide = torch.zeros(*t.shape[:-1], t.shape[-1] + 2, dtype=t.dtype, device=t.device)
    wide[..., :t.shape[-1]] = t
    return wide[..., :t.shape[-1]]


def _run_spied(c, q, k, v, mask, dout, monkeypatch):
    """_run, also returning the (q, k, v) that reached _SeqAttn.apply."""
    from csa_amd import seq_attn_ops
    seen, real = [], seq_attn_ops._SeqAttn.apply
    monkeypatch.setattr(seq_attn_ops._SeqAttn, "apply", staticmethod(lambda *a: (seen.append(a[:3]), real(*a))[1]))
    got = _run(c, (q, k, v, mask, dout))
    assert len(seen) == 1
    return got, seen[0]


@pytest.mark.parametrize("which, form", [(w, f) for f in ("transposed", "offset1", "padded") for w in "qkv"])
@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_one_operand_in_another_layout(name, which, form, monkeypatch):
    """ONE of q, k, v in another layout, the other two contiguous: k and v (or q and the output rows) then have different
    strides, and a kernel that read one with the other's would leave the bound. A transposed operand is read in place;
    one that is misaligned or has a row stride that is no multiple of 4 is copied."""
    from csa_amd.seq_attn_ops import _operand
    c, inputs, want, (q, k, v, mask, dout) = _layout_case(name)
    ops = dict(q=q, k=k, v=v)
    plain = ops[which]
    t = dict(transposed=_transposed, offset1=_offset1, padded=_padded)[form](plain)
    assert torch.equal(t, plain) and (form == "offset1" or t.stride() != plain.stride())
    ops[which] = t
    got, seen = _run_spied(c, ops["q"], ops["k"], ops["v"], mask, dout, monkeypatch)
    for n, passed in zip("qkv", seen):
        in_place = n != which or form == "transposed"
        assert (_operand(ops[n]) is ops[n]) == in_place, (n, form)
        assert (passed.data_ptr() == ops[n].data_ptr()) == in_place, (n, form)
        assert passed.data_ptr() % 16 == 0 and passed.stride(-1) == 1 and not any(s % 4 for s in passed.stride()[:-1])
        if in_place:
            assert passed.stride() == ops[n].stride()
    ref.check(c, got, inputs, want, what=f"{which} {form} ")


@pytest.mark.parametrize("form", ["bool", "wide", "wide_view"])
@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_key_mask_forms_are_bitwise_equal(name, form):
    """torch.bool, (rows, S + 5) with the columns past S all set (ignored), and its [:, :S] view (row stride above S):
    the same bits as the plain uint8 (rows, S) run in out and the three gradients."""
    c, _, _, (q, k, v, mask, dout) = _layout_case(name)
    S = c["S"]
    wide = torch.cat([mask, torch.ones(mask.shape[0], 5, dtype=torch.uint8, device="cuda")], 1)
    other = dict(bool=mask.bool(), wide=wide, wide_view=wide[:, :S])[form]
    assert form != "wide_view" or (other.stride(0) == S + 5 and other.shape == mask.shape)
    a, b = _run(c, (q, k, v, mask, dout)), _run(c, (q, k, v, other, dout))
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), (name, form)


@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_non_contiguous_upstream_gradient(name):
    """dout with the same values and other strides, and (the _doutrow case) a stride-0 expansion of one row."""
    c, inputs, want, (q, k, v, mask, dout) = _layout_case(name)
    other = dout.transpose(1, 2).contiguous().transpose(1, 2)
    assert torch.equal(other, dout) and (c["T"] == 1 or other.stride() != dout.stride())
    ref.check(c, _run(c, (q, k, v, mask, other)), inputs, want, what="dout transposed ")
    c, inputs, want, (q, k, v, mask, _) = _layout_case(name + "_doutrow")
    row = inputs[4][:1, :1].contiguous().cuda().expand(c["R"], c["T"], -1)
    assert row.stride() == (0, 0, 1) and torch.equal(row.cpu(), inputs[4])
    ref.check(c, _run(c, (q, k, v, mask, row)), inputs, want, what="dout expanded ")


# ---- nothing is stored outside the outputs ----

SENTINEL = 0x7FA5C3E1  # as fp32 a NaN with a payload no result carries; compared as int32
GUARD = 64  # sentinel floats before and after every tensor


def _carve(shape, strides):
    """-> (int32 sentinel buffer, fp32 view of `shape` / `strides` inside it after GUARD elements, bool map of the
    addressed elements)."""
    span = sum((n - 1) * s for n, s in zip(shape, strides)) + 1
    buf = torch.full((GUARD + (span + 3) // 4 * 4 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    t = buf.view(torch.float32).as_strided(shape, strides, GUARD)
    addressed = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
    addressed.as_strided(shape, strides, GUARD).fill_(True)
    assert t.data_ptr() % 16 == 0 and int(addressed.sum()) == t.numel()
    return buf, t, addressed


def _stray_cases():
    out = []
    for hd in (8, 64):
        for T in (1, 17):
            for S in (1, 17, 33):
                out.append(ref.case(f"stray_cross_hd{hd}_T{T}_S{S}", 4, 2, hd, T, S, G=2, mask="memory" if S > 1 else None,
                                    seed=1000 + len(out)))
        out.append(ref.case(f"stray_causal_hd{hd}_T17", 2, 2, hd, 17, 17, causal=True, mask="pad", seed=1000 + len(out)))
    return {c["name"]: c for c in out}


STRAY_CASES = _stray_cases()


@pytest.mark.parametrize("name", list(STRAY_CASES))
def test_no_store_outside_the_addressed_output_elements(name):
    """csa_seq_attn_fwd / _bwd through the C ABI with out, lse, the workspace and the gradients carved out of
    sentinel-filled buffers: guards of 64 floats around each, and for the gradients a T / S stride of H * hd + 8, a head
    stride of hd + 4 and spare elements between rows of the batch. Every sentinel outside the addressed elements survives
    (for hd = 8 the other half of the 16-wide head-dim tile would land in the gap after the head), every addressed
    element is written, and the values are the bits seq_attention gives with outputs of its own."""
    from csa_amd import _lib
    c = STRAY_CASES[name]
    R, H, hd, T, S, G = (c[n] for n in ("R", "H", "hd", "T", "S", "G"))
    B, row = R // G, H * hd + 8
    q, k, v, mask, dout = gpu = _to_gpu(c, ref.build(c))
    want = _run(c, gpu)
    bufs = dict(out=_carve((R, T, H * hd), (T * H * hd, H * hd, 1)),
                lse=_carve((R, H, T), (H * T, T, 1)),
                ws=_carve((R, H, T), (H * T, T, 1)),
                dq=_carve((R, H, T, hd), (T * row + 16, hd + 4, row, 1)),
                dk=_carve((B, H, S, hd), (S * row + 16, hd + 4, row, 1)),
                dv=_carve((B, H, S, hd), (S * row + 32, hd + 4, row, 1)))
    t = {n: b[1] for n, b in bufs.items()}
    assert H * (hd + 4) <= row  # the heads of a row and their spare elements fit below the next row
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    L = _lib.lib()
    a = _lib.SeqAttnArgs(R=R, H=H, T=T, S=S, hd=hd, kv_group=G,
                         q=p(q), q_sr=q.stride(0), q_sh=q.stride(1), q_st=q.stride(2),
                         k=p(k), k_sb=k.stride(0), k_sh=k.stride(1), k_sn=k.stride(2),
                         v=p(v), v_sb=v.stride(0), v_sh=v.stride(1), v_sn=v.stride(2),
                         mask=p(mask) if mask is not None else None, mask_ld=mask.stride(0) if mask is not None else 0,
                         mask_mode=0, causal=int(c["causal"]), scale=float(hd) ** -0.5, out=p(t["out"]), lse=p(t["lse"]))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.csa_seq_attn_fwd(ctypes.byref(a), stream), "csa_seq_attn_fwd")
    b = _lib.SeqAttnBwdArgs(fwd=ctypes.pointer(a), dout=p(dout), workspace=p(t["ws"]),
                            dq=p(t["dq"]), dq_sr=t["dq"].stride(0), dq_sh=t["dq"].stride(1), dq_st=t["dq"].stride(2),
                            dk=p(t["dk"]), dk_sb=t["dk"].stride(0), dk_sh=t["dk"].stride(1), dk_sn=t["dk"].stride(2),
                            dv=p(t["dv"]), dv_sb=t["dv"].stride(0), dv_sh=t["dv"].stride(1), dv_sn=t["dv"].stride(2))
    _lib.check(L.csa_seq_attn_bwd(ctypes.byref(b), stream), "csa_seq_attn_bwd")
    torch.cuda.synchronize()
    for n, (buf, _, addressed) in bufs.items():
        written = buf != SENTINEL
        assert not bool((written & ~addressed).any()), f"{name}: a store outside {n}"
        assert bool(written[addressed].all()), f"{name}: {n} has elements that were never written"
    for n, x in zip(("out", "dq", "dk", "dv"), want):
        assert torch.equal(t[n].contiguous().view(torch.int32), x.contiguous().view(torch.int32)), (name, n)


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
