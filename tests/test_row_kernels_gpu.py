"""Every launch class of the small per-row kernels around the attention kernels, against fp64 on the CPU computed from
the same fp32 inputs:

  generator log-softmax (csrc/csa_gen.hip)   reg_groups 1..6 (k_gen_*_r<NG>) and the two-pass loop kernels, both sides of
                                             every threshold, underflowed rows, a 4-byte aligned row base;
  LayerNorm / k_decode_embed (csa_ln_row.hpp) CPL 1..4, each with a partial last chunk, partial workgroups, constant and
                                             ill-conditioned rows;
  csa_bias_grad through the C ABI            accumulate, rows == 0, the scalar loads of a 4-byte aligned dy;
  k_argmax_rows / k_beam_row_topk            the scalar loads of a 4-byte aligned base with V % 4 == 0;
  k_decode_attn                              that the case lists of test_decode_gpu / test_decode_graph_gpu / test_beam_gpu
                                             hold head dims whose float4 count does not divide the wave, and hd = 4.

The dispatch rules are restated here and pinned to the source lines they restate, so a moved threshold fails here
instead of quietly shrinking the coverage.

Tolerance: the project's fp32 rule, rtol 1e-4 with atol 1e-5 (times max(1, max|ref|) where a value is a sum over rows)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import PKG, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]
RTOL, ATOL = 1e-4, 1e-5
SEED = 0x1234_5678_9ABC_DEF0


def _source(name):
    with open(os.path.join(PKG, "csrc", name)) as f:
        return f.read()


def _close(got, ref, what, scaled=False):
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    atol = ATOL * max(1.0, float(np.abs(ref).max())) if scaled and ref.size else ATOL
    np.testing.assert_allclose(got.detach().cpu().numpy(), ref, rtol=RTOL, atol=atol, err_msg=what)


def _offset_view(x):
    """x's values in a CUDA tensor of the same shape whose storage starts one float into an allocation: contiguous,
    4-byte but not 16-byte aligned."""
    buf = torch.empty(x.numel() + 8, dtype=x.dtype, device="cuda")
    v = buf[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ---- A. generator log-softmax ----

GEN_LOOP = 0  # the class of k_gen_fwd / k_gen_bwd


def reg_groups(V):
    """csa_gen.hip: groups of 8 columns per thread of a 512-thread row (1..6), or 0 for the loop kernels."""
    per = -(-(-(-V // 8)) // 512)
    return per if per <= 6 else GEN_LOOP


# (V, class): both sides of every threshold; 49999 is odd (scalar loads and stores in the loop kernels), 32768 takes
# their vector path
GEN_SIZES = [(4096, 1), (4097, 2), (8192, 2), (8200, 3), (12288, 3), (12289, 4), (16384, 4), (16385, 5), (20480, 5),
             (20481, 6), (24576, 6), (24577, GEN_LOOP), (49999, GEN_LOOP), (32768, GEN_LOOP)]


def test_generator_sizes_cover_every_launch_class():
    src = _source("csa_gen.hip")
    for line in ("constexpr int RT = 512;", "const int64_t per = ((V + 7) / 8 + RT - 1) / RT;",
                 "return per <= 6 ? (int)per : 0;"):
        assert line in src, f"csa_gen.hip no longer has `{line}`: restate reg_groups here and move GEN_SIZES with it"
    for ng in range(1, 7):
        assert f"case {ng}: hipLaunchKernelGGL(k_gen_fwd_r<{ng}>" in src and f"k_gen_bwd_r<{ng}>" in src, ng
    assert [reg_groups(V) for V, _ in GEN_SIZES] == [c for _, c in GEN_SIZES]
    assert {c for _, c in GEN_SIZES} == {GEN_LOOP, 1, 2, 3, 4, 5, 6}
    for c in range(1, 7):  # the last size of a class and the first of the next
        assert reg_groups(4096 * c) == c and reg_groups(4096 * c + 1) == (c + 1 if c < 6 else GEN_LOOP)


def _gen_keep(rows, V, p):
    from oracle import philox
    if p == 0:
        return torch.ones(rows, V, dtype=torch.bool)
    return torch.from_numpy(philox.gen_keep(rows, V, SEED, 0, p))


def _gen_chain(z, keep, p, dout, dtype):
    """log(softmax(dropout(z))) and its gradient as the reference model's op chain, in `dtype` on the CPU."""
    zc = z.detach().to(dtype, copy=True).requires_grad_(True)
    ref = torch.log(torch.softmax(zc * keep.to(dtype) / (1.0 - p), -1))
    ref.backward(dout.to(dtype))
    return ref.detach(), zc.grad


def _gen_run(z, dout, p, monkeypatch):
    from csa_amd import gen_ops
    monkeypatch.setattr(gen_ops, "_draw_seed", lambda: SEED)
    zg = z.detach().requires_grad_(True)
    out = gen_ops.gen_log_softmax(zg, p)
    seen = []
    out.register_hook(lambda g: seen.append(g.data_ptr()))  # the dlogp the backward kernel is handed
    out.backward(dout)
    assert (zg.data_ptr(), seen[0]) == (z.data_ptr(), dout.data_ptr())
    return out.detach(), zg.grad


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("V,cls", GEN_SIZES)
def test_generator_matches_fp64_in_every_launch_class(V, cls, p, monkeypatch):
    """dout is scaled by 1 / sqrt(V) so that the row sum of the backward stays O(1) and the plain atol applies."""
    assert reg_groups(V) == cls
    rows = 3
    g = torch.Generator().manual_seed(V)
    z = torch.randn(rows, V, generator=g) * 3.0
    dout = torch.randn(rows, V, generator=g) / np.sqrt(V)
    out, dz = _gen_run(z.cuda(), dout.cuda(), p, monkeypatch)
    ref, dref = _gen_chain(z, _gen_keep(rows, V, p), p, dout, torch.float64)
    _close(out, ref, "logp")
    _close(dz, dref, "dlogits")


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("V,cls", [(24584, GEN_LOOP), (12289, 4)])
def test_generator_underflowed_row(V, cls, p, monkeypatch):
    """Row 1 has one logit raised and a few hundred pushed far down: their probabilities underflow to an exact 0, so
    log(softmax) is -inf there and the row's gradient is NaN, as torch computes the chain in fp32. No column lies where
    exp is an fp32 denormal (a device that flushes them and the host may differ there): every one is within 80 of the
    row maximum or more than 120 below it. The other rows are compared with fp64 as usual."""
    assert reg_groups(V) == cls
    rows = 3
    g = torch.Generator().manual_seed(V + 1)
    z = torch.randn(rows, V, generator=g) * 3.0
    dout = torch.randn(rows, V, generator=g) / np.sqrt(V)
    low = torch.cat([torch.arange(5, V, 37), torch.tensor([0, V - 1, V - 2, V - 9])])  # incl. the row's ragged tail
    z[1, low] = -100.0 - torch.rand(low.numel(), generator=g) * 20.0
    keep = _gen_keep(rows, V, p)
    z[1, 100 + int(keep[1, 100:].nonzero()[0])] = 40.0  # a column that the dropout keeps
    x = z.double() * keep.double() / (1.0 - p)
    gap = x[1].max() - x[1]
    assert bool(((gap < 80) | (gap > 120)).all()) and int((gap > 120).sum()) >= 200
    out, dz = _gen_run(z.cuda(), dout.cuda(), p, monkeypatch)
    out, dz = out.cpu(), dz.cpu()
    ref32, dref32 = _gen_chain(z, keep, p, dout, torch.float32)
    assert bool(torch.isinf(ref32[1]).any()) and bool(torch.isnan(dref32[1]).all())  # the case shows what it is built for
    assert torch.equal(torch.isinf(out), torch.isinf(ref32)) and bool((out[torch.isinf(out)] < 0).all())
    assert torch.equal(torch.isnan(dz), torch.isnan(dref32))
    fin = torch.isfinite(ref32[1])
    _close(out[1][fin], ref32[1][fin], "logp of the underflowed row")
    ref, dref = _gen_chain(z, keep, p, dout, torch.float64)
    for r in (0, 2):
        _close(out[r], ref[r], f"logp row {r}")
        _close(dz[r], dref[r], f"dlogits row {r}")


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("V,cls", [(4100, 2), (24580, GEN_LOOP)])
def test_generator_scalar_path_of_a_4_byte_aligned_base_is_bitwise_the_vector_path(V, cls, p, monkeypatch):
    """V % 4 == 0 with logits and dlogp one float off a 16-byte boundary (contiguous views, which GenLogSoftmax keeps):
    the kernels' vec == false branch gives the bits of the aligned call."""
    assert reg_groups(V) == cls and V % 4 == 0
    rows = 2
    g = torch.Generator().manual_seed(V)
    z = torch.randn(rows, V, generator=g) * 3.0
    dout = torch.randn(rows, V, generator=g) / np.sqrt(V)
    want, dwant = _gen_run(z.cuda(), dout.cuda(), p, monkeypatch)
    got, dgot = _gen_run(_offset_view(z), _offset_view(dout), p, monkeypatch)
    assert torch.equal(got, want) and torch.equal(dgot, dwant)
    ref, dref = _gen_chain(z, _gen_keep(rows, V, p), p, dout, torch.float64)
    _close(got, ref, "logp")
    _close(dgot, dref, "dlogits")


# ---- B. decode attention: head dims whose float4 count does not divide the wave ----

def test_decode_attention_case_lists_hold_non_dividing_head_dims():
    """k_decode_attn leaves 64 % (hd / 4) lanes idle in its P.V phase when hd / 4 does not divide 64, and hd = 4 makes
    one key group per lane: the plain, device-stepped and both beam forms each run at least three such head dims, and 4."""
    import test_beam_gpu
    import test_decode_graph_gpu
    import test_decode_gpu
    assert "const bool pv_lane = kg < KG;" in _source("csa_decode.hip")
    lists = {"plain": [c[2] for c in test_decode_gpu.CASES],
             "device-stepped": [c[2] for c in test_decode_graph_gpu.STEP_CASES],
             "beam": [c[0] for c in test_beam_gpu.ATTN_CASES]}
    for name, hds in lists.items():
        assert all(hd % 4 == 0 and 4 <= hd <= 128 for hd in hds), name
        odd = {hd for hd in hds if 64 % (hd // 4) != 0}
        assert len(odd) >= 3 and 4 in hds, (name, sorted(odd))
        assert {4, 12, 96} <= set(hds), name


# ---- C. LayerNorm and k_decode_embed ----

def ln_cpl(cols):
    """csa_ln_row.hpp: dwordx4 chunks per lane of a one-wave row (1..4), or 0 when the row path does not take it."""
    if cols < 4 or cols % 4:
        return 0
    cpl = (cols + 255) // 256
    return cpl if cpl <= 4 else 0


LN_COLS = [(4, 1), (252, 1), (260, 2), (508, 2), (516, 3), (772, 4), (1020, 4), (1024, 4)]
LN_ROWS = [1, 5, 33, 130]  # partial groups of 4 rows (forward) and partial workgroups of 32 rows (backward)


def test_layernorm_sizes_cover_every_cpl_with_a_partial_chunk():
    src = _source("csa_ln_row.hpp")
    for line in ("const int64_t cpl = (cols + 255) / 256;", "return cpl <= 4 ? (int)cpl : 0;"):
        assert line in src, f"csa_ln_row.hpp no longer has `{line}`: restate ln_cpl here and move LN_COLS with it"
    assert [ln_cpl(c) for c, _ in LN_COLS] == [k for _, k in LN_COLS]
    for k in (1, 2, 3, 4):  # a row whose last chunk covers only part of the wave
        assert any(ln_cpl(c) == k and c % 256 != 0 for c, _ in LN_COLS), k
    assert any(c % 256 == 0 for c, _ in LN_COLS)
    assert any(r % 4 for r in LN_ROWS) and any(r > 32 and r % 32 for r in LN_ROWS)


def _ln64(x, w, b, eps=1e-5):
    """LayerNorm over the last dim in fp64, written out: mean, biased variance, eps inside the root."""
    x, w, b = x.double(), w.double(), b.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w + b


def _ln_fwd_bwd64(x, w, b, gy):
    x, w, b = (t.double().requires_grad_(True) for t in (x, w, b))
    y = _ln64(x, w, b)
    y.backward(gy.double())
    return y.detach(), x.grad, w.grad, b.grad


def _ln_module(w, b):
    from csa_amd.glue import LayerNorm
    ln = LayerNorm(w.numel()).cuda()
    with torch.no_grad():
        ln.weight.copy_(w)
        ln.bias.copy_(b)
    return ln


def _ln_run(x, w, b, gy, monkeypatch):
    """glue.LayerNorm on the GPU through csa_layernorm_fwd / _bwd (torch's own LayerNorm must not run)."""
    def no_fallback(*a, **k):
        raise AssertionError("glue.LayerNorm fell back to torch.nn.LayerNorm")
    monkeypatch.setattr(torch.nn.LayerNorm, "forward", no_fallback)
    ln = _ln_module(w, b)
    xg = x.cuda().requires_grad_(True)
    y = ln(xg)
    y.backward(gy.cuda())
    return y.detach(), xg.grad, ln.weight.grad, ln.bias.grad


def _ln_check(x, w, b, gy, monkeypatch, what=""):
    got = _ln_run(x, w, b, gy, monkeypatch)
    ref = _ln_fwd_bwd64(x, w, b, gy)
    _close(got[0], ref[0], what + "y")
    for name, a, r in zip(("dx", "dgamma", "dbeta"), got[1:], ref[1:]):
        _close(a, r, what + name, scaled=True)
    return got, ref


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("cols,cpl", LN_COLS)
def test_layernorm_matches_fp64(rows, cols, cpl, monkeypatch):
    assert ln_cpl(cols) == cpl
    g = torch.Generator().manual_seed(1000 * rows + cols)
    x = torch.randn(rows, cols, generator=g) * 3 + 1
    w, b = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    gy = torch.randn(rows, cols, generator=g)
    _ln_check(x, w, b, gy, monkeypatch)


@pytest.mark.parametrize("cols", [4, 260, 1020])
def test_layernorm_constant_rows(cols, monkeypatch):
    """Rows of variance 0 between ordinary ones: y = beta there and dx follows fp64 (rstd = 1 / sqrt(eps) = 316). The
    constants are dyadic, so the fp32 row sum and the mean are exact and x - mean is an exact 0; with any other
    constant the rounding of the mean, multiplied by rstd, is the error of every fp32 implementation."""
    g = torch.Generator().manual_seed(cols)
    x = torch.randn(5, cols, generator=g) * 3 + 1
    x[1], x[3] = 3.5, -0.75
    w, b = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    gy = torch.randn(5, cols, generator=g)
    got, ref = _ln_check(x, w, b, gy, monkeypatch)
    for r in (1, 3):
        assert float(ref[0][r].sub(b.double()).abs().max()) == 0.0
        _close(got[0][r], b, f"y of constant row {r}")


@pytest.mark.parametrize("cols", [260, 1020])
@pytest.mark.parametrize("kind", ["100+randn", "1000+0.1*randn"])
def test_layernorm_ill_conditioned_rows(kind, cols, monkeypatch):
    """Large mean, small variance: the error of fp32 is set by the rounding of the mean (about ulp(mean) / std), not
    by a tolerance chosen in advance. The yardstick is torch's own fp32 LayerNorm on the CPU against fp64 on the same
    inputs: the kernel's maximum error must stay within 4 times that (plus the atol floor). A one-pass
    E[x^2] - mean^2 is off by orders of magnitude here. 33 rows, so that each maximum is over many row means."""
    g = torch.Generator().manual_seed(cols + len(kind))
    r = torch.randn(33, cols, generator=g)
    x = 100 + r if kind == "100+randn" else 1000 + 0.1 * r
    w, b = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    gy = torch.randn(33, cols, generator=g)
    y = _ln_run(x, w, b, gy, monkeypatch)[0].cpu()
    ref = _ln64(x, w, b)
    cpu = torch.nn.functional.layer_norm(x, (cols,), w, b, 1e-5)
    e_kernel = float((y.double() - ref).abs().max())
    e_cpu = float((cpu.double() - ref).abs().max())
    msg = f"{kind} cols={cols}: kernel max error {e_kernel:.3e}, fp32 CPU layer_norm max error {e_cpu:.3e}"
    print(msg)
    assert e_kernel <= 4 * e_cpu + ATOL, msg


@pytest.mark.parametrize("t", [0, 7])
@pytest.mark.parametrize("E,cpl", [(260, 2), (772, 4)])
def test_decode_embed_with_a_partial_chunk(E, cpl, t):
    """k_decode_embed at embedding widths whose last chunk is partial: bitwise Embeddings.step, and within tolerance of
    the fp64 gather + add + LayerNorm; one row gathers the last vocabulary index, one the first."""
    from csa_amd.decode_ops import decode_embed
    from csa_amd.model import Embeddings
    assert ln_cpl(E) == cpl and E % 256 != 0
    torch.manual_seed(E + t)
    B, vocab, T = 3, 37, 9
    emb = Embeddings(E, vocab, 0.1, with_pos=True).cuda().eval()
    with torch.no_grad():
        emb.norm.weight.add_(0.1 * torch.randn_like(emb.norm.weight))
        emb.norm.bias.add_(0.1 * torch.randn_like(emb.norm.bias))
        emb.word_embeddings.weight[0].normal_()  # the padding row, zero at init
    buf = torch.randint(0, vocab, (B, T + 5), device="cuda")
    ys = buf[:, 2:2 + T]  # row stride T + 5, storage offset 2
    ys[0, t], ys[B - 1, t] = 0, vocab - 1
    step = torch.tensor([t], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        want = emb.step(ys[:, t:t + 1], t)
        got = decode_embed(ys, step, emb)
    assert got.shape == (B, E) and torch.equal(got, want[:, 0])
    W, pe = emb.word_embeddings.weight.detach().cpu().double(), emb.pos_emb.pe[0].detach().cpu().double()
    ref = _ln64(W[ys[:, t].cpu()] + pe[t], emb.norm.weight.detach().cpu(), emb.norm.bias.detach().cpu(), emb.norm.eps)
    _close(got, ref, "fp64 gather + add + LayerNorm")


# ---- D. csa_bias_grad through the C ABI ----

def bg_slices(rows):
    """csa_glue.hip: row slices of the first pass, at least 256 rows each, at most 64."""
    return min(64, max(1, (rows + 255) // 256))


def _bias_grad_abi(dy, db, rows, cols, accumulate):
    from csa_amd._lib import check, lib
    L = lib()
    ws = torch.empty(max(1, L.csa_bias_grad_workspace_bytes(rows, cols)), dtype=torch.uint8, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(L.csa_bias_grad(ptr(dy), ptr(db), rows, cols, accumulate, ptr(ws), stream), "csa_bias_grad")
    return db


@pytest.mark.parametrize("rows,cols", [(255, 65), (1, 4), (20000, 64)])
def test_bias_grad_accumulates_onto_db(rows, cols):
    assert "return (int)(rs < 1 ? 1 : rs > 64 ? 64 : rs);" in _source("csa_glue.hip")
    assert bg_slices(20000) == 64 and bg_slices(255) == 1
    g = torch.Generator().manual_seed(rows + cols)
    dy = torch.randn(rows, cols, generator=g)
    pre = torch.randn(cols, generator=g) * 10
    ref = dy.double().sum(0)
    _close(_bias_grad_abi(dy.cuda(), pre.cuda(), rows, cols, 1), pre.double() + ref, "accumulate = 1", scaled=True)
    over = _bias_grad_abi(dy.cuda(), pre.cuda(), rows, cols, 0)  # accumulate = 0 overwrites the same pre-fill
    _close(over, ref, "accumulate = 0", scaled=True)
    assert torch.equal(over, _bias_grad_abi(dy.cuda(), torch.empty(cols, device="cuda"), rows, cols, 0))


@pytest.mark.parametrize("cols", [4, 65])
def test_bias_grad_of_no_rows(cols):
    pre = torch.randn(cols, generator=torch.Generator().manual_seed(cols)).cuda()
    assert torch.equal(_bias_grad_abi(None, pre.clone(), 0, cols, 1), pre)  # nothing to add
    assert bool((_bias_grad_abi(None, pre.clone(), 0, cols, 0) == 0).all())   # an empty sum


@pytest.mark.parametrize("rows", [1, 300, 20000])
def test_bias_grad_scalar_path_of_a_4_byte_aligned_dy_is_bitwise_the_vector_path(rows):
    cols = 64
    dy = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows))
    want = _bias_grad_abi(dy.cuda(), torch.empty(cols, device="cuda"), rows, cols, 0)
    got = _bias_grad_abi(_offset_view(dy), torch.empty(cols, device="cuda"), rows, cols, 0)
    assert torch.equal(got, want)
    _close(got, dy.double().sum(0), "column sums", scaled=True)


# ---- D2. the workspace contracts of csa_bias_grad and csa_layernorm_bwd: guards, poison, written ----
# (tests/abi_arena.py; the method of tests/test_sbm_abi_guard_gpu.py: outputs and workspace carved at exactly the
# byte counts the size queries return, between guards, prefilled 0x00 and then 0xFF)

def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


@pytest.mark.parametrize("rows,cols", [(255, 65), (1, 4)])
def test_bias_grad_workspace_guards_poison_written(rows, cols):
    from abi_arena import POISON_ONES, POISON_ZERO, Arena
    from csa_amd._lib import check, lib
    L = lib()
    g = torch.Generator().manual_seed(rows + cols)
    dy = torch.randn(rows, cols, generator=g).cuda()
    pre = (torch.randn(cols, generator=g) * 10).cuda()
    dy0 = dy.clone()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = {}
    for poison in (POISON_ZERO, POISON_ONES):
        ar = Arena("cuda", capacity=1 << 20, poison=poison)
        db = ar.carve("db", shape=(cols,))
        acc = ar.carve("db_acc", shape=(cols,))
        ws = ar.carve("workspace", nbytes=L.csa_bias_grad_workspace_bytes(rows, cols))
        check(L.csa_bias_grad(_vp(dy), _vp(db), rows, cols, 0, _vp(ws), stream), "csa_bias_grad")
        ar.assert_guards_intact(f"bias_grad {rows}x{cols} accumulate=0")
        ar.fill("workspace", poison)
        acc.copy_(pre)
        check(L.csa_bias_grad(_vp(dy), _vp(acc), rows, cols, 1, _vp(ws), stream), "csa_bias_grad")
        ar.assert_guards_intact(f"bias_grad {rows}x{cols} accumulate=1")
        if poison == POISON_ONES:
            ar.assert_written(db, "db")
            ar.assert_written(acc, "db (accumulate)")
        runs[poison] = (db.cpu(), acc.cpu())
    assert all(_same_bits(a, b) for a, b in zip(runs[POISON_ZERO], runs[POISON_ONES])), "db depends on the workspace's old bytes"
    assert _same_bits(dy, dy0)
    assert torch.equal(runs[POISON_ONES][0], _bias_grad_abi(dy, torch.empty(cols, device="cuda"), rows, cols, 0).cpu())
    _close(runs[POISON_ONES][0], dy.double().sum(0).cpu(), "column sums", scaled=True)


@pytest.mark.parametrize("cols,cpl", [(252, 1), (260, 2), (516, 3), (772, 4)])
def test_layernorm_bwd_workspace_guards_poison_written(cols, cpl, monkeypatch):
    """One width per CPL whose last chunk is partial (LN_COLS), 33 rows (a partial group of 4, a partial workgroup of
    32): y, stats, dx, dgamma, dbeta and the workspace between guards; bitwise glue.LayerNorm on the same inputs."""
    from abi_arena import POISON_ONES, POISON_ZERO, Arena
    from csa_amd._lib import check, lib
    L = lib()
    assert (cols, cpl) in LN_COLS and ln_cpl(cols) == cpl and cols % 256
    rows = 33
    g = torch.Generator().manual_seed(1000 * rows + cols)
    x = torch.randn(rows, cols, generator=g) * 3 + 1
    w, b = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    gy = torch.randn(rows, cols, generator=g)
    inp = [t.cuda() for t in (x, w, b, gy)]
    xd, wd, bd, gyd = inp
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = {}
    for poison in (POISON_ZERO, POISON_ONES):
        ar = Arena("cuda", capacity=4 << 20, poison=poison)
        out = {"y": ar.carve("y", shape=(rows, cols), align=16), "stats": ar.carve("stats", shape=(rows, 2)),
               "dx": ar.carve("dx", shape=(rows, cols), align=16), "dgamma": ar.carve("dgamma", shape=(cols,)),
               "dbeta": ar.carve("dbeta", shape=(cols,))}
        ws = ar.carve("workspace", nbytes=L.csa_layernorm_bwd_workspace_bytes(rows, cols))
        check(L.csa_layernorm_fwd(_vp(xd), _vp(wd), _vp(bd), _vp(out["y"]), _vp(out["stats"]), rows, cols, 1e-5, stream),
              "csa_layernorm_fwd")
        ar.assert_guards_intact(f"layernorm fwd {rows}x{cols}")
        check(L.csa_layernorm_bwd(_vp(gyd), _vp(xd), _vp(out["stats"]), _vp(wd), _vp(out["dx"]), _vp(out["dgamma"]),
                                  _vp(out["dbeta"]), rows, cols, _vp(ws), stream), "csa_layernorm_bwd")
        ar.assert_guards_intact(f"layernorm bwd {rows}x{cols}")
        if poison == POISON_ONES:
            for n, t in out.items():
                ar.assert_written(t, n)
        runs[poison] = {n: t.cpu() for n, t in out.items()}
    for n in runs[POISON_ONES]:
        assert _same_bits(runs[POISON_ZERO][n], runs[POISON_ONES][n]), f"{n} depends on the buffers' old bytes"
    for t, h in zip(inp, (x, w, b, gy)):
        assert _same_bits(t, h)
    anchor = _ln_run(x, w, b, gy, monkeypatch)
    for n, t in zip(("y", "dx", "dgamma", "dbeta"), anchor):
        assert _same_bits(runs[POISON_ONES][n], t), f"{n} differs from glue.LayerNorm"


# ---- E. the scalar loads of the scan kernels ----

def _distinct_rows(rows, V, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(rows * V, generator=g).float() - rows * V / 2).view(rows, V)


def test_argmax_rows_on_a_4_byte_aligned_base():
    from csa_amd.decode_ops import argmax_rows
    rows, V = 3, 1024
    x = _distinct_rows(rows, V, 5)
    x[1, V - 1] = 1e9  # the last column of a row
    mx_a, mx_o = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    want = argmax_rows(x.cuda(), maxval=mx_a)
    got = argmax_rows(_offset_view(x), maxval=mx_o)
    assert torch.equal(got, want) and torch.equal(mx_o, mx_a)
    assert torch.equal(got.cpu(), x.double().argmax(1)) and torch.equal(mx_o.cpu().double(), x.double().max(1).values)


@pytest.mark.parametrize("W", [1, 4, 8])
def test_beam_row_topk_on_a_4_byte_aligned_base(W):
    from csa_amd.decode_ops import beam_row_topk
    rows, V = 3, 1024
    x = _distinct_rows(rows, V, 7 + W)
    for name, z in (("plain", x), ("small range", x / (rows * V) * 8)):  # the second: a sum of many comparable terms
        want = beam_row_topk(z.cuda(), W)
        got = beam_row_topk(_offset_view(z), W)
        for a, b in zip(got, want):
            assert torch.equal(a, b), name
        tv, ti = torch.topk(z.double(), W, dim=1)
        assert torch.equal(got[2].cpu().long(), ti) and torch.equal(got[1].cpu().double(), tv), name
        _close(got[0], torch.logsumexp(z.double(), 1), name + " lse", scaled=True)
