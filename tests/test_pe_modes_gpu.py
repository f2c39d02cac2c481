"""The structure-encoding ablations on the GPU: the batched Laplacian eigenvector kernel against fp64 invariants, the
tree positional encoding kernels against fp64 autograd, and the model in each mode against the reference's tiny
fixtures (tools/gen_golden.py pe)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pe_ref
from conftest import has_gpu
from golden_inputs import fill_params_deterministic

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]

TINY = dict(src_vocab_size=50, tgt_vocab_size=60, hidden_size=64, num_heads=8, num_layers=1, sbm_layers=2,
            dim_feed_forward=128, dropout=0.2, pe_dim=32, pegen_dim=128, sbm_enc_dim=512, clusters=[10, 12],
            full_att=False)
MODES = {"sequential": ("csatrans_tiny_seq", dict(pe_dim=0), 73), "treepos": ("csatrans_tiny_treepos", dict(pegen_dim=256), 74),
         "triplet": ("csatrans_tiny_triplet", {}, 75), "laplacian": ("csatrans_tiny_lap", {}, 76)}


# ---- the eigenvector kernel ----

def test_lap_pe_kernel_invariants():
    """One batch, N = 150, n = 1, 2, 3, 12, 37, 64, 65, 150 (odd n and the bye, n = 1, the wave-size boundary, the
    largest size), garbage ones outside each n x n block, against fp64 numpy of the reference's formula. With
    u = 2^-24 and |M|_2 < 3 a backward-stable fp32 solver allows a few n u |M|; the bounds are four times that
    (pe_ref.lap_bounds): residual and eigenvalues 12 n u, orthogonality 4 n u, projectors per eigenvalue cluster at gap
    1e-2 2 (12 n u) / 1e-2 (Davis-Kahan). Also the sign rule, exact zeros outside [:n, :n], status 0, two runs bitwise
    equal."""
    from csa_amd.pe_ops import lap_pe
    adj, nn_ = pe_ref.lap_batch()
    ref = pe_ref.lap_reference()
    dadj, dn = torch.from_numpy(adj.copy()).cuda(), torch.from_numpy(nn_).cuda()
    r = lap_pe(dadj, dn, 512, backend="device", check=True)
    assert r.pe.shape == (len(nn_), 150, 512) and r.pe.dtype == torch.float32
    assert not bool(r.status.any())
    print("sweeps", dict(zip((int(n) for n in nn_), r.sweeps.tolist())))
    pe_ref.check_lap_result(r.pe.cpu().numpy(), r.eigenvalues.cpu().numpy(), adj, nn_, ref)
    r2 = lap_pe(dadj.to(torch.uint8), dn.to(torch.int32), 512)  # uint8 adj, int32 counts, the default backend
    assert torch.equal(r.pe, r2.pe) and torch.equal(r.eigenvalues, r2.eigenvalues) and torch.equal(r.sweeps, r2.sweeps)


def test_lap_pe_kernel_small_n_and_narrow_pegen_dim(golden):
    """A second shape: N = 20, pegen_dim = 128 (the tiny model's), the adjacency of the reference fixture."""
    from csa_amd.pe_ops import lap_pe
    z = golden("csatrans_tiny_lap")
    adj, nn_ = z["adj"], z["num_node"]
    ref = []
    for b, n in enumerate(nn_):
        L = pe_ref.laplacian64(adj[b], int(n))
        ref.append((L,) + tuple(np.linalg.eigh(L)))
    r = lap_pe(torch.from_numpy(adj).cuda(), torch.from_numpy(nn_).cuda(), 128, backend="device", check=True)
    assert r.pe.shape == (2, 20, 128)
    pe_ref.check_lap_result(r.pe.cpu().numpy(), r.eigenvalues.cpu().numpy(), adj, nn_, ref)
    # N = pegen_dim, and an AST count of zero nodes, stay in bounds
    r = lap_pe(torch.from_numpy(adj).cuda(), torch.tensor([0, 20]).cuda(), 20, backend="device", check=True)
    assert r.pe.shape == (2, 20, 20) and not bool(r.pe[0].any()) and not bool(r.eigenvalues[0].any())
    L = pe_ref.laplacian64(adj[1], 20)
    pe_ref.check_lap_result(r.pe[1:].cpu().numpy(), r.eigenvalues[1:].cpu().numpy(), adj[1:], [20],
                            [(L,) + tuple(np.linalg.eigh(L))])


@pytest.mark.parametrize("N", [33, 64, 65, 128, 160, 161, 201])
def test_lap_pe_kernel_every_launch_class(N):
    """The kernel is instantiated per ceil(N / 8) (elements per lane of a pair's 8 lanes: 4, 8, 16, 20, 32) and the
    launch takes ceil(N / 16) waves: both sides of every boundary, up to the largest N the CU's LDS holds (201; 202 is
    refused), with n = N and an odd / even n below it. The same invariants and bounds as above."""
    from csa_amd._lib import lib
    from csa_amd.pe_ops import lap_pe
    assert lib().csa_lap_pe_supported(201, 201) and not lib().csa_lap_pe_supported(202, 256)
    assert not lib().csa_lap_pe_supported(150, 149)
    sizes = (N, N - 1, max(1, N // 2))
    adj, nn_ = pe_ref.lap_batch(N, sizes, 100 + N)
    ref = pe_ref.lap_reference(N, sizes, 100 + N)
    r = lap_pe(torch.from_numpy(adj.copy()).cuda(), torch.from_numpy(nn_).cuda(), 208, backend="device", check=True)
    print("sweeps", r.sweeps.tolist())
    pe_ref.check_lap_result(r.pe.cpu().numpy(), r.eigenvalues.cpu().numpy(), adj, nn_, ref)


# ---- the tree-position kernels ----

TP_CASES = [((1, 1), 1, True, False), ((1, 1), 2, True, False), ((1, 65), 4, True, False), ((1, 65), 1, False, False),
            ((3, 100), 2, True, True), ((3, 100), 4, True, False), ((64, 150), 1, True, False),
            ((64, 150), 2, True, False), ((64, 150), 4, True, False)]


@pytest.mark.parametrize("shape,F,binary,zero_p", TP_CASES)
def test_tree_pos_kernels_match_fp64_autograd(shape, F, binary, zero_p):
    """Forward to rtol 1e-6; dp within R u sum|terms| of fp64 (R rows; the worst case of an fp32 sum of R terms,
    computed in fp64 by pe_ref.tree_pos_reference64); two runs bitwise equal. One case has non-binary pos, one an
    exact p_f = 0 (w = 0 below depth 0, sqrt(d_model / 2) at depth 0, torch's pow gradients)."""
    from csa_amd.model import TreePositionalEncodings
    pos, p, dout = pe_ref.tree_pos_case(shape, F, seed=1000 * shape[1] + F, binary=binary, zero_p=zero_p)
    ref, dp64, bound = pe_ref.tree_pos_reference64(pos, p, dout)
    enc = TreePositionalEncodings(16, 8, F, 128 * F).cuda()
    with torch.no_grad():
        enc.p.copy_(p)
    runs = []
    for _ in range(2):
        enc.p.grad = None
        out = enc(pos.cuda())
        out.backward(dout.cuda())
        runs.append((out.detach().clone(), enc.p.grad.clone()))
    out, dp = runs[0]
    assert out.shape == shape + (128 * F,) and out.dtype == torch.float32
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=1e-6, atol=0)
    err = (dp.cpu().double() - dp64).abs()
    print("dp error", err.tolist(), "bound", bound.tolist())
    assert bool((err <= bound).all())
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    if zero_p:
        o = out.cpu().reshape(-1, 16, 8, F)
        q = pos.reshape(-1, 16, 8)
        assert bool((o[:, 1:, :, 0] == 0).all())
        assert torch.equal(o[:, 0, :, 0], q[:, 0] * torch.tensor(128 * F / 2).sqrt())


@pytest.mark.parametrize("shape,F,binary,zero_p", [c for c in TP_CASES if c[0] == (1, 65)])
def test_tree_pos_bwd_workspace_guards_poison_written(shape, F, binary, zero_p):
    """csa_tree_pos_bwd's workspace contract (tests/abi_arena.py, the method of tests/test_sbm_abi_guard_gpu.py) at the
    smallest TP_CASES row count with several row blocks (65 rows: two blocks of TP_BWD_ROWS = 64, the second with one
    row): out, dp and the workspace carved at exactly csa_tree_pos_bwd_workspace_bytes between guards, prefilled 0x00
    and 0xFF; dp bitwise equal either way and bitwise the module's."""
    import ctypes
    import os
    from abi_arena import POISON_ONES, POISON_ZERO, Arena
    from conftest import PKG
    from csa_amd._lib import check, lib
    from csa_amd.model import TreePositionalEncodings
    with open(os.path.join(PKG, "csrc", "csa_pe.hip")) as f:
        assert "constexpr int TP_BWD_ROWS = 64;" in f.read()
    L = lib()
    pos, p, dout = pe_ref.tree_pos_case(shape, F, seed=1000 * shape[1] + F, binary=binary, zero_p=zero_p)
    rows, depth, width = shape[0] * shape[1], 16, 8
    assert 64 < rows < 128
    inp = [t.reshape(rows, -1).contiguous().cuda() if t.dim() > 1 else t.cuda() for t in (pos, p, dout)]
    host = [t.cpu().clone() for t in inp]
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = {}
    for poison in (POISON_ZERO, POISON_ONES):
        ar = Arena("cuda", capacity=4 << 20, poison=poison)
        out = ar.carve("out", shape=(rows, depth * width * F), align=16)
        dp = ar.carve("dp", shape=(F,))
        ws = ar.carve("workspace", nbytes=L.csa_tree_pos_bwd_workspace_bytes(rows, depth, width, F))
        check(L.csa_tree_pos_fwd(vp(inp[0]), vp(inp[1]), vp(out), rows, depth, width, F, float(128 * F), stream),
              "csa_tree_pos_fwd")
        ar.assert_guards_intact("tree_pos fwd")
        check(L.csa_tree_pos_bwd(vp(inp[0]), vp(inp[1]), vp(inp[2]), vp(dp), rows, depth, width, F, float(128 * F), vp(ws),
                                 stream), "csa_tree_pos_bwd")
        ar.assert_guards_intact("tree_pos bwd")
        if poison == POISON_ONES:
            ar.assert_written(out, "out")
            ar.assert_written(dp, "dp")
        runs[poison] = (out.cpu(), dp.cpu())
    bits = lambda t: t.contiguous().view(torch.int32)
    for a, b in zip(runs[POISON_ZERO], runs[POISON_ONES]):
        assert torch.equal(bits(a), bits(b)), "the result depends on the buffers' old bytes"
    assert all(torch.equal(bits(t.cpu()), bits(h)) for t, h in zip(inp, host))
    enc = TreePositionalEncodings(16, 8, F, 128 * F).cuda()
    with torch.no_grad():
        enc.p.copy_(p)
    ref = enc(pos.cuda())
    ref.backward(dout.cuda())
    assert torch.equal(bits(ref.detach().cpu().reshape(rows, -1)), bits(runs[POISON_ONES][0]))
    assert torch.equal(bits(enc.p.grad.cpu()), bits(runs[POISON_ONES][1]))


# ---- the model ----

def _model_and_data(mode, z, tgt=True):
    from csa_amd.model import CSATrans
    name, over, seed = MODES[mode]
    m = CSATrans(**{**TINY, **over}, use_pegen=mode)
    fill_params_deterministic(m, seed)
    m = m.cuda().eval()
    c = lambda k, dt: torch.from_numpy(z[k]).to(dt).cuda()

    def data(**extra):
        """A fresh batch, and the fixture's uniforms armed for the next encode (SBMAttention consumes them)."""
        for i in range(2):
            getattr(m.SBM, f"transformer_{i}").mha.attn.uniforms = torch.from_numpy(z[f"u{i}"]).cuda()
        d = SimpleNamespace(src_seq=c("src_seq", torch.int64), tgt_seq=c("tgt_seq", torch.int64) if tgt else None,
                            num_node=c("num_node", torch.int32))
        for k, dt in (("tree_pos", torch.float32), ("triplet", torch.int64), ("adj", torch.uint8)):
            if k in z:
                setattr(d, k, c(k, dt))
        for k, v in extra.items():
            setattr(d, k, v)
        return d
    return m, data


@pytest.mark.parametrize("mode", list(MODES))
def test_mode_forward_backward_matches_reference(mode, golden):
    """Each mode against the reference CSATrans on identical weights, inputs and uniforms, at the tolerances of
    test_csatrans_forward_backward_matches_reference. The laplacian mode is fed the fixture's (LAPACK's)
    eigenvectors as data.lap_pe: inside a repeated eigenvalue's eigenspace no other solver reproduces them."""
    from csa_amd.model import label_smoothing_loss
    z = golden(MODES[mode][0])
    m, data = _model_and_data(mode, z)
    x = data(**({"lap_pe": torch.from_numpy(z["lap_vec"]).cuda()} if mode == "laplacian" else {}))
    out, sparsity, pe, graphs, attns = m(x)
    loss = label_smoothing_loss(out, torch.from_numpy(z["target"]).cuda())
    np.testing.assert_allclose(out.detach().cpu().numpy(), z["out"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(sparsity.item(), z["sparsity"][0], rtol=1e-6)
    np.testing.assert_allclose(loss.item(), z["loss"][0], rtol=1e-5)
    (loss + 1e-2 * sparsity).backward()
    named = dict(m.named_parameters())
    checked = set()
    for k in z:
        if k.startswith("g:"):
            np.testing.assert_allclose(named[k[2:]].grad.cpu().numpy(), z[k], rtol=1e-3, atol=2e-5, err_msg=k)
            checked.add(k[2:])
    assert len(checked) >= 10
    assert {"treepos": "tree_pos_enc.p", "triplet": "triplet_emb.weight"}.get(mode, "SBM.out.bias") in checked


def test_laplacian_mode_with_device_eigenvectors(golden):
    """Without data.lap_pe the eigenvectors come from the kernel: finite output of the right shape, bitwise the same
    twice (the kernel's own result is covered by the invariants above)."""
    z = golden("csatrans_tiny_lap")
    m, data = _model_and_data("laplacian", z)
    with torch.no_grad():
        a = m(data())[0]
        b = m(data())[0]
    assert a.shape == z["out"].shape and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)


def test_treepos_cached_greedy_matches_uncached(golden):
    """The generators need nothing mode-specific: CachedGreedyGenerator and GreedyGenerator give the same ids on a
    treepos model."""
    from csa_amd.model import CachedGreedyGenerator, GreedyGenerator
    z = golden("csatrans_tiny_treepos")
    m, data = _model_and_data("treepos", z, tgt=False)
    with torch.no_grad():
        m.generator.linear.weight.mul_(8.0)  # a spread-out generator, as the greedy fixture uses
        plain = GreedyGenerator(m, 7)(data())
    ys = CachedGreedyGenerator(m, 7)(data())
    assert ys.shape == plain.shape == (2, 6) and torch.equal(ys, plain)
