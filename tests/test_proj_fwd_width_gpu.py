"""The projection forward's cluster products at their true width (k_proj_fwd_l W16, fp32 with k <= 16:
sigmoid(C p^T) on the 16x16x1 four-block MFMA, T = Kh S^T on the 16x16x4 MFMA, lanes16 fragments from k_prep)
against the fp64 closed form.

Shapes: the cluster mask (k = 1, 4, 5, 10, 15, 16: one cluster, a full lane group of 4, a mask inside a lane
group, the headline k, one dead cluster, none), the row halves of a 32-row item (N = 17: a single row in the second
half; N = 33 / 45 / 47 / 49: partial last items on both sides of the half), H >= 2 so a wrong head's C or S fragment
shows, k = 17 (kp = 32: the 32-wide path must still be taken) and d = 96. Inputs are test_sbm_gpu._rand_case with
padding: non-zero biases that differ per feature, valid lengths that differ per AST.

The sampling depends on hat: each case first asserts, on the oracle alone, that at least 90 % of expA lies
strictly inside (0.01, 0.99), so a wrong hat moves the sampled graph and not only the clamped tails.
"""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from oracle import closed_form
from test_sbm_gpu import ATOL, RTOL, _match_oracle_up_to_relu_ties, _rand_case, _run_module

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]

# (B, H, N, d, k); _rand_case seeds sum(shape) (eval) and 3 * sum(shape) (train) meet the expA condition and the
# ReLU-tie cap on the CPU oracle alone: 100 % inside, no tie, edge rates 0.21 .. 0.25
SHAPES = [(2, 2, 17, 64, 1), (2, 2, 33, 64, 4), (2, 2, 45, 64, 5), (2, 3, 49, 64, 10), (2, 2, 64, 64, 15),
          (2, 2, 33, 64, 16), (1, 2, 40, 64, 17), (2, 2, 33, 96, 10), (1, 2, 47, 96, 16)]
TRAIN_SHAPES = [(2, 2, 45, 64, 16), (1, 2, 33, 96, 10)]


def _inside(expA):
    """Fraction of expA strictly inside the clamp range (0.01, 0.99)."""
    e = expA.double()
    return float(((e > 0.01) & (e < 0.99)).double().mean())


def _check_eval(shape, got, inputs):
    Q, K, V, mask, u, dX, dsp, params = inputs
    k = shape[4]
    X, sp, graph, dQ, dK, dV, grads = got

    def run_oracle(ov):
        out, rg = closed_form.sbm_fwd_bwd(Q, K, V, mask, params, u, k, dX, dsp, graph_override=graph, relu_override=ov)
        return out, rg

    def check(ref, rg):
        inside = _inside(ref["expA"])
        print(f"proj-fwd-width {shape}: expA inside (0.01, 0.99): {inside:.4f}")
        assert inside >= 0.9, f"only {inside:.3f} of expA inside (0.01, 0.99): the case does not test the sampling"
        own = (u < ref["expA"].clamp(0.01, 0.99))
        near = (torch.abs(u - ref["expA"].clamp(0.01, 0.99)) < 1e-6)
        diff = graph.bool() != own
        print(f"proj-fwd-width {shape}: {int(diff.sum())} graph flips, edge rate {float(graph.mean()):.3f}")
        assert bool(torch.all(near[diff])), "graph flips away from fp32 ties"
        np.testing.assert_allclose(X.numpy(), ref["X"].numpy(), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(sp.numpy(), ref["sparsity"].numpy(), rtol=1e-6)
        for name, t, key in (("dQ", dQ, "Q"), ("dK", dK, "K"), ("dV", dV, "V")):
            np.testing.assert_allclose(t.numpy(), rg[key].numpy(), rtol=RTOL, atol=ATOL, err_msg=name)
        for pn, gv in grads.items():
            if pn.startswith("orth_clusters"):
                continue
            np.testing.assert_allclose(gv.numpy(), rg[pn].numpy(), rtol=RTOL, atol=ATOL, err_msg=pn)

    nt = _match_oracle_up_to_relu_ties(run_oracle, check)
    print(f"proj-fwd-width {shape}: {nt} ReLU tie element(s)")


@pytest.mark.parametrize("shape", SHAPES)
def test_proj_fwd_width_shapes_vs_oracle(shape):
    """Graph (flips at sampling ties only), X, sparsity, dQ / dK / dV and every parameter gradient at the fp32
    suite's tolerance, under the ReLU-tie rule."""
    B, H, N, d, k = shape
    inputs = _rand_case(B, H, N, d, k, seed=sum(shape), pad=True)
    Q, K, V, mask, u, dX, dsp, params = inputs
    _check_eval(shape, _run_module(Q, K, V, mask, u, dX, dsp, params, k), inputs)


def test_proj_fwd_width_deterministic():
    """Two runs of one case are bit-identical (forward outputs and every gradient)."""
    shape = (2, 3, 49, 64, 10)
    B, H, N, d, k = shape
    Q, K, V, mask, u, dX, dsp, params = _rand_case(B, H, N, d, k, seed=sum(shape), pad=True)
    a = _run_module(Q, K, V, mask, u, dX, dsp, params, k)
    b = _run_module(Q, K, V, mask, u, dX, dsp, params, k)
    for x, y in zip(a[:6], b[:6]):
        assert torch.equal(x, y)
    for n in a[6]:
        assert torch.equal(a[6][n], b[6][n]), n


@pytest.mark.parametrize("shape", TRAIN_SHAPES)
def test_proj_fwd_width_train_mode_matches_oracle_with_regenerated_masks(shape):
    """Train mode (attention dropout 0.2, projection dropout 0.1): the bias meets dropout and ReLU in the
    reference's order, Linear -> Dropout -> ReLU. The oracle regenerates the kernels' Philox streams
    (test_sbm_gpu.test_train_mode_matches_oracle_with_regenerated_masks)."""
    from oracle import philox
    B, H, N, d, k = shape
    Q, K, V, mask, _, dX, dsp, params = _rand_case(B, H, N, d, k, seed=3 * sum(shape), pad=True)
    seed, offset, attn_p, proj_p = (0x1234567 << 32) | 0x89ABCDE, 77, 0.2, 0.1
    cw = params["layer.weight"].cuda()
    pw = [params[f"proj.{i}.weight"].cuda() for i in (0, 3, 6)]
    pb = [params[f"proj.{i}.bias"].cuda() for i in (0, 3, 6)]
    q, kk, v, mk = Q.cuda(), K.cuda(), V.cuda(), mask.cuda()
    X, sp, state = torch.ops.csa.sbm_fwd(q, kk, v, mk, cw, pw, pb, None, k, seed, offset, attn_p, proj_p, False)
    graph, _ = torch.ops.csa.sbm_maps(q, kk, v, mk, state, k, False)
    g = torch.ops.csa.sbm_bwd(q, kk, v, mk, cw, pw, pb, k, attn_p, proj_p, seed, offset, False, state, X,
                              dX.cuda(), dsp.cuda(), None)
    torch.cuda.synchronize()
    graph = graph.cpu()
    keep = philox.attn_keep(B, H, N, N, seed, offset, attn_p)
    ks = 1.0 / (1.0 - np.float32(proj_p))
    pk = {f"{s}{l}": torch.from_numpy(philox.proj_keep(B, H, N, d, seed, offset, proj_p, l, int(s == "k")) * ks)
          for s in "qk" for l in (0, 1)}
    u16 = philox.attn_uniforms(B, H, N, N, seed, offset, philox.RNG_STE)
    names = ["Q", "K", "V", "layer.weight", "proj.0.weight", "proj.0.bias", "proj.3.weight", "proj.3.bias",
             "proj.6.weight", "proj.6.bias"]

    def run_oracle(ov):
        return closed_form.sbm_fwd_bwd(Q, K, V, mask, params, None, k, dX, dsp,
                                       attn_keep=torch.from_numpy(keep / (1.0 - np.float32(attn_p))), proj_keep=pk,
                                       graph_override=graph, relu_override=ov)

    def check(ref, rg):
        inside = _inside(ref["expA"])
        print(f"proj-fwd-width train {shape}: expA inside (0.01, 0.99): {inside:.4f}")
        assert inside >= 0.9
        want = philox.ste_graph(ref["expA"].numpy(), u16)
        thr = np.clip(ref["expA"].numpy(), 0.01, 0.99) * 65536.0
        diff = want != graph.numpy().astype(bool)
        assert np.all(np.abs(u16[diff] - thr[diff]) < 0.5), f"{int(diff.sum())} graph flips away from ties"
        assert diff.mean() < 1e-4
        np.testing.assert_allclose(X.cpu().numpy(), ref["X"].numpy(), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(sp.cpu().numpy(), ref["sparsity"].numpy(), rtol=1e-6)
        for name, t in zip(names, g):
            np.testing.assert_allclose(t.cpu().numpy(), rg[name].numpy(), rtol=RTOL, atol=ATOL, err_msg=name)

    _match_oracle_up_to_relu_ties(run_oracle, check)


def test_proj_fwd_width_bf16_mode_matches_emulation():
    """bf16 mode keeps the 32-wide cluster products, so k_prep must still lay out the 32-row C and S fragments
    for it in the slots the fp32 kernels now fill with the lanes16 ones. One eval run at the operand-exact
    emulation's tolerances (test_bf16_paths_gpu)."""
    from test_bf16_paths_gpu import PARAM_NAMES, check_sbm, eval_case
    shape = (2, 2, 45, 64, 10)
    c = eval_case(shape)
    kw = c["kw"]
    X, sp, graph, dQ, dK, dV, grads = _run_module(kw["Q"], kw["K"], kw["V"], kw["mask"], kw["u"], kw["dX"],
                                                  kw["dsparsity"], kw["params"], kw["num_clusters"], bf16=True)
    got = {"X": X, "sparsity": sp, "graph": graph, "Q": dQ, "K": dK, "V": dV}
    got.update({n: grads[n] for n in PARAM_NAMES})
    check_sbm(c, got, f"eval{shape}")
