"""bf16 mode (CSA_DTYPE_BF16): the N^2 attention contractions and the cluster projection (proj MLP and
.C^T, forward and backward) on v_mfma_f32_32x32x16_bf16 vs the reference's fp32 golden vectors, at the
north_star bf16 tolerance 2e-2. Per tensor: every element within 2e-2 relative + 2e-2 of the tensor's
largest magnitude (and, as a gross-error guard, a relative Frobenius error below 5e-2: small parameter
gradients such as the cluster embeddings' sum many cancelling bf16-rounded terms).

The bf16 projection moves expA by ~1e-2, so the sampled graph differs from the fp32 one beyond fp32 ties.
The comparisons against the fp32 golden therefore run on the reference's own graph, forced through the
host-supplied uniforms (u = 0 where the reference sampled an edge, u = 0.995 where it did not: every
clamp(expA) lies in [0.01, 0.99]), and a separate check compares the bf16 mode's sampling with the fp32
mode's on the same uniforms (edge rate and agreement). A last check makes sure the bf16 path really ran.

These 2e-2-against-fp32 tests are the north-star ACCEPTANCE bar of bf16 mode (is bf16 mode close enough to the
reference to be used). They run eval mode on a forced graph only and cannot see a wrong tile. The CORRECTNESS bar
(does every bf16 kernel instantiation compute what it is designed to compute: train mode, dropout, map gradients,
dead key tiles, degenerate rows, long ASTs, schedules, dense) is tests/test_bf16_paths_gpu.py, which compares
with the operand-exact emulation oracle/closed_form.py (bf16=True) at a tolerance one to two orders tighter."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]
TOL = 2e-2


def close_bf16(got, ref, name, tol=TOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), 1e-30)
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * scale, err_msg=name)
    rel = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
    assert rel < 5e-2, f"{name}: relative Frobenius error {rel:.3g}"
    return rel


def dev(x, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().requires_grad_(grad)


def elem_metric(got, ref):
    """The smallest tol with |got - ref| <= tol |ref| + tol max|ref| element-wise (close_bf16's test)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (np.abs(ref) + max(float(np.abs(ref).max()), 1e-30))).max())


def fro(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def forced_uniforms(graph):
    """Uniforms that make u < clamp(p, .01, .99) reproduce `graph` for ANY p (STE.py:11-13)."""
    return np.where(np.asarray(graph) > 0, 0.0, 0.995).astype(np.float32)


@pytest.mark.parametrize("case", ["sbm_n37", "sbm_n150", "sbm_n33_d96", "sbm_n7_d96_k16", "sbm_n64_noncontig"])
def test_sbm_bf16_matches_reference_within_2e2(golden, case):
    from csa_amd.module.sbm_attn import SBMAttention
    z = golden(case)
    B, H, N, d, k = (int(v) for v in z["meta"])
    m = SBMAttention({"attention_dropout": 0.2, "head_dim": d, "num_head": H, "num_clusters": [k],
                      "attn_precision": "bf16"}, 0)
    m.load_state_dict({kk[2:]: torch.from_numpy(v) for kk, v in z.items() if kk.startswith("p:")}, strict=False)
    m = m.cuda().eval()
    Q, K, V = dev(z["Q"], True), dev(z["K"], True), dev(z["V"], True)
    m.uniforms = dev(forced_uniforms(z["graph"]))
    X, sp, graph, attn = m(Q, K, V, dev(z["mask"]))
    assert np.array_equal(graph.detach().cpu().numpy().astype(np.uint8), z["graph"].astype(np.uint8))
    close_bf16(X.detach().cpu().numpy(), z["X"], "X")
    ((X * dev(z["dX"])).sum() + (sp * dev(z["dsparsity"])).sum()).backward()
    for name, t in (("dQ", Q), ("dK", K), ("dV", V)):
        close_bf16(t.grad.cpu().numpy(), z[name], name)
    # Parameter gradients: 2e-2 is not reachable for ANY bf16-operand implementation here. The fp64 closed
    # form with exactly the bf16 mode's operands rounded to bf16 (oracle/closed_form.py, bf16=True: an ideal
    # bf16 implementation, exact accumulation) lands up to 0.03-0.30 of scale from the fp32 reference on the
    # MLP weight gradients: relu masks of pre-activations near 0 flip under bf16 inputs, and proj.0 / proj.3
    # are batch sums of the flipped rows. So each parameter gradient must meet 2e-2, or stay within 2x that
    # ideal implementation's own error (element-wise metric below, and relative Frobenius error).
    from oracle import closed_form
    t_ = lambda n: torch.from_numpy(np.ascontiguousarray(z[n]))
    params = {kk[2:]: torch.from_numpy(v) for kk, v in z.items() if kk.startswith("p:")}
    _, ge = closed_form.sbm_fwd_bwd(t_("Q"), t_("K"), t_("V"), t_("mask"), params, t_("u"), k, t_("dX"),
                                    t_("dsparsity"), graph_override=torch.from_numpy(z["graph"]).double(), bf16=True)
    for pn, p in m.named_parameters():
        ref = z["g:" + pn]
        got = p.grad.cpu().numpy()
        emu = ge[pn].numpy()
        m_got, m_emu = elem_metric(got, ref), elem_metric(emu, ref)
        f_got, f_emu = fro(got, ref), fro(emu, ref)
        print(f"bf16 {case} {pn}: element metric GPU {m_got:.4f} ideal-bf16 {m_emu:.4f}; Frobenius GPU {f_got:.4f}"
              f" ideal-bf16 {f_emu:.4f}")
        assert m_got <= max(TOL, 2 * m_emu), (pn, m_got, m_emu)
        assert f_got <= max(TOL, 2 * f_emu), (pn, f_got, f_emu)


@pytest.mark.parametrize("case", ["full_n37", "full_n150"])
def test_full_attention_bf16_matches_reference_within_2e2(golden, case):
    from csa_amd.module.sbm_attn import FullAttention
    z = golden(case)
    B, H, N, d = (int(v) for v in z["meta"])
    m = FullAttention({"attention_dropout": 0.2, "head_dim": d, "num_head": H, "attn_precision": "bf16"}, 0)
    m = m.cuda().eval()
    Q, K, V = dev(z["Q"], True), dev(z["K"], True), dev(z["V"], True)
    X, _, _, _ = m(Q, K, V, dev(z["mask"]))
    close_bf16(X.detach().cpu().numpy(), z["X"], "X")
    (X * dev(z["dX"])).sum().backward()
    for name, t in (("dQ", Q), ("dK", K), ("dV", V)):
        close_bf16(t.grad.cpu().numpy(), z[name], name)


def _rel_case(golden, case):
    z = golden(case)
    if "q" in z:
        return z, (z["q"], z["k"], z["v"], z["lq"], z["lk"], z["dO"])
    import golden_inputs as gi
    B, H, N, dk, L, seed = (int(v) for v in z["meta"])
    return z, gi.rel_inputs(B, H, N, dk, L, seed)


@pytest.mark.parametrize("case", ["rel_attn_n20_dk64", "rel_attn_n150_dk64"])
def test_rel_attn_bf16_matches_reference_within_2e2(golden, case):
    from csa_amd import rel_ops
    z, (qn, kn, vn, lqn, lkn, dOn) = _rel_case(golden, case)
    rel = dev(np.stack([z["L"], z["T"]], 1).astype(np.uint8))
    mask = dev(np.stack([z["L_mask"], z["T_mask"]], 1).astype(np.uint8))
    q, k, v, lq, lk = (dev(a, True) for a in (qn, kn, vn, lqn, lkn))
    o = rel_ops.rel_attn(q, k, v, lq, lk, rel, mask, bf16=True)
    close_bf16(o.detach().cpu().numpy(), z["out"], "out")
    (o * dev(dOn)).sum().backward()
    for n, x in (("dq", q), ("dk", k), ("dv", v), ("dlq", lq), ("dlk", lk)):
        close_bf16(x.grad.cpu().numpy(), z[n], n)


def test_bf16_sampling_matches_fp32_sampling_statistically():
    """With the same host-supplied uniforms, the bf16 projection's expA samples the same graph as the fp32
    path up to the draws that fall between the two expA values: head-wise sparsity within 1% (relative)
    and at least 97% of the edges identical (B=16, N=150, k=10, python dims)."""
    from test_sbm_gpu import _rand_case
    from csa_amd import ops
    B, H, N, d, k = 16, 8, 150, 64, 10
    Q, K, V, mask, u, dX, dsp, params = _rand_case(B, H, N, d, k, seed=21, pad=False)
    proj = [params[f"proj.{i}.{w}"].cuda() for i in (0, 3, 6) for w in ("weight", "bias")]
    res = {}
    for bf in (False, True):
        X, sp, graph, _ = ops.sbm_attention(Q.cuda(), K.cuda(), V.cuda(), mask.cuda(), params["layer.weight"].cuda(),
                                            proj, k, uniforms=u.cuda(), want_maps=True, bf16=bf)
        res[bf] = (sp.cpu().numpy(), graph.cpu().numpy())
    sp32, g32 = res[False]
    sp16, g16 = res[True]
    np.testing.assert_allclose(sp16, sp32, rtol=1e-2)
    agree = float((g16 == g32).mean())
    assert agree >= 0.97, agree
    assert agree < 1.0, "bf16 projection did not change a single sampled edge: did the bf16 path run?"


def test_bf16_path_really_runs_and_is_deterministic():
    """bf16 results differ from fp32 ones (the bf16 kernels ran) and repeat bitwise."""
    from test_sbm_gpu import _rand_case
    from csa_amd import ops
    B, H, N, d, k = 2, 8, 150, 64, 10
    Q, K, V, mask, u, dX, dsp, params = _rand_case(B, H, N, d, k, seed=5)
    proj = [params[f"proj.{i}.{w}"].cuda() for i in (0, 3, 6) for w in ("weight", "bias")]
    outs = {}
    uu = u.cuda()
    for mode in ("f32", "bf16", "bf16b"):
        q, kk, v = (t.cuda().requires_grad_(True) for t in (Q, K, V))
        X, sp, graph, _ = ops.sbm_attention(q, kk, v, mask.cuda(), params["layer.weight"].cuda(), proj, k, uniforms=uu,
                                            want_maps=True, bf16=mode != "f32")
        torch.autograd.backward([X, sp], [dX.cuda(), dsp.cuda()])
        outs[mode] = [X.detach().cpu(), q.grad.cpu(), kk.grad.cpu(), v.grad.cpu()]
        if mode == "f32":  # the bf16 runs sample the fp32 run's graph (compare like with like)
            uu = torch.from_numpy(forced_uniforms(graph.detach().cpu().numpy())).cuda()
    for a, b in zip(outs["bf16"], outs["bf16b"]):
        assert torch.equal(a, b)
    assert not torch.equal(outs["f32"][0], outs["bf16"][0])
    for a, b in zip(outs["bf16"], outs["f32"]):
        close_bf16(a.numpy(), b.numpy(), "bf16 vs f32")
