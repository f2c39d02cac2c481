"""The reference side of tests/test_sbm_rect_gpu.py (N queries, M != N keys), pinned on the CPU before any kernel is
blamed: the two oracles agree on every rectangular case (closed_form in fp64 on the fp32 op-for-op oracle's graph,
against sbm_ref + autograd); the conditions the GPU comparison relies on hold from the reference alone (at most 4
ReLU tie elements per case, a case with query rows that sample no edge, a case with a fully valid mask); the bf16
tolerance constants of the GPU file are at least 4 x the recomputed emulation budget; and the shared case builder
_rand_case is, for M = N, exactly the function it was before it took M."""
import numpy as np
import pytest
import torch

import test_sbm_rect_gpu as R
from oracle import closed_form, sbm_ref
from test_bf16_paths_gpu import PARAM_NAMES, tol_class
from test_sbm_gpu import ATOL, RTOL, _rand_case


def _close(a, r, name):
    np.testing.assert_allclose(a.detach().numpy(), r.detach().numpy(), rtol=RTOL, atol=ATOL, err_msg=name)


@pytest.fixture(scope="module")
def fp32_cases():
    return R.fp32_cases()


@pytest.fixture(scope="module")
def bf16_cases():
    return R.bf16_cases()


def test_the_two_oracles_agree_on_rectangular_sbm_cases(fp32_cases):
    """Eval, train (regenerated dropout masks over (N, M), rows = N | M) and map-gradient cases."""
    for label, c in fp32_cases:
        kw = c["kw"]
        B, H, N, d, k = c["shape"]
        M = kw["K"].shape[2]
        assert kw["mask"].shape == (B, M) and kw["u"].shape == (B, H, N, M) and kw["V"].shape == (B, H, M, d)
        if bool((kw["mask"].sum(1) == M).any()):
            continue  # an AST without a valid key is 0/0 in the reference
        q, kk, v = (kw[n].clone().requires_grad_(True) for n in ("Q", "K", "V"))
        params = {n: p.clone().requires_grad_(True) for n, p in kw["params"].items()}
        pk = {n: t.float() for n, t in kw.get("proj_keep", {}).items()} or None
        ak = kw["attn_keep"].float() if "attn_keep" in kw else None
        X, sp, graph, attn = sbm_ref.sbm_attention(q, kk, v, kw["mask"], params, kw["u"].float(), k, attn_keep=ak,
                                                   proj_keep=pk)
        assert graph.shape == attn.shape == (B, H, N, M)
        loss = (X * kw["dX"]).sum() + (sp * kw["dsparsity"]).sum()
        if "dgraph" in kw:
            loss = loss + (graph * kw["dgraph"]).sum() + (attn * kw["dattn"]).sum()
        loss.backward()
        ref, rg = closed_form.sbm_fwd_bwd(**kw, graph_override=graph.detach())
        _close(X, ref["X"], f"{label} X")
        _close(attn, ref["attn"], f"{label} attn")
        np.testing.assert_allclose(sp.detach().numpy(), ref["sparsity"].numpy(), rtol=1e-6)
        np.testing.assert_allclose(sp.detach().numpy(), graph.detach().sum((0, 2, 3)).numpy() / (B * N * M), rtol=1e-6)
        for name, t in (("Q", q), ("K", kk), ("V", v)):
            _close(t.grad, rg[name], f"{label} d{name}")
        for name in PARAM_NAMES:
            _close(params[name].grad, rg[name], f"{label} {name}")


def test_the_two_oracles_agree_on_rectangular_dense_cases():
    for shape in R.DENSE_SHAPES:
        c = R.rect_dense_case(shape)
        kw = c["kw"]
        B, H, N, M, d = shape
        assert kw["K"].shape == (B, H, M, d) and kw["mask"].shape == (B, M) and kw["dattn"].shape == (B, H, N, M)
        assert c["keep"].shape == (B, H, N, M)
        q, kk, v = (kw[n].clone().requires_grad_(True) for n in ("Q", "K", "V"))
        X, _, _, attn = sbm_ref.full_attention(q, kk, v, kw["mask"], attn_keep=kw["attn_keep"].float())
        ((X * kw["dX"]).sum() + (attn * kw["dattn"]).sum()).backward()
        ref, rg = closed_form.dense_fwd_bwd(**kw)
        _close(X, ref["X"], f"dense{shape} X")
        _close(attn, ref["attn"], f"dense{shape} attn")
        for name, t in (("Q", q), ("K", kk), ("V", v)):
            _close(t.grad, rg[name], f"dense{shape} d{name}")


def test_conditions_of_the_gpu_comparison_hold_from_the_reference_alone(fp32_cases, bf16_cases):
    """At most 4 ReLU tie elements in every case (the rule of _match_oracle_up_to_relu_ties; bf16 cases under the
    bf16-rounded operands), a case with a query row that samples no edge, a case with a fully valid mask."""
    no_edge = full_mask = 0
    for bf16, cases in ((False, fp32_cases), (True, bf16_cases)):
        for label, c in cases:
            kw = c["kw"]
            if "params" not in kw:
                continue
            out, _ = closed_form.sbm_fwd_bwd(**kw, bf16=bf16)
            assert len(out["relu_ties"]) <= 4, (label, bf16, out["relu_ties"][:8])
            assert 0 < float(out["graph"].mean()) < 1, label
            no_edge += int((out["graph"].sum(-1) == 0).sum())
            full_mask += int(bool((kw["mask"] == 0).all()))
    assert no_edge > 0 and full_mask > 0, (no_edge, full_mask)


def test_rect_bf16_tolerances_cover_four_times_the_recomputed_budget(bf16_cases):
    import test_bf16_paths_gpu as T
    assert set(R.TOL) == set(T.TOL)
    assert all(R.TOL[n] >= max(T.TOL[n], T.FLOOR) for n in T.TOL)
    assert R.TOL["X"] <= 5e-3 and R.TOL["dQKV"] <= 5e-3
    n = 0
    for label, c in bf16_cases:
        kw = c["kw"]
        if max(kw["Q"].shape[2], kw["K"].shape[2]) > 150:
            continue
        n += 1
        for name, (m, f) in closed_form.emulation_budget(kw).items():
            tol = R.TOL[tol_class(name)]
            print(f"budget {label} {name}: element metric {m:.3g} Frobenius {f:.3g}")
            assert tol >= 4 * max(m, f), (label, name, m, f, tol)
    assert n == 7


def _rand_case_before_m(B, H, N, d, k, seed, pad=True):
    """A frozen copy of test_sbm_gpu._rand_case as it was before it took M."""
    g = torch.Generator().manual_seed(seed)
    Q, K, V = (torch.randn(B, H, N, d, generator=g) for _ in range(3))
    mask = torch.zeros(B, N)
    if pad:
        for b in range(B):
            n = int(torch.randint(max(1, N // 3), N + 1, (1,), generator=g))
            mask[b, n:] = 1.0
    u = torch.rand(B, H, N, N, generator=g)
    dX = torch.randn(B, H, N, d, generator=g)
    dsp = torch.full((H,), 3.125e-4)
    params = {"layer.weight": torch.nn.init.orthogonal_(torch.empty(H * k, d), generator=g)}
    for i in (0, 3, 6):
        params[f"proj.{i}.weight"] = torch.nn.init.xavier_uniform_(torch.empty(d, d), generator=g)
        params[f"proj.{i}.bias"] = 0.1 * torch.randn(d, generator=g)
    return Q, K, V, mask, u, dX, dsp, params


@pytest.mark.parametrize("shape,pad", [((2, 2, 45, 64, 5), True), ((1, 3, 150, 96, 20), True), ((2, 2, 37, 64, 10), False)])
def test_rand_case_is_unchanged_for_square_shapes(shape, pad):
    B, H, N, d, k = shape
    old = _rand_case_before_m(B, H, N, d, k, seed=sum(shape), pad=pad)
    for new in (_rand_case(B, H, N, d, k, seed=sum(shape), pad=pad), _rand_case(B, H, N, d, k, seed=sum(shape), pad=pad, M=N)):
        for a, b in zip(old[:7], new[:7]):
            assert a.shape == b.shape and torch.equal(a, b)
        assert list(old[7]) == list(new[7]) and all(torch.equal(old[7][n], new[7][n]) for n in old[7])
    # dense_case drew Q, K, V, dX as four tensors of one shape from one generator, then the default mask on N
    g = torch.Generator().manual_seed(sum(shape))
    old_dense = [torch.randn(B, H, N, d, generator=g) for _ in range(4)]
    kw = R.dense_case((B, H, N, d), seed=sum(shape))["kw"]
    assert all(torch.equal(a, kw[n]) for a, n in zip(old_dense, ("Q", "K", "V", "dX")))
    old_mask = torch.zeros(B, N)
    old_mask[B - 1, N - N // 4:] = 1.0
    assert torch.equal(kw["mask"], old_mask)
    Q, K, V, mask, u, dX, _, _ = _rand_case(B, H, N, d, k, seed=1, M=N + 7)
    assert K.shape == V.shape == (B, H, N + 7, d) and mask.shape == (B, N + 7) and u.shape == (B, H, N, N + 7)
    assert Q.shape == dX.shape == (B, H, N, d)
