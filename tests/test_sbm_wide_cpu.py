"""The reference side of tests/test_sbm_wide_gpu.py (train mode, map gradients, dead key tiles and host uniforms in the
fp32 SBM launch classes with k > 16), pinned on the CPU before any kernel is blamed:

  * the two oracles agree on every case (closed_form in fp64 on the fp32 op-for-op oracle's graph, against sbm_ref +
    autograd under the regenerated attn_keep / proj_keep) at the fp32 suite's 1e-4 / 1e-5;
  * the conditions the GPU comparison relies on hold from the reference alone: at most 4 ReLU tie elements per case,
    0 < graph.mean() < 1, near-tie draws (a 16-bit draw within 0.5 of 65536 clamp(expA); a host uniform within 1e-6 of
    clamp(expA)) at or below floor(1e-4 draws), so an honest kernel cannot trip the graph rule's cap and a wrong one
    cannot hide in it, and the dead-tile cases sample edges past key 64;
  * the comparison is decisive: on the graph of the first train case of class B, C, D and F, the oracle rerun with
    one dropout mask wrong (the q0 and q1 projection masks swapped, two rows of k1 swapped, every projection mask set
    to one, the attention keep mask rolled by one key) leaves 1e-4 / 1e-5 on more than 1% of the elements of a tensor
    the GPU test compares;
  * the case lists cover every class x mode pair (test_sbm_wide_gpu.assert_every_class_and_mode_is_covered).

Two things the decisiveness runs record. On a fixed graph X does not see the projection masks at all (they act
through expA, that is through the sampled graph, and through the gradients of the MLPs), and an error in two rows of
a projection mask flips next to no sampled draw at these sizes. So the parameter gradients carry the check of the
projection dropout: a case list that dropped them would be blind there. The test prints, per class and wrong mask,
the share of each tensor's elements that leaves the tolerance (layer.weight: 98-100% in all 16 runs; proj.*: 84-100%, but
37-86% for the two swapped k1 rows at k = 100, the narrowest error over the widest cluster product), and the number of
draws the oracle's own sampling flips under the two swapped rows (5 and 1 of 12150 in classes B and F, 0 of 8100 and
0 of 4050 in C and D: far too few for the graph rule to notice).

Every figure here comes from the CPU oracles; none from GPU output."""
import numpy as np
import pytest
import torch

import test_sbm_wide_gpu as W
from oracle import closed_form, sbm_ref
from test_bf16_paths_gpu import PARAM_NAMES
from test_sbm_gpu import ATOL, RTOL

COMPARED = ["X", "Q", "K", "V"] + PARAM_NAMES  # what check_fp32 compares in a train-mode test without maps


def _close(a, r, name):
    np.testing.assert_allclose(a.detach().numpy(), r.detach().numpy(), rtol=RTOL, atol=ATOL, err_msg=name)


@pytest.fixture(scope="module")
def wide_cases():
    """(label, mode, case, closed_form's (out, grads) on its own sampling) of every case of the GPU file."""
    return [(label, mode, c, closed_form.sbm_fwd_bwd(**c["kw"])) for label, mode, c in W.wide_cases()]


def test_wide_case_lists_cover_every_launch_class_and_mode():
    W.assert_every_class_and_mode_is_covered()


def test_the_two_oracles_agree_on_the_wide_sbm_cases(wide_cases):
    assert len(wide_cases) == 30
    for label, mode, c, own in wide_cases:
        kw = c["kw"]
        B, H, N, d, k = c["shape"]
        M = kw["K"].shape[2]
        assert kw["mask"].shape == (B, M) and kw["u"].shape == (B, H, N, M) and kw["V"].shape == (B, H, M, d)
        assert bool((kw["mask"].sum(1) < M).all()), label  # every AST has a valid key: nothing is left out
        assert ("attn_keep" in kw) == c["train"] and ("proj_keep" in kw) == (c["proj_p"] > 0)
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
        graph = graph.detach()
        same = torch.equal(graph.double(), own[0]["graph"])  # then closed_form's own run is the run on this graph
        ref, rg = own if same else closed_form.sbm_fwd_bwd(**kw, graph_override=graph)
        _close(X, ref["X"], f"{label} X")
        _close(attn, ref["attn"], f"{label} attn")
        np.testing.assert_allclose(sp.detach().numpy(), ref["sparsity"].numpy(), rtol=1e-6)
        np.testing.assert_allclose(sp.detach().numpy(), graph.sum((0, 2, 3)).numpy() / (B * N * M), rtol=1e-6)
        for name, t in (("Q", q), ("K", kk), ("V", v)):
            _close(t.grad, rg[name], f"{label} d{name}")
        for name in PARAM_NAMES:
            _close(params[name].grad, rg[name], f"{label} {name}")


def test_conditions_of_the_gpu_comparison_hold_from_the_reference_alone(wide_cases):
    seen = set()
    for label, mode, c, (out, _) in wide_cases:
        kw = c["kw"]
        assert len(out["relu_ties"]) <= 4, (label, out["relu_ties"][:8])
        assert 0 < float(out["graph"].mean()) < 1, label
        p = out["expA"].clamp(0.01, 0.99).numpy()
        if c["train"] and not c.get("host_uniforms"):
            near = np.abs(c["u16"].astype(np.float64) - 65536.0 * p) < 0.5
        else:
            assert kw["u"].dtype == torch.float32  # the host draws, as the kernel reads them
            near = np.abs(kw["u"].double().numpy() - p) < 1e-6
        cap = int(np.floor(1e-4 * near.size))
        print(f"wide {label}: {len(out['relu_ties'])} ReLU tie element(s), {int(near.sum())} of {near.size} near-tie "
              f"draws (cap {cap})")
        assert int(near.sum()) <= cap, (label, int(near.sum()), near.size)
        if mode.startswith("dead"):
            assert float(out["graph"][:, :, :, 64:].sum()) > 0, label
            assert bool((kw["mask"][:, 64:96] == 1).all(1).any()), label  # a fully masked key tile
        seen.add(mode)
    assert seen == {"train", "proj0", "maps eval", "maps train", "dead eval", "dead train", "host-u"}


def _wrong_masks(kw):
    """(name, keyword arguments with one dropout mask wrong)."""
    pk = kw["proj_keep"]
    k1 = pk["k1"].clone()
    k1[:, :, [0, 1]] = pk["k1"][:, :, [1, 0]]
    assert not torch.equal(k1, pk["k1"])
    return [("q0 and q1 swapped", dict(kw, proj_keep=dict(pk, q0=pk["q1"], q1=pk["q0"]))),
            ("two rows of k1 swapped", dict(kw, proj_keep=dict(pk, k1=k1))),
            ("projection masks all one", dict(kw, proj_keep={n: torch.ones_like(t) for n, t in pk.items()})),
            ("attention keep rolled by one key", dict(kw, attn_keep=kw["attn_keep"].roll(1, -1)))]


def test_a_wrong_dropout_mask_leaves_the_tolerance_in_every_class(wide_cases):
    """Decisiveness of the train-mode comparison, from the oracle alone."""
    first = {f"train{s}": W.launch_class(s[4], s[5]) for s in W.FIRST_SHAPES}
    done = []
    for label, mode, c, (out, g) in wide_cases:
        if label not in first:
            continue
        kw = c["kw"]
        ref = dict(g, X=out["X"])
        for name, kw2 in _wrong_masks(kw):
            out2, g2 = closed_form.sbm_fwd_bwd(**kw2, graph_override=out["graph"])
            bad = dict(g2, X=out2["X"])
            frac = {n: float(((bad[n] - ref[n]).abs() > ATOL + RTOL * ref[n].abs()).double().mean()) for n in COMPARED}
            worst = max(frac, key=frac.get)
            print(f"class {first[label]} {label}, {name}: " + ", ".join(f"{n} {100 * f:.0f}%" for n, f in frac.items()))
            assert frac[worst] > 0.01, (label, name, frac)
            if name.startswith("two rows"):
                flips = int((closed_form.sbm_fwd_bwd(**kw2)[0]["graph"] != out["graph"]).sum())
                print(f"class {first[label]} {label}, {name}: {flips} of {out['graph'].numel()} sampled draws flip")
            if not name.startswith("attention"):  # on a fixed graph X does not see the projection masks
                assert frac["X"] == 0.0 and torch.equal(out2["X"], out["X"]), (label, name)
                assert max(frac[n] for n in PARAM_NAMES) > 0.01, (label, name, frac)
        done.append(first[label])
    assert sorted(done) == list("BCDF")
