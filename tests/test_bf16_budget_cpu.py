"""The tolerance constants of tests/test_bf16_paths_gpu.py cannot drift: the emulation budget (bf16 emulation in fp32
against fp64 arithmetic, oracle only) of that file's cases with N <= 64 is recomputed here, and every committed
constant must be at least 4 x what is found (and no constant for X / dQ / dK / dV may exceed 5e-3: beyond that the
emulation would not be modelling the kernel). Also pins that the fp32-arithmetic emulation stays an emulation of the
same thing: its own distance to the fp64 one is far below the bf16 mode's distance to exact fp32 math."""
import pytest
import torch

import test_bf16_paths_gpu as T
from oracle import closed_form


def _small_cases():
    cases = [(f"eval{s}", T.eval_case(s)) for s in T.EVAL_SHAPES if s[2] <= 64]
    cases += [(f"train{s} p={p}", T.train_case(s, p)) for s, p in T.TRAIN_CASES if s[2] <= 64]
    cases += [(f"maps{s} train={tr}", T.map_case(s, tr)) for s in T.MAP_SHAPES for tr in (False, True)]
    cases += [(f"dense-train{s}", T.dense_train_case(s)) for s in T.DENSE_TRAIN_SHAPES if s[2] <= 64]
    cases += [("dense-dattn", T.dense_dattn_case())]
    return cases


def test_committed_tolerances_cover_four_times_the_recomputed_budget():
    assert set(T.TOL) == {"X", "expA", "dQKV", "layer.weight", "proj.weight", "proj.bias"}
    assert all(v >= T.FLOOR for v in T.TOL.values())
    assert T.TOL["X"] <= 5e-3 and T.TOL["dQKV"] <= 5e-3
    cases = _small_cases()
    assert len(cases) >= 10
    for label, c in cases:
        for name, (m, f) in closed_form.emulation_budget(c["kw"]).items():
            tol = T.TOL[T.tol_class(name)]
            print(f"budget {label} {name}: element metric {m:.3g} Frobenius {f:.3g}")
            assert tol >= 4 * max(m, f), (label, name, m, f, tol)


def test_emulation_budget_uses_one_graph_and_is_far_below_the_bf16_error():
    c = T.train_case((1, 2, 45, 96, 5), 0.1)
    kw = c["kw"]
    b = closed_form.emulation_budget(kw)
    o16, g16 = closed_form.sbm_fwd_bwd(**kw, bf16=True)
    o32, g32 = closed_form.sbm_fwd_bwd(**kw, graph_override=o16["graph"], bf16=False)
    for name, a, r in (("X", o16["X"], o32["X"]), ("Q", g16["Q"], g32["Q"]), ("V", g16["V"], g32["V"])):
        bf_err = closed_form.elem_metric(a, r)
        assert 1e-4 < bf_err < 2e-2 and max(b[name]) < 0.1 * bf_err, (name, bf_err, b[name])
    # dtype is a parameter of the same code: the fp32 run returns fp32 tensors on the fp64 run's graph
    o, g = closed_form.sbm_fwd_bwd(**kw, graph_override=o16["graph"], bf16=True, dtype=torch.float32)
    assert o["X"].dtype == torch.float32 and g["proj.0.weight"].dtype == torch.float32
    assert torch.equal(o["graph"].double(), o16["graph"])


def test_bf16_degenerate_case_stays_degenerate_under_rounded_scores(golden):
    """The bf16 degenerate-normaliser construction on the CPU: n of the built row is below eps under the
    bf16-rounded scores (so rho = gamma != 0 in the emulation) and the plain-fp32 scores alike."""
    c = T.degenerate_case(golden("sbm_n150"))
    for bf in (True, False):
        out, _ = closed_form.sbm_fwd_bwd(**c["kw"], bf16=bf)
        n = out["n"][:, :, T.DEGEN_I]
        assert 0 < float(n.min()) and float(n.max()) < 1e-12, (bf, float(n.max()))
