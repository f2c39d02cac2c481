"""Decoding constraints on the GPU: k_constrain_rows (csrc/csa_constrain.hip) against the loop oracle
(tests/constrain_ref.py), bitwise on the whole logits buffer (the int32 image, untouched entries and the gaps between
strided rows included), over rows x V x T x t x rules; and the three generators with all rules on: the captured graph
against the eager loop, one graph per constraint value, and nothing changed where there are no constraints."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import constrain_ref
from conftest import has_gpu
from constrain_ref import (EOS_ID, GEN_MIN_LENGTH, GEN_SUPPRESS, GEN_T, KERNEL_ROWS, KERNEL_TS, KERNEL_VS, bits,
                           constrain_np, constraints, expected, generator_case, make, run, run_op)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]

ROWS = max(KERNEL_ROWS)


def oracle(case, V, name, t, finished=False):
    """The oracle's array for one (rule, step) of a case, for the largest row count: a row's result depends on the row
    alone, so the smaller launches are its first rows."""
    z, ys, fin = case
    return constrain_np(z, ys, t, fin=fin if finished else None, **constrain_ref.rules(V)[name]).z


class Launcher:
    """constrain_rows on device copies of one case: the rows, the tokens and the suppress list are uploaded once."""

    def __init__(self, z, ys, layout):
        self.rows, self.V = z.shape
        self.layout = layout
        self.z = torch.from_numpy(z).cuda()
        self.ys = torch.from_numpy(ys).cuda()
        self.sup = torch.tensor(constrain_ref.SUPPRESS, dtype=torch.int32, device="cuda")

    def __call__(self, rows, t, host=False, fin=None, suppress=None, **kw):
        """-> (the int32 image of the whole buffer after the call, the same before it), on the device."""
        from csa_amd.decode_ops import constrain_rows
        V = self.V
        if self.layout == "shifted":
            buf = torch.full((rows * (V + 3) + 1,), 77.0, dtype=torch.float32, device="cuda")
            view = buf[1:].view(rows, V + 3)[:, :V]
            view.copy_(self.z[:rows])
        else:
            buf = self.z[:rows].clone()
            view = buf
        before = buf.view(torch.int32).clone()
        step = int(t) if host else torch.tensor([t], dtype=torch.int32, device="cuda")
        ft = None if fin is None else torch.from_numpy(fin[:rows].copy()).cuda()
        constrain_rows(view, self.ys[:rows], step, fin=ft, suppress=None if suppress is None else self.sup, **kw)
        return buf.view(torch.int32), before


def want_image(want_z, rows, V, layout):
    return torch.from_numpy(expected(want_z, rows, V, layout).reshape(-1)).cuda()


CLASSES = [(V, "plain") for V in KERNEL_VS] + [(1028, "shifted")]  # shifted: base + 1 float, row stride V + 3


@pytest.mark.parametrize("T", KERNEL_TS)
@pytest.mark.parametrize("V,layout", CLASSES, ids=[f"{V}{'_shifted' if lay == 'shifted' else ''}" for V, lay in CLASSES])
def test_constrain_rows_kernel_is_bitwise_the_oracle(V, layout, T):
    case = constrain_ref.kernel_case(V, T)
    z, ys, fin = case
    go = Launcher(z, ys, layout)
    touched = 0
    for name, kw in constrain_ref.rules(V).items():
        for t in constrain_ref.steps(T):
            want_z = oracle(case, V, name, t)
            for rows in KERNEL_ROWS:
                what = f"V={V} {layout} T={T} rows={rows} {name} t={t}"
                want = want_image(want_z, rows, V, layout)
                got, before = go(rows, t, **kw)
                assert torch.equal(got.reshape(-1), want), what
                touched += int((got != before).sum())
            if name == "all":  # rows = 70: a second launch, the host-t form, finished rows
                again, _ = go(rows, t, **kw)
                host, _ = go(rows, t, host=True, **kw)
                assert torch.equal(again, got) and torch.equal(host, got), what
                some, before = go(rows, t, fin=fin, **kw)
                assert torch.equal(some.reshape(-1), want_image(oracle(case, V, name, t, True), rows, V, layout)), what
                if layout == "plain":
                    done = torch.from_numpy(fin != 0).cuda()
                    assert torch.equal(some[done], before[done]), what
                every, before = go(rows, t, fin=np.ones(rows, dtype=np.uint8), **kw)
                assert torch.equal(every, before), what
    assert touched > 0


@pytest.mark.parametrize("T", [2, 7, 1024])
def test_constrain_rows_kernel_stores_nothing_for_a_step_outside_its_range(T):
    V = 257
    z, ys, fin = constrain_ref.kernel_case(V, T)
    kw = constrain_ref.rules(V)["all"]
    for layout in ("plain", "shifted"):
        go = Launcher(z, ys, layout)
        for t in (-1, T - 1, T, T + 1000, 2 ** 31 - 1, -2 ** 31):
            got, before = go(ROWS, t, **kw)
            assert torch.equal(got, before), (layout, t)
        got, before = go(ROWS, T - 2, **kw)  # the last valid step does store
        assert not torch.equal(got, before)


def test_constrain_rows_hand_built_rows_through_the_kernel():
    """The ban on a penalised column, special values under the penalty and ids outside the vocabulary, as in the CPU
    test, through the kernel (run_op compares the whole buffer)."""
    ninf = -np.inf
    z = np.array([[4.0, -4.0, 2.0, 1.0, ninf, 0.5, 0.0, -0.0, np.nan, np.inf]] * 3, dtype=np.float32)
    ys = np.array([[2, 0, 1, 0, 6, 7, 8, 9, 2 ** 40, -1, 10, 0]] * 3, dtype=np.int64)
    fin = np.array([0, 1, 0], dtype=np.uint8)
    for t in range(ys.shape[1] - 1):
        for kw in (dict(repetition_penalty=2.0, no_repeat_ngram=2, min_length=9, eos_id=5, suppress=(3, 10, -4)),
                   dict(repetition_penalty=3.0), dict(repetition_penalty=0.3), dict(no_repeat_ngram=1)):
            want = constrain_np(z, ys, t, fin=fin, **kw).z
            for form in ("dev", "host"):
                got, _ = run_op(z, ys, t, device="cuda", fin=fin, form=form, **kw)
                assert np.array_equal(got, bits(want)), (t, kw, form)
    want = constrain_np(z, ys, 3, repetition_penalty=2.0, no_repeat_ngram=2).z
    assert want[0, 1] == ninf and want[0, 0] == 2.0  # 1 follows 0: banned although penalised


def test_constrain_rows_beyond_the_limit_takes_the_fallback():
    from csa_amd import _lib
    L = _lib.lib()
    assert L.csa_constrain_rows_supported(1024) == 1 and L.csa_constrain_rows_supported(1025) == 0
    assert L.csa_constrain_rows_supported(1) == 0
    z, ys, fin = constrain_ref.kernel_case(19, 1025, rows=3)
    kw = constrain_ref.rules(19)["all"]
    for t in (2, 1023):
        got, _ = run_op(z, ys, t, device="cuda", fin=fin, **kw)
        assert np.array_equal(got, bits(constrain_np(z, ys, t, fin=fin, **kw).z))


# ---- the generators ----

def graph_nodes(gen):
    (entry,) = gen._graphs.values()
    with open("/proc/self/maps") as f:  # the HIP runtime torch has loaded, not a second copy of it
        path = next(ln.split()[-1] for ln in f if "libamdhip64" in ln)
    hip = ctypes.CDLL(path)
    n = ctypes.c_size_t(0)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    assert hip.hipGraphGetNodes(ctypes.c_void_p(entry.graph.raw_cuda_graph()), None, ctypes.byref(n)) == 0
    return int(n.value)


def tensors(out):
    return out if isinstance(out, tuple) else (out,)


@pytest.mark.parametrize("kind", ["greedy", "beam", "sample"])
def test_generator_graph_equals_eager_with_one_graph_per_constraint_value(kind):
    m, enc, src_mask = generator_case(device="cuda")
    con, other = constraints(), constraints(no_repeat_ngram_size=3, suppress_ids=(7,))
    extra = dict(beam=dict(return_all=True)).get(kind, dict(return_logp=True))
    eager = make(kind, m, constraints=con)
    gen = make(kind, m, constraints=con, graph=True)
    want = tensors(run(kind, eager, enc, src_mask, **extra))
    got = tensors(run(kind, gen, enc, src_mask, **extra))
    again = tensors(run(kind, gen, enc, src_mask, **extra))
    assert gen.captures == 1 and eager.captures == 0
    for a, b, c in zip(want, got, again):
        assert torch.equal(a, b) and torch.equal(a, c)  # ids and log-probabilities, bitwise
    ids = got[0].reshape(-1, GEN_T - 1).cpu().numpy() if kind != "beam" else got[1].reshape(-1, GEN_T - 1).cpu().numpy()
    assert constrain_ref.output_faults(ids, 2, GEN_MIN_LENGTH, GEN_SUPPRESS) == (0, 0, 0)
    if kind == "greedy":  # return_logp reports the constrained distribution, renormalised
        logp = got[1]
        assert bool((logp[:, :, list(GEN_SUPPRESS)] == -np.inf).all())
        assert bool((logp[:GEN_MIN_LENGTH, :, EOS_ID] == -np.inf).all())
        np.testing.assert_allclose(logp.exp().sum(-1).cpu().numpy(), 1.0, rtol=1e-5)
    gen.constraints = other  # another value: a graph of its own, and again the eager result
    eager.constraints = other
    got2 = tensors(run(kind, gen, enc, src_mask, **extra))
    assert gen.captures == 2
    for a, b in zip(tensors(run(kind, eager, enc, src_mask, **extra)), got2):
        assert torch.equal(a, b)
    gen.constraints = con  # back: the first graph is still there
    for a, b in zip(want, tensors(run(kind, gen, enc, src_mask, **extra))):
        assert torch.equal(a, b)
    assert gen.captures == 2


@pytest.mark.parametrize("kind", ["greedy", "beam", "sample"])
def test_no_constraints_leave_the_captured_graph_as_it_was(kind):
    from csa_amd.model import DecodingConstraints
    m, enc, src_mask = generator_case(device="cuda")
    nodes, outs = {}, {}
    for name, kw in (("plain", {}), ("none", dict(constraints=None)), ("inactive", dict(constraints=DecodingConstraints())),
                     ("active", dict(constraints=constraints()))):
        gen = make(kind, m, graph=True, **kw)
        gen._keep_graph = True
        outs[name] = run(kind, gen, enc, src_mask)
        assert gen.captures == 1
        nodes[name] = graph_nodes(gen)
    print(kind, "captured nodes:", nodes)
    assert nodes["none"] == nodes["plain"] and nodes["inactive"] == nodes["plain"]
    assert nodes["active"] == nodes["plain"] + 1  # the one constrain_rows launch
    assert torch.equal(outs["none"], outs["plain"]) and torch.equal(outs["inactive"], outs["plain"])
    assert torch.equal(outs["plain"], run(kind, make(kind, m), enc, src_mask))  # the eager path, as before
    assert not torch.equal(outs["active"], outs["plain"])


def test_generator_graph_refuses_a_token_buffer_beyond_the_kernel():
    m, enc, src_mask = generator_case(device="cuda")
    from csa_amd.model import CachedGreedyGenerator, SamplingGenerator
    for gen in (CachedGreedyGenerator(m, 1025, graph=True, constraints=constraints()),
                SamplingGenerator(m, 1025, graph=True, constraints=constraints())):
        with pytest.raises(ValueError):
            gen(SimpleNamespace()) if isinstance(gen, CachedGreedyGenerator) else gen.sample(enc, src_mask, seed=1)
        assert gen.captures == 0
