"""Global gradient-norm clipping in the AdamW step, the part that needs no GPU: the fp64 oracle (clip_ref) against
the per-op CPU path of csa_amd.train.AdamW(max_grad_norm=...), proof that every wrong variant of the clipped step
is far outside the tolerance the GPU tests use, the argument validation of the three C entry points, two gloo ranks,
and the constructor's checks."""
import ctypes
import math
import multiprocessing as mp
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

import clip_ref
import elementwise_ref as ref


def _cpu_optimizer(case, correct_bias, max_norm):
    from csa_amd.train import AdamW
    ws = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in case["p"]]
    opt = AdamW(ws, correct_bias=correct_bias, max_grad_norm=max_norm, **ref.ADAMW_HP)
    for w, m, v in zip(ws, case["m"], case["v"]):
        opt.state[w] = {"step": ref.ADAMW_STEP0, "exp_avg": torch.from_numpy(m.copy()),
                        "exp_avg_sq": torch.from_numpy(v.copy())}
    return ws, opt


# ---- (a) the oracle is the CPU path ----

@pytest.mark.parametrize("max_norm", [1.0, 50.0, 1e4])
@pytest.mark.parametrize("correct_bias", [False, True])
def test_oracle_is_the_cpu_path_of_the_clipped_step(correct_bias, max_norm):
    """Two steps under grad_scale = 3073 from the non-zero state: parameters and moments at the AdamW tolerances,
    the norm (of the unscaled gradients) and the coefficient at rtol 1e-6, p.grad untouched."""
    case = ref.adamw_case(steps=2)
    ws, opt = _cpu_optimizer(case, correct_bias, max_norm)
    opt.grad_scale = torch.tensor(ref.GRAD_SCALE)
    scaled = [ref.scaled_grads(g) for g in case["g"]]
    want, norms, coefs = clip_ref.clipped_steps64(case, scaled, correct_bias, max_norm, scale=ref.GRAD_SCALE)
    for k in range(2):
        for w, g in zip(ws, scaled[k]):
            w.grad = torch.from_numpy(g.copy())
        opt.step()
        for w, g in zip(ws, scaled[k]):
            assert np.array_equal(w.grad.numpy(), g)
        assert opt.last_grad_norm.shape == () and opt.last_clip_coef.shape == ()
        np.testing.assert_allclose(opt.last_grad_norm.item(), norms[k], rtol=clip_ref.NORM_RTOL)
        np.testing.assert_allclose(opt.last_clip_coef.item(), coefs[k], rtol=clip_ref.NORM_RTOL)
        assert (coefs[k] == 1.0) == (max_norm == 1e4)
    for i, w in enumerate(ws):
        st = opt.state[w]
        assert st["step"] == ref.ADAMW_STEP0 + 2
        for got, exp, atol in ((w.detach(), want[0][i], ref.ADAMW_ATOL), (st["exp_avg"], want[1][i], ref.ADAMW_ATOL),
                               (st["exp_avg_sq"], want[2][i], ref.ADAMW_ATOL_V)):
            np.testing.assert_allclose(got.numpy(), exp, rtol=ref.ADAMW_RTOL, atol=atol, err_msg=f"tensor {i}")


@pytest.mark.parametrize("correct_bias", [False, True])
def test_cpu_path_skips_the_step_on_a_non_finite_norm(correct_bias):
    case = ref.adamw_case(steps=1)
    ws, opt = _cpu_optimizer(case, correct_bias, 1.0)
    grads = [g.copy() for g in case["g"][0]]
    grads[7][9000] = np.nan
    for w, g in zip(ws, grads):
        w.grad = torch.from_numpy(g)
    opt.step()
    assert not math.isfinite(opt.last_grad_norm.item()) and opt.last_clip_coef.item() == 0.0
    for i, w in enumerate(ws):
        st = opt.state[w]
        assert st["step"] == ref.ADAMW_STEP0
        assert np.array_equal(w.detach().numpy(), case["p"][i]) and np.array_equal(st["exp_avg"].numpy(), case["m"][i])
        assert np.array_equal(st["exp_avg_sq"].numpy(), case["v"][i])


def test_cpu_path_without_clipping_keeps_its_bits_and_allocates_nothing():
    """max_grad_norm=None is the step as it was; a max_grad_norm above the norm gives the same bits (coefficient 1)."""
    case = ref.adamw_case(steps=2)
    runs = []
    for max_norm in (None, 1e4):
        ws, opt = _cpu_optimizer(case, False, max_norm)
        for k in range(2):
            for w, g in zip(ws, case["g"][k]):
                w.grad = torch.from_numpy(g.copy())
            opt.step()
        runs.append((ws, opt))
    (wa, oa), (wb, ob) = runs
    assert oa.last_grad_norm is None and oa.last_clip_coef is None and oa._clip_partials is None and oa._clip_state is None
    assert ob.last_clip_coef.item() == 1.0
    for a, b in zip(wa, wb):
        assert np.array_equal(a.detach().numpy(), b.detach().numpy())
        assert np.array_equal(oa.state[a]["exp_avg_sq"].numpy(), ob.state[b]["exp_avg_sq"].numpy())


# ---- (b) decisiveness ----

def _first_step(case, grads, correct_bias, max_norm, scale=None, mutant=None):
    state = [(p, m, v) for p, m, v in zip(case["p"], case["m"], case["v"])]
    new, norm, coef = clip_ref.clipped_step64(state, grads, ref.ADAMW_STEP0 + 1, correct_bias, max_norm, scale, mutant)
    return [s[0] for s in new], norm, coef


@pytest.mark.parametrize("correct_bias", [False, True])
def test_wrong_variants_of_the_clipped_step_are_far_outside_the_tolerance(correct_bias):
    """adamw_case() step 0: 42,788 elements, global norm 554.13. Each mutant moves more than 90% of the parameters
    outside the AdamW tolerance (measured: the fractions printed below), so the GPU tests cannot pass with one."""
    case = ref.adamw_case(steps=1)
    g = case["g"][0]
    assert sum(a.size for a in g) == 42788
    np.testing.assert_allclose(clip_ref.global_norm64(g), 554.13, rtol=1e-5)
    scaled = ref.scaled_grads(g)
    for max_norm in clip_ref.MAX_NORMS:
        want, _, coef = _first_step(case, g, correct_bias, max_norm)
        assert coef < 1.0
        for mutant in ("no_clip", "per_tensor"):
            frac = clip_ref.outside_fraction(_first_step(case, g, correct_bias, max_norm, mutant=mutant)[0], want)
            print(f"max_norm {max_norm}: {mutant}: {frac:.4f}")
            assert frac > 0.9, (max_norm, mutant, frac)
        want_s = _first_step(case, scaled, correct_bias, max_norm, scale=ref.GRAD_SCALE)[0]
        frac = clip_ref.outside_fraction(
            _first_step(case, scaled, correct_bias, max_norm, scale=ref.GRAD_SCALE, mutant="scaled_norm")[0], want_s)
        print(f"max_norm {max_norm}: scaled_norm: {frac:.4f}")
        assert frac > 0.9, (max_norm, "scaled_norm", frac)
    big = clip_ref.MAX_NORM_INACTIVE
    want, _, coef = _first_step(case, g, correct_bias, big)
    unclipped = [ref.adamw64(p, m, v, a, ref.ADAMW_STEP0 + 1, correct_bias)[0]
                 for p, m, v, a in zip(case["p"], case["m"], case["v"], g)]
    assert coef == 1.0 and all(np.array_equal(a, b) for a, b in zip(want, unclipped))
    frac = clip_ref.outside_fraction(_first_step(case, g, correct_bias, big, mutant="unclamped")[0], want)
    print(f"max_norm {big}: unclamped: {frac:.4f}")
    assert frac > 0.9, frac
    want_s = _first_step(case, scaled, correct_bias, big, scale=ref.GRAD_SCALE)[0]
    frac = clip_ref.outside_fraction(
        _first_step(case, scaled, correct_bias, big, scale=ref.GRAD_SCALE, mutant="scaled_norm")[0], want_s)
    print(f"max_norm {big}: scaled_norm: {frac:.4f}")
    assert frac > 0.9, frac


# ---- (c) the C ABI ----

def test_entry_points_validate_without_gpu():
    from csa_amd import _lib
    L = _lib.lib()
    some = (ctypes.c_double * 8)()      # a non-null address; no call below gets as far as a launch
    addr = ctypes.addressof(some)
    # csa_grad_sumsq
    assert L.csa_grad_sumsq(None, None) == 1
    assert L.csa_grad_sumsq(ctypes.byref(_lib.GradSumsqArgs(nchunks=0)), None) == 0  # nothing to sum: no launch
    assert L.csa_grad_sumsq(ctypes.byref(_lib.GradSumsqArgs(nchunks=3, ntensors=1, partials=addr)), None) == 1
    assert b"null tensor table" in L.csa_last_error_str()
    a = _lib.GradSumsqArgs(tensors=addr, chunk_tensor=addr, chunk_start=addr, ntensors=1, nchunks=3)
    assert L.csa_grad_sumsq(ctypes.byref(a), None) == 1
    assert b"null partials" in L.csa_last_error_str()
    for bad in (dict(nchunks=-1), dict(ntensors=-1, nchunks=1), dict(nchunks=1, first=-1), dict(nchunks=2 ** 31)):
        a = _lib.GradSumsqArgs(tensors=addr, chunk_tensor=addr, chunk_start=addr, partials=addr, **bad)
        assert L.csa_grad_sumsq(ctypes.byref(a), None) == 1, bad
    # csa_grad_norm_finish
    assert L.csa_grad_norm_finish(addr, 4, None, 1.0, None, None) == 1
    assert b"null state" in L.csa_last_error_str()
    assert L.csa_grad_norm_finish(addr, -1, None, 1.0, addr, None) == 1
    assert L.csa_grad_norm_finish(None, 4, None, 1.0, addr, None) == 1
    assert L.csa_grad_norm_finish(addr, 4, None, float("nan"), addr, None) == 1
    assert b"NaN" in L.csa_last_error_str()
    # csa_adamw_step_clipped validates as csa_adamw_step does
    assert L.csa_adamw_step_clipped(None, addr, None) == 1
    assert L.csa_adamw_step_clipped(ctypes.byref(_lib.AdamwArgs(nchunks=0, beta1=0.9, beta2=0.999)), addr, None) == 0
    a = _lib.AdamwArgs(nchunks=3, ntensors=1, beta1=0.9, beta2=0.999)
    assert L.csa_adamw_step_clipped(ctypes.byref(a), addr, None) == 1
    assert b"null tensor table" in L.csa_last_error_str()
    a = _lib.AdamwArgs(tensors=addr, chunk_tensor=addr, chunk_start=addr, nchunks=3, ntensors=1, beta1=1.5, beta2=0.999)
    assert L.csa_adamw_step_clipped(ctypes.byref(a), addr, None) == 1
    assert L.csa_abi_version() == 10


# ---- (d) two gloo ranks ----

def _worker(rank, world, port, q, impls, steps, max_norm):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from test_train_cpu import Tiny, _batch
    from csa_amd.model import label_smoothing_loss
    from csa_amd.train import AdamW, grad_norm, init_distributed, make_train_step, wrap_ddp
    torch.cuda.is_available = lambda: False  # the gloo / host path is the one under test, also on a box with GPUs
    _, _, _, dev = init_distributed()
    out = {}
    for impl in impls:
        torch.manual_seed(0 if rank == 0 else 1 + rank)
        model = Tiny()
        ddp = wrap_ddp(model, dev, impl=impl, bucket_cap_mb=64)
        opt = AdamW(model.parameters(), lr=1e-3, correct_bias=False, max_grad_norm=max_norm)
        step = make_train_step(ddp, opt, label_smoothing_loss, sw=1e-2)
        rec = []
        for i in range(steps):
            step(*_batch(rank, i))  # a different batch on every rank
            rec.append(dict(norm=opt.last_grad_norm.numpy().copy(), coef=opt.last_clip_coef.numpy().copy(),
                            logged=grad_norm(model.parameters()).numpy().copy(),
                            grads=[p.grad.numpy().copy() for p in model.parameters()],
                            weights=[p.detach().numpy().copy() for p in model.parameters()]))
        out[impl] = rec
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_compute_one_norm_and_stay_identical():
    """2-rank gloo, different batches per rank: step() runs after the all-reduce, so both ranks clip by the same
    norm, bit for bit (no collective of its own), that norm is the fp64 norm of the averaged gradient, and the
    replicas stay identical. max_norm is small enough for the clipping to be active on every step."""
    from test_train_cpu import _free_port
    impls, steps, max_norm = ("torch", "bucketed"), 2, 1e-3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, impls, steps, max_norm)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for impl in impls:
        for s in range(steps):
            a, b = res[0][impl][s], res[1][impl][s]
            assert a["norm"].dtype == np.float32 and a["norm"].tobytes() == b["norm"].tobytes()
            assert a["coef"].tobytes() == b["coef"].tobytes() and a["logged"].tobytes() == a["norm"].tobytes()
            want = clip_ref.global_norm64(a["grads"])
            np.testing.assert_allclose(float(a["norm"]), want, rtol=clip_ref.NORM_RTOL)
            np.testing.assert_allclose(float(a["coef"]), clip_ref.clip_coef64(want, max_norm), rtol=clip_ref.NORM_RTOL)
            assert float(a["coef"]) < 1.0
            for x, y in zip(a["grads"], b["grads"]):
                np.testing.assert_array_equal(x, y)
            for x, y in zip(a["weights"], b["weights"]):
                np.testing.assert_array_equal(x, y)


# ---- (e) the constructor ----

@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("inf"), float("nan")])
def test_constructor_rejects_a_max_grad_norm_that_is_not_positive_and_finite(bad):
    from csa_amd.train import AdamW
    w = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError):
        AdamW([w], max_grad_norm=bad)
    assert AdamW([w], max_grad_norm=1).max_grad_norm == 1.0 and AdamW([w]).max_grad_norm is None
