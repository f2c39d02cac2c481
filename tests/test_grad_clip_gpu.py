"""Global gradient-norm clipping inside the fused AdamW step on the GPU: k_grad_sumsq, k_grad_norm_finish and the
clipped k_adamw (csrc/csa_optim.hip) through the C ABI and through csa_amd.train.AdamW(max_grad_norm=...) /
csa_amd.train.grad_norm, against the fp64 oracle of clip_ref.py. test_grad_clip_cpu.py shows on the CPU that the
oracle is the per-op CPU path and that every wrong variant of the clipped step is far outside these tolerances.

Launch classes of k_grad_sumsq: one workgroup per chunk of CSA_ADAMW_CHUNK = 4096 elements, as k_adamw; inside a
chunk dwordx4 loads when the chunk's gradient pointer is 16-byte aligned (with a scalar tail of n % 4 elements),
scalar loads otherwise. elementwise_ref.ADAMW_SIZES has chunk lengths 1, 3, 4, 7, 4095 and 4096, an empty tensor
and tensors of several chunks; every second tensor starts one float off a 16-byte boundary. k_grad_norm_finish sums
n partials with a 256-lane strided loop: n = 274 here (one tensor of 257 * 4096 + 5 elements), so the loop passes
twice, and n = 1 .. 16 in the optimizer tests."""
import ctypes
import math

import numpy as np
import pytest
import torch

import clip_ref
import elementwise_ref as ref
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _dev_view(a, shift):
    """a's values on the device as a view that starts 4 * shift bytes off a 16-byte boundary."""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
    view = buf[4 + shift:4 + shift + a.size]
    view.copy_(torch.from_numpy(a))
    assert a.size == 0 or view.data_ptr() % 16 == 4 * shift
    return view


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. the two norm kernels through the C ABI ----

def test_sumsq_launch_classes_and_finish_through_the_c_abi():
    from csa_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(3)
    sizes = list(ref.ADAMW_SIZES) + [clip_ref.FINISH_PASSES_N]
    grads = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-2.0, 1.0, n)).astype(np.float32) for n in sizes]
    views = [_dev_view(g, i % 2) for i, g in enumerate(grads)]  # every second pointer is 4-byte aligned only
    owner, start, nchunks = clip_ref.chunk_tables(sizes)
    assert nchunks == 274 and nchunks > 256
    # csa_adamw_tensor descriptors {param, grad, exp_avg, exp_avg_sq, numel}: the kernel reads grad and numel only
    desc = torch.tensor([[0, v.data_ptr(), 0, 0, n] for v, n in zip(views, sizes)], dtype=torch.int64).cuda()
    owner_d, start_d = torch.from_numpy(owner).cuda(), torch.from_numpy(start).cuda()
    first, guard = 3, 5
    want_chunks = clip_ref.chunk_sumsq64(grads)
    want_norm = clip_ref.global_norm64(grads)
    scale = torch.full((), ref.GRAD_SCALE, device="cuda")
    runs = []
    for _ in range(2):
        partials = torch.full((first + nchunks + guard,), float("nan"), dtype=torch.float64, device="cuda")
        states = torch.full((3, 4 + guard), float(ref.SENTINEL), dtype=torch.float32, device="cuda")
        a = _lib.GradSumsqArgs(tensors=desc.data_ptr(), chunk_tensor=owner_d.data_ptr(), chunk_start=start_d.data_ptr(),
                               ntensors=len(sizes), nchunks=nchunks, partials=partials.data_ptr(), first=first)
        _lib.check(L.csa_grad_sumsq(ctypes.byref(a), _stream()), "csa_grad_sumsq")
        p0 = partials.data_ptr() + 8 * first
        for row, (sc, max_norm) in enumerate(((None, 50.0), (scale, 50.0), (None, 0.0))):
            _lib.check(L.csa_grad_norm_finish(p0, nchunks, None if sc is None else sc.data_ptr(), max_norm,
                                              states[row].data_ptr(), _stream()), "csa_grad_norm_finish")
        runs.append((partials.cpu(), states.cpu()))
    (pa, sa), (pb, sb) = runs
    assert torch.equal(pa.view(torch.int64), pb.view(torch.int64)) and torch.equal(_bits(sa), _bits(sb))
    assert bool(torch.isnan(pa[:first]).all()) and bool(torch.isnan(pa[first + nchunks:]).all())
    np.testing.assert_allclose(pa[first:first + nchunks].numpy(), want_chunks, rtol=1e-12)
    assert bool((sa[:, 4:] == float(ref.SENTINEL)).all())
    for row, (sc, max_norm) in enumerate(((1.0, 50.0), (ref.GRAD_SCALE, 50.0), (1.0, 0.0))):
        norm, coef, bad, zero = sa[row, :4].tolist()
        np.testing.assert_allclose(norm, want_norm / sc, rtol=clip_ref.NORM_RTOL)
        want_coef = clip_ref.clip_coef64(want_norm / sc, max_norm) if max_norm > 0 else 1.0
        np.testing.assert_allclose(coef, want_coef, rtol=clip_ref.NORM_RTOL)
        assert bad == 0.0 and zero == 0.0
    assert sa[0, 1] < 1.0 and sa[2, 1] == 1.0
    # n = 0: norm 0, coefficient 1, no partials read
    st = torch.full((4,), float(ref.SENTINEL), dtype=torch.float32, device="cuda")
    _lib.check(L.csa_grad_norm_finish(None, 0, None, 1.0, st.data_ptr(), _stream()), "csa_grad_norm_finish")
    assert st.tolist() == [0.0, 1.0, 0.0, 0.0]


# ---- the optimizer on a layout with every second tensor one float off ----

class _Layout:
    def __init__(self, case, correct_bias, max_norm):
        from csa_amd.train import AdamW
        self.views = {k: [_dev_view(a, i % 2) for i, a in enumerate(case["g"][0] if k == "g" else case[k])]
                      for k in ("p", "g", "m", "v")}
        self.params = [torch.nn.Parameter(v) for v in self.views["p"]]
        for w, g in zip(self.params, self.views["g"]):
            w.grad = g
        kw = {} if max_norm is None else dict(max_grad_norm=max_norm)
        self.opt = AdamW(self.params, correct_bias=correct_bias, **ref.ADAMW_HP, **kw)
        for w, m, v in zip(self.params, self.views["m"], self.views["v"]):
            self.opt.state[w] = {"step": ref.ADAMW_STEP0, "exp_avg": m, "exp_avg_sq": v}

    def step(self, grads):
        for gv, a in zip(self.views["g"], grads):
            gv.copy_(torch.from_numpy(a))
        self.opt.step()
        for w, gv, a in zip(self.params, self.views["g"], grads):  # p.grad: the same memory, the same bits
            assert w.grad.data_ptr() == gv.data_ptr()
            assert np.array_equal(gv.cpu().numpy().view(np.int32), a.view(np.int32)), "step() changed p.grad"

    def snapshot(self):
        return [[t.clone() for t in self.views[k]] for k in ("p", "m", "v")]

    def assert_matches(self, want, what):
        for i, w in enumerate(self.params):
            st = self.opt.state[w]
            for name, got, exp, atol in (("p", w.detach(), want[0][i], ref.ADAMW_ATOL),
                                         ("exp_avg", st["exp_avg"], want[1][i], ref.ADAMW_ATOL),
                                         ("exp_avg_sq", st["exp_avg_sq"], want[2][i], ref.ADAMW_ATOL_V)):
                np.testing.assert_allclose(got.cpu().numpy(), exp, rtol=ref.ADAMW_RTOL, atol=atol,
                                           err_msg=f"{what}: {name} of tensor {i} ({exp.size} elements)")


def _assert_norm(opt, norm, coef):
    assert opt.last_grad_norm.shape == () and opt.last_grad_norm.is_cuda and opt.last_clip_coef.is_cuda
    np.testing.assert_allclose(opt.last_grad_norm.item(), norm, rtol=clip_ref.NORM_RTOL)
    np.testing.assert_allclose(opt.last_clip_coef.item(), coef, rtol=clip_ref.NORM_RTOL)


# ---- 2. range ----

def _range_case(g, seed):
    base = ref.adamw_case(sizes=[g.size], seed=seed, steps=1)
    return dict(p=base["p"], m=base["m"], v=base["v"], g=[[g]])


def test_gradients_whose_fp32_squares_overflow():
    """4096 gradients of 1e25: their squares overflow fp32 (1e50), the fp64 sum does not. norm = 64e25 = 6.4e26,
    coefficient 1 / 6.4e26 = 1.5625e-27, and the update sees gradients of 1.5625e-2."""
    g = np.full(4096, 1e25, dtype=np.float32)
    with np.errstate(over="ignore"):
        assert np.isinf(g * g).all()
    case = _range_case(g, 21)
    lay = _Layout(case, False, 1.0)
    lay.step([g])
    want, norms, coefs = clip_ref.clipped_steps64(case, [[g]], False, 1.0)
    np.testing.assert_allclose([norms[0], coefs[0]], [6.4e26, 1.5625e-27], rtol=1e-6)
    _assert_norm(lay.opt, norms[0], coefs[0])
    assert all(bool(torch.isfinite(t).all()) for k in ("p", "m", "v") for t in lay.views[k])
    lay.assert_matches(want, "1e25 gradients")


def test_one_large_entry_among_many_small_ones():
    g = np.full(40001, 1e-4, dtype=np.float32)
    g[12345] = 1e4
    case = _range_case(g, 22)
    lay = _Layout(case, False, 1.0)
    lay.step([g])
    want, norms, coefs = clip_ref.clipped_steps64(case, [[g]], False, 1.0)
    _assert_norm(lay.opt, norms[0], coefs[0])
    lay.assert_matches(want, "1e4 among 1e-4")


# ---- 3. the clipped step against the oracle ----

@pytest.mark.parametrize("max_norm", clip_ref.MAX_NORMS)
@pytest.mark.parametrize("correct_bias", [False, True])
def test_clipped_step_matches_fp64_from_a_non_zero_state(correct_bias, max_norm):
    case = ref.adamw_case()
    lay = _Layout(case, correct_bias, max_norm)
    want, norms, coefs = clip_ref.clipped_steps64(case, case["g"], correct_bias, max_norm)
    for k in range(4):
        lay.step(case["g"][k])
        _assert_norm(lay.opt, norms[k], coefs[k])
        assert coefs[k] < 1.0
    lay.assert_matches(want, f"4 steps, max_norm {max_norm}")
    assert all(lay.opt.state[w]["step"] == ref.ADAMW_STEP0 + 4 for w in lay.params)


@pytest.mark.parametrize("correct_bias", [False, True])
def test_clipped_step_under_a_grad_scale(correct_bias):
    """grad_scale = 3073 handed over as GradScaler does: the norm is that of the unscaled gradients, and the update
    uses (g * fl32(1 / 3073)) * coef."""
    case = ref.adamw_case(steps=1)
    lay = _Layout(case, correct_bias, 50.0)
    lay.opt.grad_scale = torch.full((), ref.GRAD_SCALE, device="cuda")
    scaled = ref.scaled_grads(case["g"][0])
    want, norms, coefs = clip_ref.clipped_steps64(case, [scaled], correct_bias, 50.0, scale=ref.GRAD_SCALE)
    lay.step(scaled)
    _assert_norm(lay.opt, norms[0], coefs[0])
    lay.assert_matches(want, "scaled gradients")


# ---- 4. inactive clipping ----

def test_a_max_norm_above_the_norm_and_none_keep_the_bits():
    case = ref.adamw_case()
    plain, big = _Layout(case, False, None), _Layout(case, False, clip_ref.MAX_NORM_INACTIVE)
    for k in range(4):
        plain.step(case["g"][k])
        big.step(case["g"][k])
        assert big.opt.last_clip_coef.item() == 1.0
    for k in ("p", "m", "v"):
        for a, b in zip(plain.views[k], big.views[k]):
            assert torch.equal(_bits(a), _bits(b))
    o = plain.opt
    assert o.max_grad_norm is None and o._clip_partials is None and o._clip_state is None
    assert o.last_grad_norm is None and o.last_clip_coef is None
    assert big.opt._clip_partials.dtype == torch.float64 and big.opt._clip_state.shape == (4,)


# ---- 5. under torch.amp.GradScaler ----

def test_clipped_step_under_gradscaler_unscales_clips_and_skips_on_inf():
    from csa_amd.train import AdamW
    g = torch.Generator().manual_seed(11)
    w0 = torch.randn(300, 7, generator=g)
    x = torch.randn(64, 300, generator=g)
    max_norm = 0.05
    pg, pc = torch.nn.Parameter(w0.cuda()), torch.nn.Parameter(w0.clone())
    og = AdamW([pg], lr=1e-3, correct_bias=False, max_grad_norm=max_norm)
    oc = AdamW([pc], lr=1e-3, correct_bias=False, max_grad_norm=max_norm)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    for step in range(3):
        og.zero_grad(set_to_none=True)
        oc.zero_grad(set_to_none=True)
        scaler.scale((x.cuda() @ pg).square().mean()).backward()
        (x @ pc).square().mean().backward()
        kept = pg.grad.clone()
        scaler.step(og)
        scaler.update()
        oc.step()
        assert torch.equal(_bits(pg.grad), _bits(kept))  # still the scaled gradient
        unscaled = clip_ref.global_norm64([kept.cpu().numpy()], scale=2.0 ** 16)
        np.testing.assert_allclose(og.last_grad_norm.item(), unscaled, rtol=clip_ref.NORM_RTOL)
        np.testing.assert_allclose(og.last_clip_coef.item(), clip_ref.clip_coef64(unscaled, max_norm),
                                   rtol=clip_ref.NORM_RTOL)
        assert og.last_clip_coef.item() < 1.0
        np.testing.assert_allclose(og.last_grad_norm.item(), oc.last_grad_norm.item(), rtol=1e-5)
    np.testing.assert_allclose(pg.detach().cpu().numpy(), pc.detach().numpy(), rtol=1e-5, atol=1e-7)
    before, m_before, v_before = pg.detach().clone(), og.state[pg]["exp_avg"].clone(), og.state[pg]["exp_avg_sq"].clone()
    og.zero_grad(set_to_none=True)
    scale = scaler.get_scale()
    scaler.scale((x.cuda() @ pg).square().mean() * float("inf")).backward()
    scaler.step(og)
    scaler.update()
    assert torch.equal(_bits(pg), _bits(before)) and torch.equal(_bits(og.state[pg]["exp_avg"]), _bits(m_before))
    assert torch.equal(_bits(og.state[pg]["exp_avg_sq"]), _bits(v_before))
    assert not math.isfinite(og.last_grad_norm.item()) and og.last_clip_coef.item() == 0.0
    assert scaler.get_scale() == scale * 0.5


@pytest.mark.parametrize("correct_bias", [False, True])
def test_a_nan_gradient_skips_the_step_without_a_scaler(correct_bias):
    case = ref.adamw_case(steps=2)
    lay = _Layout(case, correct_bias, 1.0)
    bad = [a.copy() for a in case["g"][0]]
    bad[7][9000] = np.nan
    before = lay.snapshot()
    lay.step(bad)
    assert math.isnan(lay.opt.last_grad_norm.item()) and lay.opt.last_clip_coef.item() == 0.0
    for got, exp in zip(lay.snapshot(), before):
        for a, b in zip(got, exp):
            assert torch.equal(_bits(a), _bits(b))
    if correct_bias:  # decided on the host: the step counter did not advance
        assert all(lay.opt.state[w]["step"] == ref.ADAMW_STEP0 for w in lay.params)
    for w in lay.params:  # a skipped step is no step
        lay.opt.state[w]["step"] = ref.ADAMW_STEP0
    lay.step(case["g"][0])
    want, norms, coefs = clip_ref.clipped_steps64(case, case["g"][:1], correct_bias, 1.0)
    _assert_norm(lay.opt, norms[0], coefs[0])
    lay.assert_matches(want, "the step after the skipped one")


# ---- 6. two parameter groups ----

def test_two_param_groups_share_one_global_norm_and_keep_their_tables():
    from csa_amd.train import AdamW
    g = torch.Generator().manual_seed(8)
    shapes = [(300, 7), (5000,), (64, 64), (9,)]
    base = [torch.randn(s, generator=g) for s in shapes]
    cpu = [torch.nn.Parameter(t.clone()) for t in base]
    gpu = [torch.nn.Parameter(t.cuda()) for t in base]
    groups = lambda ps: [{"params": ps[:2], "weight_decay": 0.01}, {"params": ps[2:], "weight_decay": 0.0}]
    o_cpu = AdamW(groups(cpu), lr=2e-3, correct_bias=False, max_grad_norm=2.0)
    o_gpu = AdamW(groups(gpu), lr=2e-3, correct_bias=False, max_grad_norm=2.0)
    seen = None
    for step in range(3):
        grads = [torch.randn(s, generator=g) for s in shapes]
        for pc, pg, gr in zip(cpu, gpu, grads):
            if pg.grad is None:
                pc.grad, pg.grad = gr.clone(), gr.cuda()
            else:
                pc.grad.copy_(gr)
                pg.grad.copy_(gr.cuda())
        o_cpu.step()
        o_gpu.step()
        norm = clip_ref.global_norm64([gr.numpy() for gr in grads])  # over both groups
        _assert_norm(o_gpu, norm, clip_ref.clip_coef64(norm, 2.0))
        assert o_gpu.last_clip_coef.item() < 1.0
        now = {k: (id(e["desc"]), id(e["owner"])) for k, e in o_gpu._tables.items()}
        now["clip"] = (id(o_gpu._clip_partials), id(o_gpu._clip_state))
        assert len(now) == 3
        if seen is not None:
            assert now == seen
        seen = now
    for pc, pg in zip(cpu, gpu):
        np.testing.assert_allclose(pg.detach().cpu().numpy(), pc.detach().numpy(), rtol=1e-5, atol=1e-7)


# ---- 7. grad_norm(model.parameters()) ----

def test_grad_norm_of_a_model(golden):
    from csa_amd.model import CSATrans, batch_to_device, label_smoothing_loss
    from csa_amd.train import grad_norm
    from golden_inputs import fill_params_deterministic
    from test_model_gpu import TINY
    z = golden("csatrans_tiny")
    m = CSATrans(**TINY)
    fill_params_deterministic(m, 71)
    m = m.cuda().eval()
    x, y = batch_to_device({k: z[k] for k in ("src_seq", "tgt_seq", "target", "L", "T", "L_mask", "T_mask")},
                           torch.device("cuda"))
    out, sparsity, *_ = m(x)
    (label_smoothing_loss(out, y) + 1e-2 * sparsity).backward()
    got = grad_norm(m.parameters())
    assert got.shape == () and got.is_cuda and got.dtype == torch.float32
    grads = [p.grad.cpu().numpy() for p in m.parameters() if p.grad is not None]
    assert len(grads) > 20
    want = clip_ref.global_norm64(grads)
    assert want > 0.0
    np.testing.assert_allclose(got.item(), want, rtol=clip_ref.NORM_RTOL)
    scale = torch.full((), 1024.0, device="cuda")
    np.testing.assert_allclose(grad_norm(m.parameters(), grad_scale=scale).item(), want / 1024.0, rtol=clip_ref.NORM_RTOL)
