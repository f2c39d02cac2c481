"""Every launch class of the three elementwise kernels of the train step, against the oracles of
tests/elementwise_ref.py (test_elementwise_train_cpu.py shows that the cases are decisive):

  k_res_drop<BWD>   (csa_glue.hip, through the C ABI: seed, offset and p are free)   bitwise against numpy fp32
  k_gelu_drop<BWD>  (csa_glue.hip, through the C ABI)   mask exact, values against fp64 at rtol 1e-5, atol 1e-5
  k_adamw           (csa_optim.hip, through csa_amd.train.AdamW)   against fp64 at rtol 1e-5, atol 1e-7 (1e-12 for v)

Launch classes of the two dropout kernels. Both launch
    `const unsigned blocks = (unsigned)std::min<int64_t>((groups + 255) / 256, 256 * 16);`
workgroups of 256 threads, one group of 8 elements per thread and pass (`const int64_t groups = (a.n + 7) >> 3;`),
and loop with `g += (int64_t)gridDim.x * 256`; a group takes the dwordx4 path when `i0 + 8 <= a.n`, else the scalar
tail (test_dropout_cases_cover_every_launch_class pins these lines):
  single group        n = 1..8                        one thread; tail lengths 1..7 and one full group
  several workgroups  n = 8 * 256 * 3 + r, r = 0..7   3 full workgroups; for r > 0 the ragged group alone in a 4th
  stride wrap         n = 8 * 256 * 4096 + 8 * 300 + 5   4096 workgroups, a second pass of 301 groups (one full
                                                      workgroup, 45 threads of the next), the last group ragged
Every output buffer is 64 floats longer than n and pre-filled; the whole int32 image is compared, so a store past
n fails. Key and counter: seeds with bits 31, 32, 62 and 63 set and non-zero offsets up to 32 bits, at
n = 8 * 256 * 3 + 5. Thresholds `a.thr = (uint32_t)ceil((double)p * 65536.0)`: 1, 13108, 16384 (p = 0.25), 32768
(p = 0.5) and 65536 (nothing kept) at the stride-wrap size, where the raw draws hold thr and thr - 1.
k_gelu_drop takes `a.thr ? res_keep8<RNG_FFN_DROP>(a, g) : 0xffu`: p = 0 is a class of its own.

Launch classes of k_adamw: one workgroup per chunk of CSA_ADAMW_CHUNK = 4096 elements; within a chunk the dwordx4
path when param, grad and both moments are 16-byte aligned (`const bool vec = ...& 15) == 0;`), with a scalar tail
`if (i + 4 <= n)`, else the scalar path. Sizes 1, 3, 4, 4095, 0, 4096, 4097, 10005, 3 * 4096 + 7, 2 * 4096 as views
into sentinel-filled buffers; the even-indexed views start one float off a 16-byte boundary.

What the file was tried against, each as a hand-made variant of the library: `> a.thr` for `>= a.thr` fails the four
threshold cases below 65536 of both stride-wrap tests and both key tests; `a.off` ignored and `seed_hi` masked to 30
bits fail every test that draws a mask (40 and 41 of the 80 cases); the decay applied before the update fails the six
AdamW cases that have a non-zero update; a grid stride of `gridDim.x * 512` fails all eleven stride-wrap cases, their
second pass being left unwritten. A stride of `gridDim.x * 128` fails nothing and cannot: every group is still visited,
some twice, and the second visit stores the same values again (the kernels write out of place), so it costs time
only."""
import ctypes
import os

import numpy as np
import pytest
import torch

import elementwise_ref as ref
from conftest import PKG, has_gpu
from oracle import philox

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]
RTOL, ATOL = 1e-5, 1e-5  # of test_gelu_dropout_matches_oracle


def _source(name):
    with open(os.path.join(PKG, "csrc", name)) as f:
        return f.read()


def test_dropout_cases_cover_every_launch_class():
    src = _source("csa_glue.hip")
    for line, times in ((ref.LAUNCH_LINE, 2), (ref.STRIDE_LINE, 2), ("const int64_t groups = (a.n + 7) >> 3;", 2),
                        ("__global__ __launch_bounds__(256) void k_res_drop(", 1),
                        ("__global__ __launch_bounds__(256) void k_gelu_drop(", 1), ("if (i0 + 8 <= a.n) {", 1),
                        ("const bool full = i0 + 8 <= a.n;", 1),
                        ("a.thr = (uint32_t)ceil((double)p * 65536.0);", 1),
                        ("a.thr = p > 0.f ? (uint32_t)ceil((double)p * 65536.0) : 0u;", 1),
                        ("const uint32_t keep = a.thr ? res_keep8<RNG_FFN_DROP>(a, g) : 0xffu;", 1),
                        ("(STREAM << 28) ^ a.off}", 1)):
        assert src.count(line) == times, f"csa_glue.hip no longer has `{line}` {times} time(s): restate " \
                                         "elementwise_ref.drop_launch and move the sizes with it"
    assert [ref.drop_launch(n)[1:] for n in ref.N_SINGLE] == [(1, 1)] * 8
    assert [ref.drop_launch(n)[1:] for n in ref.N_SEVERAL] == [(3, 1)] + [(4, 1)] * 7
    assert ref.drop_launch(ref.N_WRAP) == (1048576 + 301, 4096, 2) and ref.N_WRAP % 8 == 5
    src = _source("csa_optim.hip")
    for line in ("const int64_t base = (chunk - chunk_start[t]) * CSA_ADAMW_CHUNK;", "if (i + 4 <= n) {",
                 "const bool vec = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;"):
        assert line in src, f"csa_optim.hip no longer has `{line}`"
    from csa_amd._lib import ADAMW_CHUNK
    assert ADAMW_CHUNK == 4096
    assert {n % 4096 for n in ref.ADAMW_SIZES} >= {0, 1, 3, 4, 4095, 7} and 0 in ref.ADAMW_SIZES[1:-1]


# ---- the C ABI of the dropout kernels ----

def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out(n):
    """An output buffer of n floats and PAD more behind them, all pre-filled with the sentinel."""
    return torch.full((n + ref.PAD,), float(ref.SENTINEL), dtype=torch.float32, device="cuda")


def _dev(a):
    t = torch.from_numpy(np.array(a, dtype=np.float32)).cuda()  # a copy: the shared inputs are read-only
    assert t.data_ptr() % 16 == 0
    return t


def _res_fwd(x, o, n, p, seed, offset):
    from csa_amd._lib import check, lib
    y = _out(n)
    check(lib().csa_residual_dropout_fwd(_ptr(x), _ptr(o), _ptr(y), n, p, seed, offset, _stream()), "res fwd")
    return y


def _res_bwd(dy, n, p, seed, offset):
    from csa_amd._lib import check, lib
    d = _out(n)
    check(lib().csa_residual_dropout_bwd(_ptr(dy), _ptr(d), n, p, seed, offset, _stream()), "res bwd")
    return d


def _gelu_fwd(h, n, p, seed, offset):
    from csa_amd._lib import check, lib
    y = _out(n)
    check(lib().csa_gelu_dropout_fwd(_ptr(h), _ptr(y), n, p, seed, offset, _stream()), "gelu fwd")
    return y


def _gelu_bwd(dy, h, n, p, seed, offset):
    from csa_amd._lib import check, lib
    d = _out(n)
    check(lib().csa_gelu_dropout_bwd(_ptr(dy), _ptr(h), _ptr(d), n, p, seed, offset, _stream()), "gelu bwd")
    return d


def _bits(t):
    return t.view(torch.int32)


def _same_image(got, want_values, what):
    """The whole buffer, sentinels included, holds the bits of the expected image (built on the CPU, compared on
    the device)."""
    want = torch.from_numpy(ref.image(want_values)).cuda()
    if not torch.equal(_bits(got), want):
        bad = (_bits(got) != want).nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {want.numel()} words differ, the first at {i} "
                             f"(n = {want_values.size}): got {got[i].item()!r}, want "
                             f"{np.asarray(want_values)[i] if i < want_values.size else ref.SENTINEL!r}")


def _same_image_nan(got, want_values, what):
    """_same_image where the expected value may be NaN: there any NaN will do (the payload is the hardware's)."""
    want = ref.image(want_values)
    g = _bits(got).cpu().numpy()
    nan = np.zeros(want.size, dtype=bool)
    nan[:want_values.size] = np.isnan(want_values)
    gf = g.view(np.float32)
    assert np.isnan(gf[nan]).all(), f"{what}: {int((~np.isnan(gf[nan])).sum())} expected NaNs are numbers"
    bad = np.flatnonzero((g != want) & ~nan)
    assert bad.size == 0, (f"{what}: {bad.size} words differ, the first at {bad[0]}: got {gf[bad[0]]!r}, want "
                           f"{want.view(np.float32)[bad[0]]!r}")


def _tail_untouched(buf, n, what):
    tail = _bits(buf[n:]).cpu().numpy()
    assert tail.size == ref.PAD and (tail == np.array([ref.SENTINEL]).view(np.int32)[0]).all(), \
        f"{what}: stored past n = {n}"


# ---- A. k_res_drop ----

@pytest.mark.parametrize("n", ref.N_SINGLE + ref.N_SEVERAL)
def test_residual_dropout_small_launch_classes_bitwise(n):
    rng = np.random.default_rng(n)
    x, o = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
    seed, offset, p = ref.SEED_HI, 1, 0.2
    keep = philox.res_keep(n, seed, offset, p)
    xd, od = _dev(x), _dev(o)
    y = _res_fwd(xd, od, n, p, seed, offset)
    _same_image(y, ref.res_fwd(x, o, keep, p), f"fwd n={n}")
    d = _res_bwd(od, n, p, seed, offset)
    _same_image(d, ref.res_bwd(o, keep, p), f"bwd n={n}")
    assert torch.equal(_bits(_res_fwd(xd, od, n, p, seed, offset)), _bits(y))  # two runs, the same bits
    assert torch.equal(_bits(_res_bwd(od, n, p, seed, offset)), _bits(d))


@pytest.mark.parametrize("p,thr", ref.P_THR)
def test_residual_dropout_stride_wrap_and_thresholds_bitwise(p, thr):
    """The second pass of the grid-stride loop, at every threshold class (p = 0.2 is the train step's)."""
    n, seed, offset = ref.N_WRAP, ref.SEED_THR, ref.OFFSET_THR
    assert ref.drop_launch(n)[2] == 2 and philox.keep_threshold(p) == thr
    x, o = ref.wrap_inputs()
    keep = ref.keep_of(ref.flat_u16(n, seed, offset, ref.RES_STREAM), p)
    assert keep.any() == (thr < 65536)
    xd, od = _dev(x), _dev(o)
    y = _res_fwd(xd, od, n, p, seed, offset)
    _same_image(y, ref.res_fwd(x, o, keep, p), f"fwd p={p}")
    d = _res_bwd(xd, n, p, seed, offset)
    _same_image(d, ref.res_bwd(x, keep, p), f"bwd p={p}")
    if thr == 65536:  # every element dropped: y == x + 0 * o
        assert torch.equal(_bits(y[:n]), _bits(xd + 0.0 * od)) and not bool(d[:n].any())
    if p == 0.2:
        assert torch.equal(_bits(_res_fwd(xd, od, n, p, seed, offset)), _bits(y))


def test_residual_dropout_key_and_counter_words():
    """All 64 bits of the seed and the low 32 of the offset: each (seed, offset) pair gives the oracle's mask, and
    the 20 masks differ from each other."""
    n, p = ref.N_KEY, 0.2
    rng = np.random.default_rng(1)
    x, o = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
    assert (o != 0).all()
    xd, od = _dev(x), _dev(o)
    masks = set()
    for seed in ref.SEEDS:
        for offset in ref.OFFSETS:
            keep = philox.res_keep(n, seed, offset, p)
            _same_image(_res_fwd(xd, od, n, p, seed, offset), ref.res_fwd(x, o, keep, p), f"fwd {seed:#x} {offset:#x}")
            d = _res_bwd(od, n, p, seed, offset)
            _same_image(d, ref.res_bwd(o, keep, p), f"bwd {seed:#x} {offset:#x}")
            masks.add((d[:n] != 0).cpu().numpy().tobytes())
    assert len(masks) == len(ref.SEEDS) * len(ref.OFFSETS)


def test_residual_dropout_special_values_bitwise():
    """+-inf, NaN, +-0, fp32 subnormals and +-FLT_MAX in x and o, every pair at a kept and at a dropped position: the
    bits of numpy's fp32 (subnormal products included: the kernel does not flush them), NaN where numpy has NaN."""
    n, seed, offset, p = ref.N_KEY, ref.SEED_HI, 1, 0.2
    keep = philox.res_keep(n, seed, offset, p)
    x, o = ref.res_special_case(keep, np.random.default_rng(3))
    want = ref.res_fwd(x, o, keep, p)
    sub = np.abs(want) < np.finfo(np.float32).tiny
    assert np.isnan(want).any() and np.isinf(want).any() and (sub & (want != 0)).any()
    _same_image_nan(_res_fwd(_dev(x), _dev(o), n, p, seed, offset), want, "fwd")
    _same_image_nan(_res_bwd(_dev(o), n, p, seed, offset), ref.res_bwd(o, keep, p), "bwd")


# ---- B. k_gelu_drop ----

def _close64(got, want, what):
    got = got.cpu().numpy().astype(np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern"
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), f"{what}: infinities"
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=ATOL, err_msg=what)


def _gelu_mask_case(n, p, seed, offset, h, dy, what):
    """Forward and backward on values whose outputs are 0 only where dropped: the zero pattern is the oracle mask
    exactly, the values are fp64's within tolerance, nothing behind n is stored."""
    if p == 0:
        keep = np.ones(n, dtype=bool)
    elif n == ref.N_WRAP:  # one cached stream of raw draws for all thresholds
        keep = ref.keep_of(ref.flat_u16(n, seed, offset, ref.FFN_STREAM), p)
    else:
        keep = philox.ffn_keep(n, seed, offset, p)
    hd, dyd = _dev(h), _dev(dy)
    y = _gelu_fwd(hd, n, p, seed, offset)
    d = _gelu_bwd(dyd, hd, n, p, seed, offset)
    for name, out, want in (("fwd", y, ref.gelu_fwd64(h, keep, p)), ("bwd", d, ref.gelu_bwd64(dy, h, keep, p))):
        _tail_untouched(out, n, f"{what} {name}")
        kept = (out[:n] != 0).cpu().numpy()
        assert np.array_equal(kept, keep), f"{what} {name}: {int((kept != keep).sum())} mask bits differ"
        _close64(out[:n], want, f"{what} {name}")
    return y, d


@pytest.mark.parametrize("p", [0.2, 0.0])
@pytest.mark.parametrize("n", ref.N_SINGLE + ref.N_SEVERAL)
def test_gelu_dropout_small_launch_classes(n, p):
    h, dy = ref.mask_visible_values(n, np.random.default_rng(100 + n))
    y, d = _gelu_mask_case(n, p, ref.SEED_HI, 1, h, dy, f"n={n} p={p}")
    y2, d2 = _gelu_fwd(_dev(h), n, p, ref.SEED_HI, 1), _gelu_bwd(_dev(dy), _dev(h), n, p, ref.SEED_HI, 1)
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(d2), _bits(d))


_WRAP_GELU = []


def _wrap_gelu_inputs():
    if not _WRAP_GELU:
        _WRAP_GELU.extend(ref.mask_visible_values(ref.N_WRAP, np.random.default_rng(21)))
    return _WRAP_GELU


@pytest.mark.parametrize("p,thr", ref.P_THR + [(0.0, 0)])
def test_gelu_dropout_stride_wrap_and_thresholds(p, thr):
    n = ref.N_WRAP
    h, dy = _wrap_gelu_inputs()
    y, d = _gelu_mask_case(n, p, ref.SEED_THR, ref.OFFSET_THR, h, dy, f"p={p}")
    if thr == 65536:
        assert not bool(y[:n].any()) and not bool(d[:n].any())


def test_gelu_dropout_key_and_counter_words():
    n = ref.N_KEY
    h, dy = ref.mask_visible_values(n, np.random.default_rng(2))
    fwd, bwd, plain = set(), set(), set()
    for seed in ref.SEEDS:
        for offset in ref.OFFSETS:
            y, d = _gelu_mask_case(n, 0.2, seed, offset, h, dy, f"{seed:#x} {offset:#x}")
            fwd.add((y[:n] != 0).cpu().numpy().tobytes())
            bwd.add((d[:n] != 0).cpu().numpy().tobytes())
            y0, d0 = _gelu_fwd(_dev(h), n, 0.0, seed, offset), _gelu_bwd(_dev(dy), _dev(h), n, 0.0, seed, offset)
            plain.add(_bits(y0).cpu().numpy().tobytes() + _bits(d0).cpu().numpy().tobytes())
    assert len(fwd) == len(bwd) == len(ref.SEEDS) * len(ref.OFFSETS)
    assert len(plain) == 1  # p = 0 reads neither the seed nor the offset


@pytest.mark.parametrize("p", [0.2, 0.0])
def test_gelu_dropout_values_match_fp64(p):
    """h over [-14, 14] in 2^16 steps with +-0, +-1e-40, +-1e-30, +-40 and +-88 among them."""
    h = ref.gelu_values(np.random.default_rng(5))
    n = h.size
    dy = np.random.default_rng(6).standard_normal(n, dtype=np.float32)
    seed, offset = ref.SEED_HI, 0xDEADBEEF
    keep = philox.ffn_keep(n, seed, offset, p) if p > 0 else np.ones(n, dtype=bool)
    hd = _dev(h)
    y, d = _gelu_fwd(hd, n, p, seed, offset), _gelu_bwd(_dev(dy), hd, n, p, seed, offset)
    _tail_untouched(y, n, "fwd")
    _tail_untouched(d, n, "bwd")
    _close64(y[:n], ref.gelu_fwd64(h, keep, p), "fwd")
    _close64(d[:n], ref.gelu_bwd64(dy, h, keep, p), "bwd")
    big = np.abs(h) >= 1.0  # where gelu and (for most h) gelu' are visible, the zeros are the mask's
    assert np.array_equal((y[:n] != 0).cpu().numpy()[big & (h > -5)], keep[big & (h > -5)])


def test_gelu_negative_tail_is_as_accurate_as_torch_fp32():
    """h in [-14, -4], where |gelu| < 1.3e-4 and every value is inside the atol of the tests above: the kernel's maximum
    absolute error against fp64, forward and derivative, is within 4 times that of torch's fp32 gelu and its autograd
    on the CPU at the same inputs (the method and the factor of test_layernorm_ill_conditioned_rows, without its
    atol floor, which would hide the tail again). Both errors are printed; on an MI355X: gelu 8.3e-08 against 4.1e-07,
    gelu' 1.5e-08 against 4.4e-08."""
    h = np.linspace(-14.0, -4.0, 2 ** 16).astype(np.float32)
    n = h.size
    one = np.ones(n, dtype=np.float32)
    hd = _dev(h)
    y = _gelu_fwd(hd, n, 0.0, 0, 0)[:n].cpu().numpy().astype(np.float64)
    d = _gelu_bwd(_dev(one), hd, n, 0.0, 0, 0)[:n].cpu().numpy().astype(np.float64)
    ht = torch.from_numpy(h.copy()).requires_grad_(True)
    yt = torch.nn.functional.gelu(ht)
    yt.backward(torch.ones(n))
    for name, got, cpu, want in (("gelu", y, yt.detach().numpy(), ref.gelu64(h)),
                                 ("gelu'", d, ht.grad.numpy(), ref.gelu_d64(h))):
        e_kernel = float(np.abs(got - want).max())
        e_cpu = float(np.abs(cpu.astype(np.float64) - want).max())
        msg = f"{name} on [-14, -4]: kernel max error {e_kernel:.3e}, fp32 CPU torch max error {e_cpu:.3e}"
        print(msg)
        assert e_cpu > 0 and e_kernel <= 4 * e_cpu, msg


def test_gelu_dropout_non_finite_h():
    """The IEEE value of the documented formulas at kept and at dropped positions: gelu(+inf) = +inf (0 * inf = NaN
    where dropped), gelu(-inf) = NaN, gelu'(+-inf) = NaN, NaN stays NaN; the neighbours are untouched."""
    n, seed, offset, p = 2 ** 10 + 3, ref.SEED_HI, 1, 0.2
    keep = philox.ffn_keep(n, seed, offset, p)
    h, dy = ref.mask_visible_values(n, np.random.default_rng(9))
    kept, dropped = np.flatnonzero(keep), np.flatnonzero(~keep)
    vals = np.array([np.inf, -np.inf, np.nan], dtype=np.float32)
    h[kept[:3]], h[dropped[:3]] = vals, vals
    h[n - 1] = np.inf  # in the ragged tail
    hd = _dev(h)
    for pp, kp in ((p, keep), (0.0, np.ones(n, dtype=bool))):
        y, d = _gelu_fwd(hd, n, pp, seed, offset), _gelu_bwd(_dev(dy), hd, n, pp, seed, offset)
        _tail_untouched(y, n, "fwd")
        _tail_untouched(d, n, "bwd")
        _close64(y[:n], ref.gelu_fwd64(h, kp, pp), f"fwd p={pp}")
        _close64(d[:n], ref.gelu_bwd64(dy, h, kp, pp), f"bwd p={pp}")
    yk = _gelu_fwd(hd, n, p, seed, offset).cpu().numpy()
    assert yk[kept[0]] == np.inf and np.isnan(yk[dropped[0]]) and np.isnan(yk[kept[1]]) and np.isnan(yk[kept[2]])
    dk = _gelu_bwd(_dev(dy), hd, n, p, seed, offset).cpu().numpy()
    assert np.isnan(dk[np.concatenate([kept[:3], dropped[:3]])]).all() and np.isnan(dk[:n]).sum() == 7


# ---- C. the autograd wrappers ----

def _offset_view(x_mem):
    """x_mem's values in a contiguous CUDA tensor of its shape that starts one float into an allocation."""
    buf = torch.empty(x_mem.numel() + 8, dtype=torch.float32, device="cuda")
    v = buf[1:1 + x_mem.numel()].view(x_mem.shape)
    v.copy_(x_mem)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("batch_major", [False, True])
@pytest.mark.parametrize("op", ["residual_dropout", "gelu_dropout"])
def test_misaligned_upstream_gradient_gives_the_aligned_gradients(op, batch_major):
    """An upstream gradient that is contiguous in the forward's memory order but starts 4 bytes into an allocation:
    the backward hands the kernel an aligned copy, and the gradients are those of the aligned call, bit for bit."""
    from csa_amd import glue
    drop = torch.nn.Dropout(0.2).train()
    mem = (5, 7, 12)  # 420 elements: a ragged last group
    g = torch.Generator().manual_seed(4)
    to_logical = (lambda t: t.transpose(0, 1)) if batch_major else (lambda t: t)
    x_mem, o_mem, gy_mem = (torch.randn(*mem, generator=g).cuda() for _ in range(3))

    def run(gy):
        seen = []
        x = to_logical(x_mem.clone()).detach().requires_grad_(True)
        o = to_logical(o_mem.clone()).detach().requires_grad_(True)
        torch.manual_seed(33)
        y = glue.residual_dropout(x, o, drop) if op == "residual_dropout" else glue.gelu_dropout(o, drop)
        assert y.grad_fn is not None and type(y.grad_fn).__name__.endswith("DropoutFnBackward")
        y.register_hook(lambda t: seen.append(t.data_ptr()))
        y.backward(gy)
        assert seen == [gy.data_ptr()]  # the backward is handed this very tensor
        return [t.grad.clone() for t in ((x, o) if op == "residual_dropout" else (o,))]

    want = run(to_logical(gy_mem.clone()))
    got = run(to_logical(_offset_view(gy_mem)))
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))
    assert bool((want[-1] == 0).any()) and bool((want[-1] != 0).any())  # a dropout mask was applied


def test_empty_tensor_goes_forward_and_backward():
    from csa_amd import glue
    drop = torch.nn.Dropout(0.2).train()
    x = torch.empty(0, 5, 8, device="cuda", requires_grad=True)
    o = torch.empty(0, 5, 8, device="cuda", requires_grad=True)
    y = glue.residual_dropout(x, o, drop)
    z = glue.gelu_dropout(o, drop)
    assert y.shape == z.shape == (0, 5, 8)
    (y + z).backward(torch.empty(0, 5, 8, device="cuda"))
    assert x.grad.shape == o.grad.shape == (0, 5, 8)


# ---- D. k_adamw ----

GUARD = 8  # sentinel floats in front of and behind every view (one more in front of the offset ones)


def _guarded(a, shift):
    """a's values as a view into a sentinel-filled device buffer, starting 4 * shift bytes off a 16-byte boundary."""
    n = a.size
    buf = torch.full((n + 2 * GUARD + 1,), float(ref.SENTINEL), dtype=torch.float32, device="cuda")
    view = buf[GUARD + shift:GUARD + shift + n]
    view.copy_(torch.from_numpy(a))
    assert n == 0 or view.data_ptr() % 16 == 4 * shift
    return buf, view


class _AdamwLayout:
    """The case's parameters, gradients and moments as guarded views; even-indexed tensors one float off."""

    def __init__(self, case, correct_bias, with_state=True):
        from csa_amd.train import AdamW
        self.bufs, self.views = {}, {}
        for key in ("p", "g", "m", "v"):
            src = case["g"][0] if key == "g" else case[key]
            pairs = [_guarded(a, 1 if i % 2 == 0 else 0) for i, a in enumerate(src)]
            self.bufs[key], self.views[key] = [b for b, _ in pairs], [v for _, v in pairs]
        self.params = [torch.nn.Parameter(v) for v in self.views["p"]]
        for w, v, gv in zip(self.params, self.views["p"], self.views["g"]):
            assert w.data_ptr() == v.data_ptr()
            w.grad = gv
        self.opt = AdamW(self.params, correct_bias=correct_bias, **ref.ADAMW_HP)
        if with_state:
            for w, m, v in zip(self.params, self.views["m"], self.views["v"]):
                self.opt.state[w] = {"step": ref.ADAMW_STEP0, "exp_avg": m, "exp_avg_sq": v}

    def set_grads(self, grads):
        for gv, a in zip(self.views["g"], grads):
            gv.copy_(torch.from_numpy(a))

    def snapshot(self):
        return {k: [b.clone() for b in bs] for k, bs in self.bufs.items()}

    def assert_guards(self):
        s = np.array([ref.SENTINEL]).view(np.int32)[0]
        for key, bufs in self.bufs.items():
            for i, (b, v) in enumerate(zip(bufs, self.views[key])):
                lo = v.storage_offset()
                img = _bits(b).cpu().numpy()
                assert (img[:lo] == s).all() and (img[lo + v.numel():] == s).all(), f"{key}[{i}]: a guard changed"

    def assert_matches(self, want_p, want_m, want_v, what):
        self.assert_guards()
        for i, w in enumerate(self.params):
            st = self.opt.state[w]
            assert st["exp_avg"].data_ptr() == self.views["m"][i].data_ptr()
            for name, got, want, atol in (("p", w.detach(), want_p[i], ref.ADAMW_ATOL),
                                          ("exp_avg", st["exp_avg"], want_m[i], ref.ADAMW_ATOL),
                                          ("exp_avg_sq", st["exp_avg_sq"], want_v[i], ref.ADAMW_ATOL_V)):
                np.testing.assert_allclose(got.cpu().numpy(), want, rtol=ref.ADAMW_RTOL, atol=atol,
                                           err_msg=f"{what}: {name} of tensor {i} ({want.size} elements)")


def _oracle_steps(case, grads_per_step, correct_bias, inv_scale=1.0, t0=ref.ADAMW_STEP0):
    state = [(p, m, v) for p, m, v in zip(case["p"], case["m"], case["v"])]
    for k, grads in enumerate(grads_per_step):
        state = [ref.adamw64(*s, g, t0 + 1 + k, correct_bias, inv_scale=inv_scale) for s, g in zip(state, grads)]
    return [[s[j] for s in state] for j in range(3)]


@pytest.mark.parametrize("steps", [1, 4])
@pytest.mark.parametrize("correct_bias", [False, True])
def test_adamw_matches_fp64_from_a_non_zero_state(correct_bias, steps):
    case = ref.adamw_case()
    lay = _AdamwLayout(case, correct_bias)
    for k in range(steps):
        lay.set_grads(case["g"][k])
        lay.opt.step()
    lay.assert_matches(*_oracle_steps(case, case["g"][:steps], correct_bias), f"{steps} step(s)")


@pytest.mark.parametrize("correct_bias", [False, True])
def test_adamw_grad_scale_and_found_inf(correct_bias):
    """grad_scale = 3073 (no power of two: 1 / scale rounds) and found_inf as GradScaler sets them. With found_inf = 1
    and an inf and a NaN among the gradients, every buffer keeps its bits; the next step, with found_inf = 0, is the
    oracle's step 4 on gradients unscaled by fl32(1 / 3073)."""
    case = ref.adamw_case()
    lay = _AdamwLayout(case, correct_bias)
    scaled = ref.scaled_grads(case["g"][0])
    bad = [g.copy() for g in scaled]
    bad[7][9000], bad[2][1], bad[9][4097] = np.inf, np.nan, -np.inf  # several tensors, several chunks
    lay.set_grads(bad)
    lay.opt.grad_scale = torch.full((), ref.GRAD_SCALE, device="cuda")
    lay.opt.found_inf = torch.full((), 1.0, device="cuda")
    before = lay.snapshot()
    lay.opt.step()
    for key, bufs in lay.bufs.items():
        for i, (b, b0) in enumerate(zip(bufs, before[key])):
            assert torch.equal(_bits(b), _bits(b0)), f"found_inf = 1 changed {key}[{i}]"
    lay.set_grads(scaled)
    lay.opt.found_inf = torch.full((), 0.0, device="cuda")
    for w in lay.params:  # a skipped step is no step: the bias correction is that of step 4
        lay.opt.state[w]["step"] = ref.ADAMW_STEP0
    lay.opt.step()
    lay.assert_matches(*_oracle_steps(case, [scaled], correct_bias, inv_scale=ref.inv_scale32()), "unscaled step")


@pytest.mark.parametrize("correct_bias", [False, True])
def test_adamw_zero_gradient_on_zero_state_only_decays(correct_bias):
    """g = 0 on m = v = 0 with eps > 0: 0 / (0 + eps) = 0, so the parameter changes by the decoupled decay alone and
    the moments stay exact zeros."""
    case = ref.adamw_case()
    zeros = [np.zeros_like(a) for a in case["p"]]
    zcase = dict(p=case["p"], m=zeros, v=zeros, g=[zeros])
    lay = _AdamwLayout(zcase, correct_bias, with_state=False)
    lay.opt.step()
    lay.assert_guards()
    d = ref.ADAMW_HP["lr"] * ref.ADAMW_HP["weight_decay"]
    for w, p0 in zip(lay.params, case["p"]):
        st = lay.opt.state[w]
        assert st["step"] == 1 and not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any())
        np.testing.assert_allclose(w.detach().cpu().numpy(), p0.astype(np.float64) * (1.0 - d),
                                   rtol=ref.ADAMW_RTOL, atol=ref.ADAMW_ATOL)
        assert p0.size == 0 or not np.array_equal(w.detach().cpu().numpy(), p0)
