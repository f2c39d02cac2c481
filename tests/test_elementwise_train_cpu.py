"""The cases of test_elementwise_train_gpu.py decide what they are built to decide (tests/elementwise_ref.py):
the sizes fall into the launch classes they are named for, the raw Philox draws hold both neighbours of every
dropout threshold (so `>=` against `>` shows), distinct (seed, offset) pairs give distinct masks, the special
values give the IEEE results the documents state, and every wrong variant of the AdamW step is far outside the
GPU test's tolerance on a large part of the elements."""
import numpy as np
import pytest

import elementwise_ref as ref
from oracle import philox


def test_sizes_fall_into_their_launch_classes():
    assert [ref.drop_launch(n) for n in ref.N_SINGLE] == [(1, 1, 1)] * 8
    assert ref.drop_launch(ref.N_SEVERAL[0]) == (768, 3, 1)
    assert [ref.drop_launch(n) for n in ref.N_SEVERAL[1:]] == [(769, 4, 1)] * 7
    assert sorted(n % 8 for n in ref.N_SINGLE) == sorted(n % 8 for n in ref.N_SEVERAL) == list(range(8))
    groups, blocks, passes = ref.drop_launch(ref.N_WRAP)
    assert (ref.N_WRAP, blocks, passes) == (8391013, 4096, 2)
    second = groups - blocks * ref.WG          # groups of the second pass: one full workgroup and a part of one
    assert second == 301 and second % ref.WG != 0 and ref.N_WRAP % 8 == 5
    assert ref.drop_launch(8 * 256 * 4096) == (1048576, 4096, 1)  # the largest size of one pass
    assert ref.drop_launch(ref.N_KEY) == (769, 4, 1)
    assert (ref.N_WRAP + ref.PAD) * 4 < 34 * 2 ** 20


@pytest.mark.parametrize("stream,keep_fn", [(ref.RES_STREAM, philox.res_keep), (ref.FFN_STREAM, philox.ffn_keep)])
def test_raw_draws_are_those_under_the_oracle_masks(stream, keep_fn):
    for seed in ref.SEEDS:
        for offset in ref.OFFSETS:
            u = ref.flat_u16(ref.N_KEY, seed, offset, stream)
            for p in (0.2, 0.99999):
                assert np.array_equal(ref.keep_of(u, p), keep_fn(ref.N_KEY, seed, offset, p)), (seed, offset, p)
    n0 = ref.N_WRAP - 100000  # the stride-wrap size, checked on its last elements (the second pass among them)
    u = ref.flat_u16(ref.N_WRAP, ref.SEED_THR, ref.OFFSET_THR, stream)[n0:]
    i = np.arange(n0, ref.N_WRAP, dtype=np.int64)
    g = (i >> 3).astype(np.uint64)
    words = philox.philox4x32(g & philox.MASK32, g >> np.uint64(32), 0, (stream << 28) ^ ref.OFFSET_THR,
                              ref.SEED_THR & 0xFFFFFFFF, ref.SEED_THR >> 32)
    assert np.array_equal(u, philox.u16_of(words, i & 7))


@pytest.mark.parametrize("stream", [ref.RES_STREAM, ref.FFN_STREAM])
def test_both_neighbours_of_every_threshold_are_drawn(stream):
    """keep <=> u16 >= thr: a kernel comparing with `>` differs exactly where u16 == thr, and one comparing
    with thr - 1 where u16 == thr - 1. Both values occur in the stride-wrap case, for every threshold below 65536."""
    u = ref.flat_u16(ref.N_WRAP, ref.SEED_THR, ref.OFFSET_THR, stream)
    counts = np.bincount(u, minlength=65536)
    for p, thr in ref.P_THR:
        assert philox.keep_threshold(p) == thr
        if thr <= 65535:
            assert counts[thr] >= 1 and counts[thr - 1] >= 1, (p, thr, counts[thr], counts[thr - 1])
            print(f"stream {stream} thr {thr}: {counts[thr]} draws == thr, {counts[thr - 1]} == thr - 1")
    assert not ref.keep_of(u, 0.99999).any()  # thr 65536: nothing is kept
    if stream == ref.RES_STREAM:
        assert ([(int(counts[t]), int(counts[t - 1])) for _, t in ref.P_THR[:4]]
                == [(128, 126), (133, 121), (145, 120), (152, 124)])


@pytest.mark.parametrize("stream", [ref.RES_STREAM, ref.FFN_STREAM])
def test_distinct_seed_offset_pairs_give_distinct_masks(stream):
    masks = {(s, o): ref.keep_of(ref.flat_u16(ref.N_KEY, s, o, stream), 0.2).tobytes()
             for s in ref.SEEDS for o in ref.OFFSETS}
    assert len(set(masks.values())) == len(ref.SEEDS) * len(ref.OFFSETS) == 20
    # what a kernel that dropped part of the key or the offset would draw instead is a different mask, too
    base = ref.keep_of(ref.flat_u16(ref.N_KEY, ref.SEED_HI, 1, stream), 0.2)
    for seed, offset in ((ref.SEED_HI & ~(3 << 62), 1), (ref.SEED_HI & 0xFFFFFFFF, 1), (ref.SEED_HI, 0)):
        assert not np.array_equal(base, ref.keep_of(ref.flat_u16(ref.N_KEY, seed, offset, stream), 0.2))


def test_residual_special_case_holds_every_pair_kept_and_dropped():
    keep = philox.res_keep(ref.N_KEY, ref.SEED_HI, 1, 0.2)
    x, o = ref.res_special_case(keep, np.random.default_rng(3))
    bits = lambda a: a.view(np.int32)
    for a in ref.SPECIALS:
        for b in ref.SPECIALS:
            at = (bits(x) == bits(np.array([a]))) & (bits(o) == bits(np.array([b])))
            assert (at & keep).any() and (at & ~keep).any(), (a, b)
    y, d = ref.res_fwd(x, o, keep, 0.2), ref.res_bwd(o, keep, 0.2)
    assert y.dtype == d.dtype == np.float32
    sub = np.float32(1e-40)
    k, dr = np.flatnonzero(keep)[0], np.flatnonzero(~keep)[0]
    one = lambda xv, ov, i: ref.res_fwd(np.array([xv], np.float32), np.array([ov], np.float32), keep[i:i + 1], 0.2)[0]
    assert one(0.0, sub, k) == sub * np.float32(1.25) and 0 < one(0.0, sub, k) < np.finfo(np.float32).tiny
    assert bits(np.array([one(-0.0, -sub, dr)]))[0] == bits(np.array([-0.0], np.float32))[0]  # -0 + 0 * -1e-40 = -0
    assert np.isnan(one(1.0, np.inf, dr)) and one(1.0, np.inf, k) == np.inf                    # 0 * inf = NaN
    assert np.isnan(one(-np.inf, ref.FLT_MAX, k)) and one(0.0, ref.FLT_MAX, dr) == 0.0         # FLT_MAX * 1.25 = inf


def test_gelu_oracle_special_values():
    """The IEEE value of h/2 (1 + erf(h / sqrt 2)) and of cdf + h pdf at the ends of the line."""
    h = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 88.0, -88.0], dtype=np.float32)
    one = np.ones(h.size, dtype=bool)
    f, d = ref.gelu_fwd64(h, one, 0.2), ref.gelu_bwd64(np.ones(h.size), h, one, 0.2)
    assert f[0] == np.inf and np.isnan(f[1]) and np.isnan(f[2]) and f[3] == 0 and f[4] == 0
    assert f[5] == 88.0 * float(ref.drop_scale(0.2)) and f[6] == 0
    assert np.isnan(d[:3]).all() and d[3] == d[4] == 0.5 * float(ref.drop_scale(0.2))
    assert d[5] == float(ref.drop_scale(0.2)) and d[6] == 0
    f0, d0 = ref.gelu_fwd64(h, ~one, 0.2), ref.gelu_bwd64(np.ones(h.size), h, ~one, 0.2)
    assert np.isnan(f0[:3]).all() and (f0[3:] == 0).all()       # a dropped +inf is 0 * inf
    assert np.isnan(d0[:3]).all() and (d0[3:] == 0).all()
    x = np.linspace(-6, 6, 101)
    num = (ref.gelu64(x + 1e-6) - ref.gelu64(x - 1e-6)) / 2e-6   # gelu' is the derivative of gelu
    np.testing.assert_allclose(ref.gelu_d64(x), num, rtol=0, atol=1e-9)
    hv = ref.gelu_values(np.random.default_rng(0))
    assert hv.size == 2 ** 16 + len(ref.GELU_FINITE_SPECIALS) and hv.size % 8 == 2 and np.isfinite(hv).all()
    hm, dy = ref.mask_visible_values(4096, np.random.default_rng(1))
    assert np.abs(ref.gelu64(hm)).min() > 1e-3 and np.abs(ref.gelu_d64(hm)).min() > 1e-3 and np.abs(dy).min() >= 0.5


@pytest.mark.parametrize("correct_bias", [False, True])
def test_adamw_mutants_are_far_outside_the_tolerance(correct_bias):
    """Each wrong variant of the step moves more than 100 times the GPU test's tolerance on at least 10 % of
    the parameters, after one step from the test's own state."""
    case = ref.adamw_case()
    p, m, v = (np.concatenate(case[k]) for k in ("p", "m", "v"))
    g = np.concatenate(case["g"][0])
    assert p.size >= 5000 and (m != 0).all() and (v > 0).all()
    assert 1e-2 <= np.abs(g).min() and np.abs(g).max() <= 10 and (g < 0).any() and (g > 0).any()
    t = ref.ADAMW_STEP0 + 1
    want = ref.adamw64(p, m, v, g, t, correct_bias)[0]
    tol = 100 * (ref.ADAMW_ATOL + ref.ADAMW_RTOL * np.abs(want))
    for mutant in ref.MUTANTS:
        if mutant == "no_bias_correction" and not correct_bias:
            continue  # nothing to drop
        frac = float((np.abs(ref.adamw64(p, m, v, g, t, correct_bias, mutant)[0] - want) > tol).mean())
        print(f"correct_bias={correct_bias} {mutant}: {100 * frac:.1f} % of the parameters beyond 100 x tolerance")
        assert frac >= 0.10, (mutant, frac)


def test_adamw_oracle_is_the_reference_step():
    """adamw64 against the per-op CPU path of csa_amd.train.AdamW (the reference's op order in fp32), at its
    rounding; the unscale and the step counter included."""
    import torch
    from csa_amd.train import AdamW
    case = ref.adamw_case(sizes=[257], steps=2)
    for correct_bias in (False, True):
        w = torch.nn.Parameter(torch.from_numpy(case["p"][0].copy()))
        opt = AdamW([w], correct_bias=correct_bias, **ref.ADAMW_HP)
        opt.state[w] = {"step": ref.ADAMW_STEP0, "exp_avg": torch.from_numpy(case["m"][0].copy()),
                        "exp_avg_sq": torch.from_numpy(case["v"][0].copy())}
        opt.grad_scale = torch.tensor(ref.GRAD_SCALE)
        want = (case["p"][0], case["m"][0], case["v"][0])
        for k in range(2):
            w.grad = torch.from_numpy(ref.scaled_grads(case["g"][k])[0])
            opt.step()
            want = ref.adamw64(*want, ref.scaled_grads(case["g"][k])[0], ref.ADAMW_STEP0 + 1 + k, correct_bias,
                               inv_scale=ref.inv_scale32())
        np.testing.assert_allclose(w.detach().numpy(), want[0], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(opt.state[w]["exp_avg"].numpy(), want[1], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(opt.state[w]["exp_avg_sq"].numpy(), want[2], rtol=1e-5, atol=1e-12)
