"""Sampled decoding without a GPU: the torch fallback of csa_amd.decode_ops.sample_rows against the fp64 oracle
(tests/sample_ref.py) on hand-built rows, the distribution of its draws, SamplingGenerator.sample on the fallback path
against the uncached oracle, and the host-side validation of csa_sample_rows. Every fixture is decisive on the oracle
(no draw and no class boundary inside its window), so tokens compare exactly."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sample_ref
from sample_ref import (ATOL, EOS_ID, PAD, RTOL, assert_decisive, assert_matches, filter_np, hand_rows, run_op,
                        sample_rows_np, sampling_ref, search_case)

T = sample_ref.KERNEL_T


def test_filters_on_hand_built_rows_keep_what_the_rule_says():
    z = hand_rows()
    keep = lambda **kw: [sorted(np.nonzero(r)[0].tolist()) for r in filter_np(z, **kw).keep]
    assert keep()[2] == [1, 3, 5, 7, 9] and keep()[3] == []          # -inf and NaN are never candidates
    assert keep(top_k=2)[1] == [1, 3, 4, 7]                          # all ties at the 2nd largest stay
    assert keep(top_k=1)[1] == [3] and keep(top_k=1)[0] == [2]
    assert keep(top_k=11)[0] == sorted(set(range(12)) - {6})         # V - 1
    assert keep(top_k=12)[0] == list(range(12)) and keep(top_k=15)[0] == list(range(12))  # V and V + 3: off
    assert keep(top_k=5)[2] == [1, 3, 5, 7, 9] and keep(top_k=2)[5] == [3, 8]   # no fewer candidates than top_k: off
    assert keep(top_p=1e-3)[4] == [1] and keep(top_p=1e-3)[1] == [3]  # only the maximal class survives
    assert keep(top_p=0.5)[4] == [1, 4, 6]                           # G = .4 < .5: the whole tie class stays
    assert keep(top_p=0.85)[4] == [1, 4, 6, 9, 10]                   # G = .8 < .85
    assert keep(top_p=0.75)[4] == [1, 4, 6]
    assert keep(top_k=2, top_p=0.75)[4] == [1, 4, 6]                 # top-p on the renormalised top-k set: G = 1/2
    assert keep(top_k=2, top_p=0.45)[4] == [1]


@pytest.mark.parametrize("tau", [0.05, 1.0, 5.0])
@pytest.mark.parametrize("top_k", [0, 1, 2, 11, 12, 15])
def test_fallback_on_hand_built_rows(tau, top_k):
    z = hand_rows()
    for top_p in (1.0, 1e-3, 0.45, 0.85):  # off, the maximal class alone, inside a tie class, wide
        for t in (0, 3, T - 2):
            kw = dict(temperature=tau, top_k=top_k, top_p=top_p)
            want = sample_rows_np(z, t, 11, eos_id=EOS_ID, **kw)
            what = f"tau={tau} top_k={top_k} top_p={top_p} t={t}"
            assert_decisive(want, what)
            got = run_op(z, t, 11, eos_id=EOS_ID, **kw)
            assert_matches(got, want, what)
            assert got.tok[3] == 0 and got.logp[3] == -np.inf  # the all -inf row
            if tau == 1.0:
                assert np.array_equal(filter_np(z, **kw).y[0], z[0])  # temperature 1 leaves the logits as they are
            other = [c for c in range(T) if c != t + 1]
            assert bool((got.ys[:, other] == 99).all()) and bool((got.pads[:, other] == 7).all())
            assert bool((got.logps[:, [c for c in range(T - 1) if c != t]] == 5.0).all())


def test_finished_rows_eos_and_pad_bytes():
    z = hand_rows()
    fin = np.array([0, 1, 0, 0, 1, 0], dtype=np.uint8)
    want = sample_rows_np(z, 2, 11, fin=fin, eos_id=7)
    assert_decisive(want)
    assert want.tok[2] == 7 and want.fin.tolist() == [0, 1, 1, 0, 1, 0]  # row 2 draws its EOS here
    got = run_op(z, 2, 11, fin=fin, eos_id=7)
    assert_matches(got, want, "finished rows")
    assert got.tok[[1, 4]].tolist() == [PAD, PAD] and got.logp[[1, 4]].tolist() == [0.0, 0.0]
    assert got.pad.tolist() == [0, 1, 0, 1, 1, 0]  # the all -inf row's index 0 is PAD as well
    never = run_op(z, 2, 11, fin=fin, eos_id=None)
    assert never.fin.tolist() == fin.tolist() and np.array_equal(never.tok, got.tok)
    assert run_op(z, 2, 11, logp=False).logp is None


def test_fallback_noise_is_the_oracles_philox_stream():
    from csa_amd.decode_ops import _sample_gumbel
    for seed, offset in ((11, 0), (0xFEDCBA9876543210, 0x1234567890)):
        g = _sample_gumbel(5, 37, 6, seed, offset, torch.device("cpu")).numpy()
        np.testing.assert_allclose(g, sample_ref.gumbel_np(5, 37, 6, seed, offset), rtol=1e-5, atol=1e-6)
    assert not np.allclose(sample_ref.gumbel_np(2, 8, 1, 5), sample_ref.gumbel_np(2, 8, 2, 5))


def test_draws_follow_the_softmax():
    """20000 rows of one 8-entry logit vector in one call: Pearson chi-square of the counts against the softmax of the
    unfiltered set (7 degrees of freedom) and of the top_k = 3 set (2), below the 99.9 % critical values. Seed 6 was
    chosen on the oracle alone (decisive, chi-square 9.92 and 2.16)."""
    v = np.array([1.2, -0.3, 0.4, 2.0, -1.5, 0.9, 0.0, 1.6], dtype=np.float32)
    n = 20000
    z = np.tile(v, (n, 1))
    for top_k, crit in ((0, 24.32), (3, 13.82)):
        want = sample_rows_np(z, 2, 6, top_k=top_k)
        assert_decisive(want)
        got = run_op(z, 2, 6, top_k=top_k)
        np.testing.assert_array_equal(got.tok, want.tok)
        keep = filter_np(z[:1], top_k=top_k).keep[0]
        assert int(keep.sum()) == (3 if top_k else 8)
        p = np.where(keep, np.exp(v.astype(np.float64)), 0.0)
        p /= p.sum()
        counts = np.bincount(got.tok, minlength=8)
        assert counts[~keep].sum() == 0
        chi2 = float(((counts[keep] - n * p[keep]) ** 2 / (n * p[keep])).sum())
        print(f"top_k={top_k} chi2={chi2:.3f}")
        assert chi2 < crit
        np.testing.assert_allclose(got.logp, np.log(p[got.tok]), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("S,kw,seed", sample_ref.GENERATOR_CASES, ids=sample_ref.GENERATOR_IDS)
def test_generator_on_the_fallback_path_matches_the_oracle(S, kw, seed):
    from csa_amd.model import SamplingGenerator
    m, enc, src_mask = search_case()
    ref = sampling_ref(m, enc, src_mask, T, S, seed, **kw)
    print(f"S={S} {kw} draw_gap={ref.draw_gap[0]:.5f} nuc_gap={ref.nuc_gap[0]:.5f}")
    assert_decisive(ref)
    assert bool(ref.fin[:-1].any()), "no row finished before the last step"
    if S > 1:
        assert bool((ref.ids[:, 0] != ref.ids[:, 1]).any()), "the samples of an AST are all equal"
    gen = SamplingGenerator(m, T, num_samples=S, graph=True, **kw)  # no CUDA model: nothing is captured
    ids, logp = gen.sample(enc, src_mask, seed=seed, return_logp=True)
    assert gen.captures == 0
    shape = (3, T - 1) if S == 1 else (3, S, T - 1)
    assert ids.shape == shape and logp.shape == shape and ids.dtype == torch.int64 and logp.dtype == torch.float32
    assert torch.equal(ids, ref.ids)
    np.testing.assert_allclose(logp.numpy(), ref.logp, rtol=RTOL, atol=ATOL)
    after_eos = (ids == EOS_ID).cumsum(-1) - (ids == EOS_ID).int() > 0
    assert bool(after_eos.any())
    assert bool((ids[after_eos] == PAD).all()) and bool((logp[after_eos] == 0).all())  # PAD, logp 0 after EOS
    assert bool((logp[~after_eos] <= 0).all()) and bool((logp[~after_eos] < 0).any())
    assert torch.equal(gen.sample(enc, src_mask, seed=seed), ids)  # the same seed repeats
    assert not torch.equal(gen.sample(enc, src_mask, seed=seed + 1), ids)


def test_seed_none_draws_from_the_cpu_generator():
    from csa_amd.model import SamplingGenerator
    m, enc, src_mask = search_case()
    gen = SamplingGenerator(m, T, num_samples=2)
    torch.manual_seed(5)
    a = gen.sample(enc, src_mask)
    b = gen.sample(enc, src_mask)
    torch.manual_seed(5)
    assert torch.equal(gen.sample(enc, src_mask), a) and not torch.equal(a, b)
    big = gen.sample(enc, src_mask, seed=2 ** 64 - 3)  # a key with its top bit set
    assert torch.equal(big, sampling_ref(m, enc, src_mask, T, 2, 2 ** 64 - 3).ids)


def test_top_k_of_one_is_the_cached_greedy_generator():
    from csa_amd.model import CachedGreedyGenerator, SamplingGenerator
    m, enc, src_mask = search_case(seed=16, gen_scale=3.0, eos_bias=-4.0)
    m.process_data = lambda data: setattr(data, "src_mask", src_mask)
    m.encode = lambda data: (enc, 1, None, [], [])
    want = CachedGreedyGenerator(m, T)(SimpleNamespace())
    # greedy key-pads its heads the reference's way, which differs only where a PAD was emitted
    assert not bool((want == PAD).any())
    got, logp = SamplingGenerator(m, T, top_k=1, eos_id=None)(SimpleNamespace(), seed=3, return_logp=True)
    assert torch.equal(got, want) and bool((logp == 0).all())  # one entry kept: its probability is 1
    cold = SamplingGenerator(m, T, temperature=0.05, eos_id=None)(SimpleNamespace(), seed=3)
    assert cold.shape == want.shape


def test_training_mode_and_bad_parameters_raise():
    from csa_amd.model import SamplingGenerator
    m, enc, src_mask = search_case()
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_k=-1), dict(top_k=2.5), dict(top_p=0.0),
               dict(top_p=-0.5), dict(num_samples=0), dict(num_samples=1.5)):
        with pytest.raises(ValueError):
            SamplingGenerator(m, T, **kw)
    with pytest.raises(ValueError):
        SamplingGenerator(m, 1)
    gen = SamplingGenerator(m.train(), T)
    with pytest.raises(RuntimeError):
        gen.sample(enc, src_mask)
    with pytest.raises(RuntimeError):
        gen(SimpleNamespace())


def test_sample_rows_checks_its_arguments():
    from csa_amd.decode_ops import sample_rows
    z = torch.zeros(4, 9)
    ok = lambda: dict(ys=torch.zeros(4, T, dtype=torch.long), pad=torch.zeros(4, T, dtype=torch.uint8),
                      fin=torch.zeros(4, dtype=torch.uint8), t_dev=torch.zeros(1, dtype=torch.int32),
                      rng=torch.zeros(2, dtype=torch.int64))
    sample_rows(z, **ok())
    for name, bad in (("ys", torch.zeros(4, T, dtype=torch.int32)), ("ys", torch.zeros(3, T, dtype=torch.long)),
                      ("pad", torch.zeros(4, T - 1, dtype=torch.uint8)), ("fin", torch.zeros(4, dtype=torch.bool)),
                      ("fin", torch.zeros(5, dtype=torch.uint8)), ("t_dev", torch.zeros(1, dtype=torch.int64)),
                      ("rng", torch.zeros(2, dtype=torch.int32)), ("rng", torch.zeros(3, dtype=torch.int64)),
                      ("logp", torch.zeros(4, T)), ("logp", torch.zeros(4, T - 1, dtype=torch.float64)),
                      ("temperature", 0.0), ("top_k", -2), ("top_p", 0.0)):
        with pytest.raises(ValueError):
            sample_rows(z, **{**ok(), name: bad})
    for t in (-1, T - 1, 1000):  # the host sees the counter here
        with pytest.raises(ValueError):
            sample_rows(z, **{**ok(), "t_dev": torch.tensor([t], dtype=torch.int32)})


def test_cache_group_without_ancestry():
    from csa_amd import model
    dec = model.BaseDecoder(model.DecoderLayer(32, 4, 64, 0.1), 1)
    cache = dec.make_cache(torch.zeros(2, 5, 32), None, 6, group=3)
    assert cache.self_k[0].shape == (6, 4, 6, 8) and cache.memory_kv[0].shape == (2, 5, 2, 4, 8)
    assert cache.anc is None and cache.head_pad is None and cache.kv_group == 3 and cache.pad.shape == (6, 6)
    assert dec.make_cache(torch.zeros(2, 5, 32), None, 6).kv_group == 1  # the default is unchanged
    for kw in (dict(group=0), dict(group=2, beam=2), dict(group=2, repeat_heads=True)):
        with pytest.raises(ValueError):
            dec.make_cache(torch.zeros(2, 5, 32), None, 6, **kw)
    assert issubclass(model.SamplingGenerator, torch.nn.Module)
    assert not issubclass(model.SamplingGenerator, model.GreedyGenerator)


def test_sample_entry_point_validates_without_gpu():
    from csa_amd import _lib
    L = _lib.lib()
    err = L.csa_last_error_str
    assert L.csa_abi_version() == 10
    assert L.csa_sample_rows_supported(1) and L.csa_sample_rows_supported(32768) and L.csa_sample_rows_supported(4100)
    assert not L.csa_sample_rows_supported(0) and not L.csa_sample_rows_supported(32769)
    assert L.csa_sample_rows(None, None) == 1 and b"csa_sample_rows" in err() and b"null args" in err()

    def call(**kw):
        base = dict(logits=16, rows=4, V=60, logits_stride=60, ys=16, ys_stride=8, pad=16, pad_stride=8, logp=16,
                    logp_stride=7, T=8, fin=16, inv_temperature=1.0, top_p=1.0, top_k=0, eos_id=3, pad_id=0, rng_dev=16,
                    t_dev=16)
        base.update(kw)
        a = _lib.SampleRowsArgs(**base)
        return L.csa_sample_rows(ctypes.byref(a), None)
    assert call(V=0) == 2 and b"csa_sample_rows" in err() and b"V must be in [1, 32768]" in err()
    assert call(V=32769, logits_stride=32769) == 2 and b"V must be" in err()
    for name in ("logits", "ys", "pad", "fin", "rng_dev", "t_dev"):
        assert call(**{name: None}) == 1 and b"csa_sample_rows" in err() and b"null pointer" in err(), name
    for name, bad in (("logits", 18), ("ys", 20), ("logp", 18), ("rng_dev", 20), ("t_dev", 17)):
        assert call(**{name: bad}) == 1 and b"misaligned" in err(), name
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(inv_temperature=bad) == 1 and b"temperature must be positive" in err()
    for bad in (0.0, -0.5, float("nan")):
        assert call(top_p=bad) == 1 and b"top_p must be positive" in err()
    assert call(top_k=-1) == 1 and b"top_k" in err()
    for kw in (dict(logits_stride=59), dict(ys_stride=7), dict(pad_stride=7), dict(logp_stride=6)):
        assert call(**kw) == 1 and b"stride" in err(), kw
    assert call(T=1) == 1 and b"T" in err()
    assert call(rows=-1) == 1
    assert call(logp=None, logp_stride=0, rows=0) == 0  # nothing to do, no launch
