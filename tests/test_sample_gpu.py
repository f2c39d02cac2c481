"""Sampled decoding on the GPU: k_sample_rows (csrc/csa_sample.hip) against the fp64 oracle (tests/sample_ref.py) in
every launch class, and SamplingGenerator against the uncached oracle, its own captured graph and the memory physically
repeated per sample. Every fixture is decisive on the oracle, so tokens compare exactly; the log-probabilities compare
at the suite's tolerance; every result repeats bitwise."""
import functools

import numpy as np
import pytest
import torch

import sample_ref
from conftest import has_gpu
from sample_ref import (ATOL, EOS_ID, FILTERS, KERNEL_ROWS, KERNEL_SEED, KERNEL_STEPS, KERNEL_T, PAD, RTOL,
                        assert_decisive, assert_matches, run_op, sampling_ref, search_case)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]

T = KERNEL_T


@functools.lru_cache(maxsize=None)
def class_oracle(V):
    """The logits of a launch class and the oracle's result for every (filter, step), computed once for the largest
    row count: a row's result depends on its index alone, so the smaller launches are its first rows."""
    z = sample_ref.kernel_logits(V)
    filt = {k: sample_ref.filter_np(z, **kw) for k, kw in FILTERS.items()}
    out = {}
    for t in KERNEL_STEPS:
        g = sample_ref.gumbel_np(z.shape[0], V, t, KERNEL_SEED)
        for k in FILTERS:
            out[k, t] = sample_ref.draw_np(filt[k], g, eos_id=EOS_ID)
            assert_decisive(out[k, t], f"V={V} {k} t={t}")
    return z, out


def first_rows(r, rows):
    return type(r)(**{k: v[:rows] for k, v in vars(r).items()})


CLASSES = [(V, False) for V in sample_ref.KERNEL_VS] + [(1028, True)]


@pytest.mark.parametrize("rows", KERNEL_ROWS)
@pytest.mark.parametrize("V,shift", CLASSES, ids=[f"{V}{'_shifted' if s else ''}" for V, s in CLASSES])
def test_sample_rows_kernel_matches_the_oracle(V, shift, rows):
    z, oracle = class_oracle(V)
    for name, kw in FILTERS.items():
        for t in KERNEL_STEPS:
            want = first_rows(oracle[name, t], rows)
            what = f"V={V} rows={rows} {name} t={t} shift={shift}"
            got = run_op(z[:rows], t, KERNEL_SEED, device="cuda", shift=shift, eos_id=EOS_ID, **kw)
            assert_matches(got, want, what)
            again = run_op(z[:rows], t, KERNEL_SEED, device="cuda", shift=shift, eos_id=EOS_ID, **kw)
            assert np.array_equal(again.tok, got.tok) and np.array_equal(again.logp, got.logp), what  # bitwise
            other = [c for c in range(T) if c != t + 1]
            assert bool((got.ys[:, other] == 99).all()) and bool((got.pads[:, other] == 7).all()), what
            assert bool((got.logps[:, [c for c in range(T - 1) if c != t]] == 5.0).all()), what
    if shift:  # the same columns per thread in the same order: bitwise the aligned launch
        for name, kw in FILTERS.items():
            a = run_op(z[:rows], 3, KERNEL_SEED, device="cuda", shift=False, **kw)
            b = run_op(z[:rows], 3, KERNEL_SEED, device="cuda", shift=True, **kw)
            assert np.array_equal(a.tok, b.tok) and np.array_equal(a.logp, b.logp), name


def test_sample_rows_kernel_keeps_all_ties_and_handles_empty_rows():
    """The hand-built rows of the CPU test through the kernel: ties at the top-k threshold, a tie class at the nucleus
    boundary, -inf and NaN entries, an all -inf row, three temperatures."""
    z = sample_ref.hand_rows()
    for tau in (0.05, 1.0, 5.0):
        for top_k in (0, 1, 2, 11, 12, 15):
            for top_p in (1.0, 1e-3, 0.45, 0.85):
                kw = dict(temperature=tau, top_k=top_k, top_p=top_p)
                want = sample_ref.sample_rows_np(z, 3, 11, eos_id=EOS_ID, **kw)
                assert_decisive(want, str(kw))
                got = run_op(z, 3, 11, device="cuda", eos_id=EOS_ID, **kw)
                assert_matches(got, want, str(kw))
                assert got.tok[3] == 0 and got.logp[3] == -np.inf


def test_sample_rows_kernel_finished_rows_and_eos_none():
    z, oracle = class_oracle(257)
    rows = z.shape[0]
    fin = (np.arange(rows) % 3 == 1).astype(np.uint8)
    for name, kw in FILTERS.items():
        free = oracle[name, 3]
        want = sample_ref.draw_np(sample_ref.filter_np(z, **kw), sample_ref.gumbel_np(rows, 257, 3, KERNEL_SEED), fin,
                                  eos_id=int(free.tok[0]))
        assert want.fin[0] == 1 and fin[0] == 0  # row 0 draws its EOS in this step
        got = run_op(z, 3, KERNEL_SEED, fin=fin, device="cuda", eos_id=int(free.tok[0]), **kw)
        assert_matches(got, want, name)
        done = fin != 0
        assert bool((got.tok[done] == PAD).all()) and bool((got.logp[done] == 0).all()) and bool((got.fin[done] == 1).all())
        assert bool((got.pad[done] == 1).all())
        never = run_op(z, 3, KERNEL_SEED, fin=fin, device="cuda", eos_id=None, **kw)
        assert np.array_equal(never.fin, fin) and np.array_equal(never.tok, got.tok)
        assert run_op(z, 3, KERNEL_SEED, device="cuda", logp=False, **kw).logp is None  # logp is optional


def test_sample_rows_kernel_stores_nothing_for_a_counter_outside_its_range():
    z, _ = class_oracle(257)
    fin = (np.arange(z.shape[0]) % 2).astype(np.uint8)
    for kw in (dict(), dict(top_k=5, top_p=0.7)):
        for t in (-1, T - 1, T, 1000, -2 ** 31):
            got = run_op(z, t, KERNEL_SEED, fin=fin, device="cuda", eos_id=EOS_ID, **kw)
            assert bool((got.ys == 99).all()) and bool((got.pads == 7).all()) and bool((got.logps == 5.0).all()), t
            assert np.array_equal(got.fin, fin)


def test_sample_rows_supported_states_its_limit():
    from csa_amd import _lib
    L = _lib.lib()
    assert L.csa_sample_rows_supported(32768) == 1 and L.csa_sample_rows_supported(32769) == 0
    assert L.csa_sample_rows_supported(0) == 0


def test_sample_rows_beyond_the_limit_takes_the_fallback():
    z = torch.randn(2, 32769, generator=torch.Generator().manual_seed(1)).numpy()
    want = sample_ref.sample_rows_np(z, 0, 5)
    assert_decisive(want)
    assert_matches(run_op(z, 0, 5, device="cuda"), want, "V = 32769")


# ---- the generator ----

@pytest.mark.parametrize("S,kw,seed", sample_ref.GENERATOR_CASES, ids=sample_ref.GENERATOR_IDS)
def test_generator_eager_graph_and_oracle_agree(S, kw, seed):
    """Eager equals graph=True bitwise with one capture over two calls, a second call with another seed changes the ids
    without a recapture, and both equal the uncached oracle on the stub case."""
    from csa_amd.model import SamplingGenerator
    m, enc, src_mask = search_case()
    ref = sampling_ref(m, enc, src_mask, T, S, seed, **kw)
    assert_decisive(ref)
    m, enc, src_mask = m.cuda(), enc.cuda(), src_mask.cuda()
    eager = SamplingGenerator(m, T, num_samples=S, **kw)
    gen = SamplingGenerator(m, T, num_samples=S, graph=True, **kw)
    want = eager.sample(enc, src_mask, seed=seed, return_logp=True)
    got = gen.sample(enc, src_mask, seed=seed, return_logp=True)
    other = gen.sample(enc, src_mask, seed=seed + 1, return_logp=True)
    again = gen.sample(enc, src_mask, seed=seed, return_logp=True)
    assert gen.captures == 1 and eager.captures == 0
    for a, b, c in zip(want, got, again):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(other[0], got[0])
    want_other = eager.sample(enc, src_mask, seed=seed + 1, return_logp=True)
    assert torch.equal(other[0], want_other[0]) and torch.equal(other[1], want_other[1])
    assert torch.equal(got[0].cpu(), ref.ids)
    np.testing.assert_allclose(got[1].cpu().numpy(), ref.logp, rtol=RTOL, atol=ATOL)
    ids_only = gen.sample(enc, src_mask, seed=seed)  # another key extra: its own graph
    assert gen.captures == 2 and torch.equal(ids_only, got[0])


def test_samples_share_one_memory_as_if_it_were_repeated():
    """num_samples = 3 against the memory physically repeated three times at num_samples = 1: a row's draws depend on
    its row index, so the ids are equal (the memory projections are GEMMs of two shapes, so the log-probabilities
    are compared at the suite's tolerance)."""
    from csa_amd.model import SamplingGenerator
    m, enc, src_mask = search_case(device="cuda")
    for kw in ({}, sample_ref.FILTERED):
        ids, lp = SamplingGenerator(m, T, num_samples=3, **kw).sample(enc, src_mask, seed=9, return_logp=True)
        rep, rlp = SamplingGenerator(m, T, **kw).sample(enc.repeat_interleave(3, 0), src_mask.repeat_interleave(3, 0),
                                                         seed=9, return_logp=True)
        assert ids.shape == (3, 3, T - 1) and rep.shape == (9, T - 1)
        assert torch.equal(ids.reshape(9, T - 1), rep)
        np.testing.assert_allclose(lp.reshape(9, T - 1).cpu().numpy(), rlp.cpu().numpy(), rtol=RTOL, atol=ATOL)
        assert bool((ids[:, 0] != ids[:, 1]).any())


def test_generator_graph_refuses_what_it_cannot_capture():
    from csa_amd.model import SamplingGenerator
    m, enc, src_mask = search_case(device="cuda")
    gen = SamplingGenerator(m, T, graph=True)
    with pytest.raises(ValueError):
        gen.sample(enc.double(), src_mask, seed=1)
    assert gen.captures == 0
    m.generator.linear = torch.nn.Linear(32, 32769).cuda()
    with pytest.raises(ValueError):
        SamplingGenerator(m.eval(), T, graph=True).sample(enc, src_mask, seed=1)
