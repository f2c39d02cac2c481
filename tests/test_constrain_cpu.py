"""Decoding constraints without a GPU: the loop oracle (tests/constrain_ref.py) on hand-built rows for each rule, the
torch fallback of csa_amd.decode_ops.constrain_rows against it bitwise, the three generators on the fallback path
(what their outputs may no longer contain, and that `None` changes nothing), and the host-side validation of
csa_constrain_rows."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import constrain_ref
from constrain_ref import (EOS_ID, GEN_MIN_LENGTH, GEN_SEED, GEN_T, bits, constrain_np, constraints, generator_case, make,
                           output_faults, run, run_op)
from constrain_ref import GEN_SUPPRESS as SUPPRESS

NINF = -np.inf


def both(z, ys, t, fin=None, **kw):
    """The oracle's array, after checking that the fallback gives the same bits."""
    want = constrain_np(z, ys, t, fin=fin, **kw).z
    for form in ("dev", "host"):
        got, _ = run_op(z, ys, t, fin=fin, form=form, **kw)
        assert np.array_equal(got, bits(want)), (form, kw)
    return want


def hist(*rows, T=8):
    ys = np.full((len(rows), T), 6, dtype=np.int64)  # the unread columns hold a valid id
    for r, h in enumerate(rows):
        ys[r, :len(h)] = h
    return ys


def test_penalty_hits_each_distinct_token_once_and_keeps_special_values():
    theta = np.float32(1.5)
    z = np.array([[2.0, -2.0, 0.0, NINF, np.nan, 3.0, 7.0, -0.0]], dtype=np.float32)
    ys = hist([0, 1, 0, 2, 0, 3, 4, 7], T=9)  # token 0 three times
    out = both(z, ys, 7, repetition_penalty=1.5)
    assert out[0, 0] == np.float32(2.0) / theta and out[0, 0] != np.float32(2.0) / theta / theta  # once, not thrice
    assert out[0, 1] == np.float32(-2.0) * theta
    assert bits(out[0, 2:5]).tolist() == bits(z[0, 2:5]).tolist()  # 0, -inf and NaN map to themselves
    assert bits(out[0, 7:]).tolist() == bits(z[0, 7:]).tolist()    # and so does -0
    assert out[0, 5] == 3.0 and out[0, 6] == 7.0                   # not in the history
    half = both(z, ys, 7, repetition_penalty=0.5)                  # below one: the other direction
    assert half[0, 0] == 4.0 and half[0, 1] == -1.0
    early = both(z, ys, 0, repetition_penalty=1.5)                 # only h[0] at t = 0
    assert early[0, 0] == np.float32(2.0) / theta and early[0, 1] == -2.0
    one_third = both(np.array([[1.0, 1.0]], dtype=np.float32), hist([0]), 0, repetition_penalty=3.0)
    assert one_third[0, 0] == np.float32(1.0) / np.float32(3.0)    # a true division, not a product by 1/theta's rounding
    assert np.array_equal(bits(both(z, ys, 7)), bits(z))           # theta = 1: off


def test_ngram_bans_with_overlapping_matches_and_short_histories():
    z = np.zeros((1, 8), dtype=np.float32)
    banned = lambda ys, t, n: sorted(np.nonzero(both(z, ys, t, no_repeat_ngram=n)[0] == NINF)[0].tolist())
    ys = hist([2, 5, 5, 5, 1, 5, 5])
    assert banned(ys, 6, 1) == [1, 2, 5]                 # n = 1: every history token
    assert banned(ys, 6, 2) == [1, 5]                    # after "5": 5 (twice, overlapping) and 1
    assert banned(ys, 6, 3) == [1, 5]                    # after "5 5": 5 (i = 1) and 1 (i = 2); i = 4 would need h[7]
    assert banned(ys, 3, 3) == [5]                       # h = 2 5 5 5: the suffix "5 5" matches itself shifted by one
    assert banned(ys, 2, 3) == []                        # h = 2 5 5: "2 5" is not "5 5"
    assert banned(ys, 1, 3) == [] and banned(ys, 0, 3) == [] and banned(ys, 0, 2) == []  # L < n: nothing
    assert banned(ys, 1, 2) == []                        # L = n, "2" against the suffix "5"
    assert banned(hist([5, 5]), 1, 2) == [5]             # L = n with a match
    assert banned(ys, 6, 7) == [] and banned(ys, 6, 8) == [] and banned(ys, 6, 1000) == []
    assert banned(hist([4, 4, 4, 4, 4, 4, 4]), 6, 7) == [4]  # L = n: the one start i = 0, whose 6 tokens are the last 6
    assert banned(hist([4, 4, 4, 4, 4, 4, 4]), 6, 6) == [4]


def test_min_length_bans_eos_up_to_the_step_before_it():
    z = np.ones((2, 8), dtype=np.float32)
    ys = hist([2, 5, 6, 7], [2, 1, 1, 1])
    kw = dict(min_length=3, eos_id=EOS_ID)
    assert both(z, ys, 2, **kw)[:, EOS_ID].tolist() == [NINF, NINF]  # t = min_length - 1
    assert both(z, ys, 3, **kw)[:, EOS_ID].tolist() == [1.0, 1.0]    # t = min_length
    for off in (dict(min_length=0, eos_id=EOS_ID), dict(min_length=3, eos_id=None), dict(min_length=3, eos_id=8)):
        assert np.array_equal(both(z, ys, 0, **off), z)
    assert int((both(z, ys, 0, **kw) == NINF).sum()) == 2              # nothing but the EOS column


def test_ids_outside_the_vocabulary_are_compared_but_never_written():
    V = 8
    z = np.arange(1, 1 + 2 * V, dtype=np.float32).reshape(2, V)
    big = 2 ** 40
    ys = hist([2, big, 5, -1, 7, big], [2, V, V, -3, -3, 4, V], T=9)
    out = both(z, ys, 5, no_repeat_ngram=2)
    assert sorted(np.nonzero(out[0] == NINF)[0].tolist()) == [5]   # "big" is followed by 5: compared as the id it is
    assert sorted(np.nonzero(out[1] == NINF)[0].tolist()) == []    # the suffix is 4 at t = 5
    out = both(z, ys, 6, no_repeat_ngram=2)
    assert sorted(np.nonzero(out[1] == NINF)[0].tolist()) == []    # after V come V and -3: neither is a column
    out = both(z, ys, 6, no_repeat_ngram=1, repetition_penalty=2.0)
    assert sorted(np.nonzero(out[1] == NINF)[0].tolist()) == [2, 4]
    assert out[0].tolist()[:2] == z[0, :2].tolist()
    sup = both(z, ys, 0, suppress=(-1, 3, V, V + 1, 2 ** 31 - 1, -2 ** 31, 0))
    assert [sorted(np.nonzero(r == NINF)[0].tolist()) for r in sup] == [[0, 3], [0, 3]]


def test_a_ban_wins_over_the_penalty_and_a_finished_row_is_untouched():
    z = np.array([[4.0, -4.0, 2.0, 1.0, NINF, 0.5]] * 3, dtype=np.float32)
    ys = hist([2, 0, 1, 0], [2, 0, 1, 0], [2, 0, 1, 0])
    fin = np.array([0, 1, 0], dtype=np.uint8)
    kw = dict(repetition_penalty=2.0, no_repeat_ngram=2, min_length=9, eos_id=5, suppress=(3,))
    out = both(z, ys, 3, fin=fin, **kw)
    assert out[0].tolist() == [2.0, NINF, 1.0, NINF, NINF, NINF]   # 1 follows 0: banned although penalised; 0 and 2 halved
    assert np.array_equal(bits(out[1]), bits(z[1])) and np.array_equal(out[2], out[0])
    every = both(z, ys, 3, fin=np.ones(3, dtype=np.uint8), **kw)
    assert np.array_equal(bits(every), bits(z))
    none = both(z, ys, 3, fin=np.zeros(3, dtype=np.uint8), **kw)
    assert np.array_equal(none[1], out[0])


@pytest.mark.parametrize("V,T", [(19, 12), (257, 40), (1028, 257), (5, 1030)])
def test_fallback_is_bitwise_the_oracle_on_seeded_cases(V, T):
    """Histories over three symbols, so n-grams repeat. From t = 8 on (nine tokens or more in each of 9 rows) every case
    must really do what its rule is for: a penalty rule penalises, a ban rule bans, all rules together do both, with
    and without finished rows. (The length rule alone acts at t < 2 only, where it must ban.)"""
    z, ys, fin = constrain_ref.kernel_case(V, T, rows=9)
    for name, kw in constrain_ref.rules(V).items():
        for t in sorted(set(constrain_ref.steps(T)) | {8, T // 2}):
            for f in (None, fin):
                want = constrain_np(z, ys, t, fin=f, **kw)
                bans = name.startswith("ngram") or name in ("suppress", "all") or (name == "min_length" and t < 2)
                if t >= 8 or name == "min_length":
                    assert (want.banned > 0) == bans, (name, t, want.banned)
                    assert (want.penalised > 0) == ("repetition_penalty" in kw), (name, t, want.penalised)
                for form in ("dev", "host"):
                    got, _ = run_op(z, ys, t, fin=f, form=form, **kw)
                    assert np.array_equal(got, bits(want.z)), (name, t, form)
            got, _ = run_op(z, ys, t, layout="shifted", **kw)
            assert np.array_equal(got, constrain_ref.expected(constrain_np(z, ys, t, **kw).z, 9, V, "shifted")), (name, t)


# ---- the generators on the fallback path ----

@pytest.mark.parametrize("kind", ["greedy", "beam", "sample"])
def test_generator_outputs_obey_the_constraints_that_the_free_run_breaks(kind):
    m, enc, src_mask = generator_case()
    free = run(kind, make(kind, m), enc, src_mask)
    held = run(kind, make(kind, m, constraints=constraints()), enc, src_mask)
    faults = output_faults(free.numpy(), 2, GEN_MIN_LENGTH, SUPPRESS)
    print(kind, "free run faults (bigrams, early EOS, listed ids):", faults)
    assert all(f > 0 for f in faults), faults
    assert output_faults(held.numpy(), 2, GEN_MIN_LENGTH, SUPPRESS) == (0, 0, 0)
    assert held.shape == free.shape and not torch.equal(held, free)
    again = run(kind, make(kind, m, constraints=constraints(), graph=True), enc, src_mask)  # CPU: nothing captured
    assert torch.equal(again, held)


@pytest.mark.parametrize("kind", ["greedy", "beam", "sample"])
def test_none_and_inactive_constraints_change_nothing(kind):
    from csa_amd.model import DecodingConstraints
    m, enc, src_mask = generator_case()
    plain = make(kind, m)
    want = run(kind, plain, enc, src_mask)
    assert plain.constraints is None
    for con in (None, DecodingConstraints(), DecodingConstraints(min_length=4, eos_id=None),
                DecodingConstraints(repetition_penalty=1, no_repeat_ngram_size=0, suppress_ids=[])):
        gen = make(kind, m, constraints=con)
        assert gen.constraints is None and gen._constraint_key() == ()
        assert torch.equal(run(kind, gen, enc, src_mask), want)
    gen = make(kind, m, constraints=constraints())
    assert gen._constraint_key() == (constraints(),)
    gen.constraints = DecodingConstraints()  # assignable between calls; inactive is None
    assert gen.constraints is None and torch.equal(run(kind, gen, enc, src_mask), want)


def test_sampled_log_probabilities_stay_finite_under_constraints():
    """The sampler renormalises over what the bans leave: every drawn token has a finite log-probability <= 0."""
    m, enc, src_mask = generator_case()
    ids, lp = run("sample", make("sample", m, constraints=constraints()), enc, src_mask, return_logp=True)
    assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all()) and bool((lp[ids != 0] < 0).any())


def test_decoding_constraints_is_a_validated_hashable_value():
    from csa_amd.model import DecodingConstraints
    a, b = constraints(), constraints(suppress_ids=list(SUPPRESS))
    assert a == b and hash(a) == hash(b) and a != constraints(min_length=6) and len({a, b, DecodingConstraints()}) == 2
    assert a.active and not DecodingConstraints().active and a.suppress_ids == SUPPRESS
    for kw in (dict(repetition_penalty=1.1), dict(no_repeat_ngram_size=1), dict(min_length=1), dict(suppress_ids=(0,))):
        assert DecodingConstraints(**kw).active, kw
    assert not DecodingConstraints(min_length=1, eos_id=None).active
    assert DecodingConstraints().eos_id == __import__("csa_amd.data", fromlist=["EOS"]).EOS
    with pytest.raises(AttributeError):
        a.min_length = 2
    import copy
    import pickle
    assert copy.deepcopy(a) == a and pickle.loads(pickle.dumps(a)) == a
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")),
               dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5),
               dict(min_length=-1), dict(min_length=2.5), dict(suppress_ids=(-1,)), dict(suppress_ids=(1.5,)),
               dict(suppress_ids=tuple(range(257))), dict(eos_id=-1), dict(eos_id=1.5)):
        with pytest.raises(ValueError):
            DecodingConstraints(**kw)
    assert len(DecodingConstraints(suppress_ids=range(256)).suppress_ids) == 256


def test_bad_generator_arguments_and_training_mode_raise():
    from csa_amd.model import CachedGreedyGenerator
    m, enc, src_mask = generator_case()
    for kind in ("greedy", "beam", "sample"):
        with pytest.raises(TypeError):
            make(kind, m, constraints=dict(min_length=2))
    gen = CachedGreedyGenerator(m.train(), GEN_T, constraints=constraints())
    with pytest.raises(RuntimeError):
        gen(SimpleNamespace())
    for kind in ("beam", "sample"):  # these two refuse training mode with or without constraints
        with pytest.raises(RuntimeError):
            run(kind, make(kind, m, constraints=constraints()), enc, src_mask)


def test_constrain_rows_checks_its_arguments():
    from csa_amd.decode_ops import constrain_rows
    T = 8
    z = lambda: torch.zeros(4, 9)
    ys = torch.zeros(4, T, dtype=torch.long)
    constrain_rows(z(), ys, 0)
    constrain_rows(z(), ys, torch.zeros(1, dtype=torch.int32), fin=torch.zeros(4, dtype=torch.uint8),
                   suppress=torch.zeros(3, dtype=torch.int32))
    for kw in (dict(ys=torch.zeros(4, T, dtype=torch.int32)), dict(ys=torch.zeros(3, T, dtype=torch.long)),
               dict(ys=torch.zeros(4, 2 * T, dtype=torch.long)[:, ::2]), dict(ys=torch.zeros(4, 1, dtype=torch.long)),
               dict(fin=torch.zeros(4, dtype=torch.bool)), dict(fin=torch.zeros(5, dtype=torch.uint8)),
               dict(t=torch.zeros(1, dtype=torch.int64)), dict(t=torch.zeros(2, dtype=torch.int32)),
               dict(suppress=torch.zeros(3, dtype=torch.int64)), dict(suppress=torch.zeros(257, dtype=torch.int32)),
               dict(suppress=[1, 2]), dict(repetition_penalty=0.0), dict(repetition_penalty=-2.0),
               dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
               dict(no_repeat_ngram=-1), dict(no_repeat_ngram=1.5), dict(min_length=-1),
               dict(z=torch.zeros(4, 18)[:, ::2]), dict(z=torch.zeros(1, 9).expand(4, 9)),
               dict(z=torch.zeros(4, 9, dtype=torch.long)), dict(z=torch.zeros(9))):
        args = dict(z=z(), ys=ys, t=0)
        args.update(kw)
        with pytest.raises(ValueError):
            constrain_rows(args.pop("z"), args.pop("ys"), args.pop("t"), **args)
    for t in (-1, T - 1, 1000):  # the host sees the step here, as an int or in the counter
        for step in (t, torch.tensor([t], dtype=torch.int32)):
            with pytest.raises(ValueError):
                constrain_rows(z(), ys, step, no_repeat_ngram=1)


def test_constrain_entry_point_validates_without_gpu():
    from csa_amd import _lib
    L = _lib.lib()
    err = L.csa_last_error_str
    assert L.csa_abi_version() == 10
    assert L.csa_constrain_rows_supported(2) and L.csa_constrain_rows_supported(50) and L.csa_constrain_rows_supported(1024)
    assert not L.csa_constrain_rows_supported(1) and not L.csa_constrain_rows_supported(1025)
    assert not L.csa_constrain_rows_supported(0) and not L.csa_constrain_rows_supported(-3)
    assert L.csa_constrain_rows(None, None) == 1 and b"csa_constrain_rows" in err() and b"null args" in err()

    def call(**kw):
        base = dict(logits=16, rows=4, V=60, logits_stride=60, ys=16, ys_stride=8, T=8, fin=16, repetition_penalty=1.2,
                    no_repeat_ngram=2, min_length=3, eos_id=3, suppress=16, n_suppress=2, t=0, t_dev=16)
        base.update(kw)
        a = _lib.ConstrainRowsArgs(**base)
        return L.csa_constrain_rows(ctypes.byref(a), None)
    for name in ("logits", "ys", "suppress"):
        assert call(**{name: None}) == 1 and b"csa_constrain_rows" in err() and b"null pointer" in err(), name
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(repetition_penalty=bad) == 1 and b"repetition_penalty" in err()
    for name in ("rows", "V", "T", "no_repeat_ngram", "min_length", "n_suppress"):
        assert call(**{name: -1}) == 1 and b"negative" in err(), name
    assert call(n_suppress=257) == 1 and b"at most 256" in err()
    assert call(logits_stride=59) == 1 and b"stride" in err()
    assert call(ys_stride=7) == 1 and b"stride" in err()
    for T in (1, 1025):
        assert call(T=T, ys_stride=2000) == 2 and b"T must be in [2, 1024]" in err()
    for name, bad in (("logits", 18), ("ys", 20), ("suppress", 18), ("t_dev", 17)):
        assert call(**{name: bad}) == 1 and b"misaligned" in err(), name
    assert call(rows=0) == 0 and call(V=0, logits_stride=0) == 0  # nothing to do, no launch
    assert call(rows=0, fin=None, suppress=None, n_suppress=0, t_dev=None, eos_id=-1) == 0  # the optional pointers
