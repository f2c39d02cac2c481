"""Early stop at EOS without a GPU: the three generators on the fallback path against their uncached oracles run for all
steps and against themselves with early_stop=False (bitwise), last_steps_run against the rule on the oracle's finished
flags, the decode_advance and finished-flag argmax fallbacks on hand-built states, and host-side validation of the two
new entry points."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import beam_ref
import early_stop_ref as ref
import sample_ref
from beam_ref import EOS_ID, PAD, STEP_TOL
from early_stop_ref import T

_CASES = {}


def _case(name):
    """(model, enc, src_mask) of a named case, built once and never modified."""
    if name not in _CASES:
        _CASES[name] = ref.tiny_case(getattr(ref, name))
    return _CASES[name]


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- beam ----

@pytest.mark.parametrize("length_penalty", [0.0, 0.7])
@pytest.mark.parametrize("W", [3, 4])
def test_beam_stops_two_steps_after_the_last_hypothesis_finishes(W, length_penalty):
    from csa_amd.model import BeamSearchGenerator
    m, enc, src_mask = _case("BEAM_STOPS")
    want = beam_ref.beam_search_ref(m, enc, src_mask, T, W, EOS_ID, length_penalty)
    beam_ref.assert_oracle_is_decisive(want, T - 1)
    steps = ref.steps_rule(want.fin.reshape(T - 1, -1).numpy(), T - 1)
    assert steps == 4  # every hypothesis has finished after step 2
    full = BeamSearchGenerator(m, T, W, length_penalty)
    gen = BeamSearchGenerator(m, T, W, length_penalty, early_stop=True)
    a, b = full.search(enc, src_mask, return_all=True), gen.search(enc, src_mask, return_all=True)
    print(f"W={W} lp={length_penalty} steps_run={gen.last_steps_run} score error", (b[2] - want.scores).abs().max().item())
    assert torch.equal(b[1], want.ids) and torch.equal(b[0], want.best)
    np.testing.assert_allclose(b[2].numpy(), want.scores.numpy(), rtol=0, atol=STEP_TOL * (T - 1))
    assert _equal(a, b)
    assert gen.last_steps_run == steps and gen.last_replays == steps
    assert full.last_steps_run == T - 1 and full.last_replays == T - 1


def test_beam_that_never_finishes_runs_every_step():
    from csa_amd.model import BeamSearchGenerator
    m, enc, src_mask = _case("NEVER")
    W = 3
    want = beam_ref.beam_search_ref(m, enc, src_mask, T, W, EOS_ID)
    assert not want.fin.reshape(T - 1, -1)[:-1].all(1).any()  # some hypothesis is live at the start of every step
    full, gen = BeamSearchGenerator(m, T, W), BeamSearchGenerator(m, T, W, early_stop=True)
    a, b = full.search(enc, src_mask, return_all=True), gen.search(enc, src_mask, return_all=True)
    assert gen.last_steps_run == T - 1 and _equal(a, b) and torch.equal(b[1], want.ids)


# ---- sampling ----

@pytest.mark.parametrize("S,steps", [(1, 3), (4, 11)])
def test_sampling_stops_two_steps_after_the_last_row_finishes(S, steps):
    from csa_amd.model import SamplingGenerator
    m, enc, src_mask = _case("NEVER")
    want = sample_ref.sampling_ref(m, enc, src_mask, T, S, ref.SAMPLING_SEED, **ref.SAMPLING)
    sample_ref.assert_decisive(want)
    assert ref.steps_rule(want.fin, T - 1) == steps
    full = SamplingGenerator(m, T, num_samples=S, **ref.SAMPLING)
    gen = SamplingGenerator(m, T, num_samples=S, early_stop=True, **ref.SAMPLING)
    a = full.sample(enc, src_mask, seed=ref.SAMPLING_SEED, return_logp=True)
    b = gen.sample(enc, src_mask, seed=ref.SAMPLING_SEED, return_logp=True)
    assert torch.equal(b[0], want.ids)
    np.testing.assert_allclose(b[1].numpy(), want.logp, rtol=sample_ref.RTOL, atol=sample_ref.ATOL)
    assert _equal(a, b)
    assert gen.last_steps_run == steps and full.last_steps_run == T - 1
    assert torch.equal(gen.sample(enc, src_mask, seed=ref.SAMPLING_SEED), b[0])  # a fresh state per call


# ---- greedy with eos_id ----

def _greedy_case():
    m, enc, src_mask = _case("GREEDY")
    return ref.FixedMemory(m, enc, src_mask), enc, src_mask


def test_greedy_with_eos_id_matches_the_uncached_oracle_and_stops_early():
    from csa_amd.model import CachedGreedyGenerator
    m, enc, src_mask = _greedy_case()
    ids, fins, gap = ref.greedy_eos_ref(m, enc, src_mask, T, EOS_ID)
    first = [int(fins[:, b].int().argmax()) for b in range(enc.shape[0])]
    print("greedy finishing steps", first, "min gap", gap)
    assert bool(fins[T - 4].all()) and len(set(first)) >= 2 and gap > ref.GREEDY_GAP
    steps = ref.steps_rule(fins.numpy(), T - 1)
    assert steps == max(first) + 2
    data = lambda: SimpleNamespace()
    full = CachedGreedyGenerator(m, T, eos_id=EOS_ID)
    gen = CachedGreedyGenerator(m, T, eos_id=EOS_ID, early_stop=True)
    a, b = full(data()), gen(data())  # return_logp has no CPU path: tests/test_early_stop_gpu.py
    assert torch.equal(b, ids) and torch.equal(a, b)
    assert gen.last_steps_run == steps and gen.last_replays == steps and full.last_steps_run == T - 1
    assert torch.equal(gen(data()), ids)
    after = (ids == EOS_ID).cumsum(1) - (ids == EOS_ID).int() > 0
    assert bool(after.any()) and bool((ids[after] == PAD).all())


def test_greedy_without_eos_id_is_todays_generator():
    """eos_id=None, early_stop=False: the ids of the eager loop over int steps, restated here with the package's own
    ops, bitwise; and an EOS changes nothing for it."""
    from csa_amd.decode_ops import argmax_rows
    from csa_amd.model import BOS, CachedGreedyGenerator
    m, enc, src_mask = _greedy_case()
    gen = CachedGreedyGenerator(m, T)
    got = gen(SimpleNamespace())
    assert gen.last_steps_run == T - 1 and gen.eos_id is None and gen.early_stop is False
    with torch.no_grad():
        cache = m.decoder.make_cache(enc, src_mask, T, repeat_heads=True)
        ys = torch.zeros(enc.shape[0], T, dtype=torch.long)
        ys[:, 0] = BOS
        for t in range(T - 1):
            dec = m.decoder.step(m.tgt_embedding.step(ys[:, t:t + 1], t), cache, t)
            logits = m.generator.linear(dec[:, 0])
            argmax_rows(logits, out=ys[:, t + 1], is_pad=cache.pad[:, t + 1], pad_id=PAD)
    assert torch.equal(got, ys[:, 1:])
    assert bool((got == EOS_ID).any()) and not torch.equal(got, ref.greedy_eos_ref(m, enc, src_mask, T, EOS_ID)[0])


def test_early_stop_needs_an_eos_id():
    from csa_amd.model import BeamSearchGenerator, CachedGreedyGenerator, SamplingGenerator
    m = beam_ref.stub_model()
    for make in (lambda **kw: CachedGreedyGenerator(m, 6, **kw), lambda **kw: BeamSearchGenerator(m, 6, 2, **kw),
                 lambda **kw: SamplingGenerator(m, 6, **kw)):
        with pytest.raises(ValueError, match="early_stop"):
            make(early_stop=True, eos_id=None)
        gen = make(eos_id=EOS_ID, early_stop=True)
        assert gen.early_stop is True and gen.last_steps_run is None
        assert make(eos_id=EOS_ID).early_stop is False
    with pytest.raises(ValueError, match="early_stop"):
        CachedGreedyGenerator(m, 6, early_stop=True)  # eos_id defaults to None there


# ---- the fallbacks of the two kernels ----

def _advance(fin, t, state, T_):
    from csa_amd.decode_ops import decode_advance
    t_dev = torch.tensor([t], dtype=torch.int32)
    st = torch.tensor(state, dtype=torch.int32)
    f = torch.tensor(fin, dtype=torch.uint8)
    keep = f.clone()
    decode_advance(f, t_dev, st, T_)
    assert torch.equal(f, keep)
    return int(t_dev), st.tolist()


def test_decode_advance_fallback_on_hand_built_states():
    from csa_amd.decode_ops import decode_advance
    T_ = 8
    assert _advance([0, 1, 1], 2, [0, 2, 0, 0], T_) == (3, [0, 3, 0, 0])      # a live row: on
    assert _advance([1, 1, 1], 2, [0, 2, 0, 0], T_) == (3, [1, 3, 0, 0])      # all finished: one more step
    assert _advance([1, 1, 1], 3, [1, 3, 0, 0], T_) == (-1, [1, 4, 1, 0])     # that step has run: parked
    assert _advance([1, 1, 1], -1, [1, 4, 1, 0], T_) == (-1, [1, 4, 1, 0])    # parked stays parked
    assert _advance([0, 0, 0], -1, [0, 7, 1, 0], T_) == (-1, [0, 7, 1, 0])
    assert _advance([0, 0, 0], T_ - 2, [0, 6, 0, 0], T_) == (-1, [0, 7, 1, 0])  # the last step parks
    assert _advance([0, 0, 0], T_ - 3, [0, 5, 0, 0], T_) == (T_ - 2, [0, 6, 0, 0])
    assert _advance([2, 255, 128], 0, [0, 0, 0, 9], T_) == (1, [1, 1, 0, 9])  # any non-zero byte is finished
    assert _advance([2, 0, 128], 0, [0, 0, 0, 9], T_) == (1, [0, 1, 0, 9])
    for fin, t, st in (([0, 1], 0, [0, 0, 0, 0]), ([1, 1], 4, [1, 5, 0, 0]), ([1], 6, [0, 6, 0, 0]), ([1], -1, [1, 3, 1, 0])):
        assert _advance(fin, t, st, T_) == ref.advance_np(fin, t, st, T_)
    buf = torch.tensor([0, 1, 1, 1], dtype=torch.uint8)  # a view that starts one byte in
    t_dev, st = torch.zeros(1, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    decode_advance(buf[1:], t_dev, st, T_)
    assert st.tolist() == [1, 1, 0, 0] and int(t_dev) == 1
    with pytest.raises(ValueError):
        decode_advance(buf, torch.zeros(1, dtype=torch.int64), st, T_)
    with pytest.raises(ValueError):
        decode_advance(buf, t_dev, torch.zeros(3, dtype=torch.int32), T_)
    with pytest.raises(ValueError):
        decode_advance(buf[::2], t_dev, st, T_)
    with pytest.raises(ValueError):
        decode_advance(buf, t_dev, st, 1)


def test_argmax_rows_fallback_with_a_finished_flag():
    from csa_amd.decode_ops import argmax_rows
    torch.manual_seed(4)
    rows, V, T_, H, t = 5, 19, 6, 2, 2
    x = torch.randn(rows, V)
    x[0, EOS_ID] = 9.0   # live, draws EOS
    x[1, PAD] = 9.0      # live, draws PAD: not finished by it
    x[2, 7] = 9.0        # finished: PAD whatever the logits
    x[3, EOS_ID] = 9.0   # finished with a byte other than 1: left as it is
    fin = torch.tensor([0, 0, 1, 5, 0], dtype=torch.uint8)
    tok, padb, fin_after = ref.argmax_fin_np(x.numpy(), fin.numpy(), EOS_ID)
    assert tok.tolist()[:4] == [EOS_ID, PAD, PAD, PAD] and fin_after.tolist() == [1, 0, 1, 5, 0]
    ys = torch.full((rows, T_), 9, dtype=torch.long)
    pad = torch.full((rows, T_), 7, dtype=torch.uint8)
    hp = torch.full((rows, H, T_), 7, dtype=torch.uint8)
    keep = (ys.clone(), pad.clone(), hp.clone())
    f = fin.clone()
    assert argmax_rows(x, out=ys, is_pad=pad, pad_id=PAD, t_dev=torch.tensor([t], dtype=torch.int32), head_pad=hp,
                       fin=f, eos_id=EOS_ID) is ys
    np.testing.assert_array_equal(ys[:, t + 1].numpy(), tok)
    np.testing.assert_array_equal(pad[:, t + 1].numpy(), padb)
    np.testing.assert_array_equal(f.numpy(), fin_after)
    for h in range(H):
        np.testing.assert_array_equal(hp.view(H, rows, T_)[h, :, t + 1].numpy(), padb)
    for got, was in zip((ys, pad, hp.view(H, rows, T_)), (keep[0], keep[1], keep[2].view(H, rows, T_))):
        other = [c for c in range(T_) if c != t + 1]
        assert torch.equal(got[..., other], was[..., other])
    f2 = fin.clone()
    argmax_rows(x, out=ys, is_pad=pad, t_dev=torch.tensor([t], dtype=torch.int32), fin=f2, eos_id=None)  # never finishes
    assert torch.equal(f2, fin) and int(ys[0, t + 1]) == EOS_ID
    with pytest.raises(ValueError):
        argmax_rows(x, out=ys[:, 1], is_pad=pad[:, 1], fin=f)  # fin goes with t_dev
    with pytest.raises(ValueError):
        argmax_rows(x, out=ys, is_pad=pad, t_dev=torch.tensor([t], dtype=torch.int32), fin=f[:3], eos_id=EOS_ID)


# ---- the C entry points, without a GPU ----

def test_new_entry_points_validate_without_gpu():
    from csa_amd import _lib
    L = _lib.lib()
    err = L.csa_last_error_str
    assert L.csa_abi_version() == 10  # additions to v10: no existing entry point changed
    # (x, rows, V, ys, ys_stride, T, pad, pad_stride, head_pad, H, pad_id, fin, eos_id, t_dev, stream)
    ok = [16, 3, 60, 16, 6, 6, 16, 6, 16, 2, 0, 17, 3, 16, None]
    names = ["x", "rows", "V", "ys", "ys_stride", "T", "pad", "pad_stride", "head_pad", "H", "pad_id", "fin", "eos_id",
             "t_dev", "stream"]

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return L.csa_argmax_rows_fin_step(*args)
    for name in ("x", "ys", "fin", "t_dev"):
        assert call(**{name: None}) == 1, name
        assert b"csa_argmax_rows_fin_step" in err() and b"null pointer" in err(), name
    for name, bad in (("x", 18), ("ys", 20), ("t_dev", 17)):
        assert call(**{name: bad}) == 1, name
        assert b"csa_argmax_rows_fin_step" in err() and b"misaligned" in err(), name
    assert call(V=0) == 1 and b"csa_argmax_rows_fin_step" in err()
    assert call(ys_stride=5) == 1 and call(pad_stride=5) == 1 and call(H=0) == 1
    assert call(rows=0) == 0  # nothing to do, no launch

    # (fin, rows, T, t_dev, state, stream)
    def adv(fin=17, rows=3, T_=8, t_dev=16, state=32):
        return L.csa_decode_advance(fin, rows, T_, t_dev, state, None)
    for kw in (dict(fin=None), dict(t_dev=None), dict(state=None)):
        assert adv(**kw) == 1, kw
        assert b"csa_decode_advance" in err() and b"null pointer" in err(), kw
    for kw in (dict(t_dev=18), dict(state=33), dict(state=34)):
        assert adv(**kw) == 1, kw
        assert b"csa_decode_advance" in err() and b"misaligned" in err(), kw
    assert adv(rows=-1) == 1 and adv(T_=1) == 1 and b"csa_decode_advance" in err()
