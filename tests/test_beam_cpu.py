"""Beam search without a GPU: BeamSearchGenerator.search on the torch fallbacks of csa_amd.decode_ops against the
uncached oracle (tests/beam_ref.py), the selection and row top-W fallbacks on hand-built states, and the host-side
validation of the beam entry points."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import beam_ref
from beam_ref import (STEP_TOL, assert_oracle_is_decisive, assert_run_is_interesting, assert_select_equal,
                      expected_select, greedy_ids_ref, run_select, search_case)

@pytest.mark.parametrize("W", [3, 4])
def test_search_on_the_fallback_path_matches_the_oracle(W):
    from csa_amd.model import BeamSearchGenerator
    T = 8
    m, enc, src_mask = search_case()
    ref = beam_ref.beam_search_ref(m, enc, src_mask, T, W, beam_ref.EOS_ID)
    print(f"W={W} min_gap={ref.min_gap:.6f} fin_before_end={int(ref.fin[:-1].sum())}")
    assert_oracle_is_decisive(ref, T - 1)
    assert_run_is_interesting(ref, greedy_ids_ref(m, enc, src_mask, T))
    gen = BeamSearchGenerator(m, T, W, graph=True)  # no CUDA model: nothing is captured
    best, ids, scores = gen.search(enc, src_mask, return_all=True)
    assert gen.captures == 0
    assert best.shape == (3, T - 1) and ids.shape == (3, W, T - 1) and scores.shape == (3, W)
    assert torch.equal(ids, ref.ids) and torch.equal(best, ref.best)
    np.testing.assert_allclose(scores.numpy(), ref.scores.numpy(), rtol=0, atol=STEP_TOL * (T - 1))
    after_eos = (ids == beam_ref.EOS_ID).cumsum(-1) - (ids == beam_ref.EOS_ID).int() > 0
    assert bool((ids[after_eos] == beam_ref.PAD).all())  # PAD after EOS
    assert torch.equal(gen.search(enc, src_mask), best)


def test_length_penalty_ranks_by_normalised_score_and_eos_none_never_finishes():
    from csa_amd.model import BeamSearchGenerator
    T, W = 8, 4
    m, enc, src_mask = search_case()
    ref = beam_ref.beam_search_ref(m, enc, src_mask, T, W, beam_ref.EOS_ID, length_penalty=1.0)
    _, ids, scores = BeamSearchGenerator(m, T, W, length_penalty=1.0).search(enc, src_mask, return_all=True)
    assert torch.equal(ids, ref.ids)
    np.testing.assert_allclose(scores.numpy(), ref.scores.numpy(), rtol=0, atol=STEP_TOL * (T - 1))
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    ref = beam_ref.beam_search_ref(m, enc, src_mask, T, W, None)
    _, ids, _ = BeamSearchGenerator(m, T, W, eos_id=None).search(enc, src_mask, return_all=True)
    assert torch.equal(ids, ref.ids) and not bool(ref.fin.any())


def test_beam_of_one_is_the_cached_greedy_generator():
    from csa_amd.model import BeamSearchGenerator, CachedGreedyGenerator
    m, enc, src_mask = search_case(seed=16, gen_scale=3.0, eos_bias=-4.0)
    m.process_data = lambda data: setattr(data, "src_mask", src_mask)
    m.encode = lambda data: (enc, 1, None, [], [])
    want = CachedGreedyGenerator(m, 8)(SimpleNamespace())
    # greedy key-pads its heads the reference's way, which differs only where a PAD was emitted
    assert not bool((want == beam_ref.PAD).any())
    got = BeamSearchGenerator(m, 8, 1, eos_id=None)(SimpleNamespace())
    assert torch.equal(got, want)


def test_training_mode_and_bad_widths_raise():
    from csa_amd.model import BeamSearchGenerator
    m, enc, src_mask = search_case()
    with pytest.raises(ValueError):
        BeamSearchGenerator(m, 8, 0)
    with pytest.raises(ValueError):
        BeamSearchGenerator(m, 8, 9)
    gen = BeamSearchGenerator(m.train(), 8, 2)
    with pytest.raises(RuntimeError):
        gen.search(enc, src_mask)
    with pytest.raises(RuntimeError):
        gen(SimpleNamespace())


@pytest.mark.parametrize("name,state,claim", beam_ref.select_states(), ids=[s[0] for s in beam_ref.select_states()])
def test_select_fallback_on_hand_built_states(name, state, claim):
    want = expected_select(state)
    assert claim(want[5], want[1], want[2], want[3]), f"{name}: the state does not show what it is built for"
    assert_select_equal(run_select(state), want, name)


def test_select_fallback_refuses_a_counter_outside_its_range():
    _, state, _ = beam_ref.select_states()[0]
    for t in (-1, state["T"] - 1, 1000):
        with pytest.raises(ValueError):
            run_select(state, t=t)


def test_row_topk_fallback():
    from csa_amd.decode_ops import beam_row_topk
    g = torch.Generator().manual_seed(3)
    x = (torch.randperm(5 * 60, generator=g).float() / 7 - 20).view(5, 60)
    x[1, [7, 41, 59]] = 1e3          # duplicated maxima: the lowest index first
    x[2] = float("-inf")             # an all -inf row gives 0 .. W-1
    x[3, ::2] = float("-inf")        # a row with -inf entries
    for W in (1, 4, 8):
        lse, tv, ti = beam_row_topk(x, W)
        rl, rv, ri = beam_ref.row_topk_np(x.numpy(), W)
        np.testing.assert_array_equal(ti.numpy(), ri)
        np.testing.assert_allclose(tv.numpy(), rv, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(lse.numpy(), rl, rtol=1e-4, atol=1e-5)
        assert ti[2].tolist() == list(range(W)) and lse[2] == float("-inf")
    assert beam_row_topk(x, 4)[2][1, :3].tolist() == [7, 41, 59]
    with pytest.raises(ValueError):
        beam_row_topk(x[:, :3], 4)   # V < W
    with pytest.raises(ValueError):
        beam_row_topk(x, 9)
    with pytest.raises(ValueError):  # the host sees the counter here
        beam_row_topk(x, 4, t_dev=torch.tensor([5], dtype=torch.int32), t_end=5)


def test_decode_attention_fallback_with_ancestry_and_group():
    """anc= equals the plain call on a physically gathered cache; kv_group= equals the memory repeated per row."""
    from csa_amd.decode_ops import decode_attention
    g = torch.Generator().manual_seed(2)
    B, W, H, hd, cap, t = 2, 3, 2, 8, 6, 4
    R = B * W
    q, kn, vn = torch.randn(R, 3, H, hd, generator=g).unbind(1)
    cache = torch.randn(2, R, H, cap, hd, generator=g)
    anc = ((torch.arange(R)[:, None] // W) * W + torch.randint(0, W, (R, cap), generator=g)).int()
    mask = (torch.rand(R, cap, generator=g) < 0.3).to(torch.uint8)
    mask[:, 0] = 0
    gathered = cache.clone()
    for j in range(t):
        gathered[:, :, :, j] = cache[:, anc[:, j].long(), :, j]
    want = decode_attention(q, gathered[0], gathered[1], key_mask=mask, k_new=kn, v_new=vn, t=t)
    before = cache.clone()
    got = decode_attention(q, cache[0], cache[1], key_mask=mask, k_new=kn, v_new=vn, t=t, anc=anc)
    assert torch.equal(got, want)
    assert torch.equal(cache[0, :, :, t], kn) and torch.equal(cache[1, :, :, t], vn)
    keep = [j for j in range(cap) if j != t]
    assert torch.equal(cache[:, :, :, keep], before[:, :, :, keep])  # no cache row moved
    kv = torch.randn(B, 5, 2, H, hd, generator=g)
    k, v = (u.transpose(1, 2) for u in kv.unbind(2))
    mm = torch.zeros(B, 5, dtype=torch.uint8)
    mm[1, 3:] = 1
    want = decode_attention(q, k.repeat_interleave(W, 0), v.repeat_interleave(W, 0), key_mask=mm.repeat_interleave(W, 0))
    assert torch.equal(decode_attention(q, k, v, key_mask=mm, kv_group=W), want)
    with pytest.raises(ValueError):
        decode_attention(q, k, v, key_mask=mm, kv_group=4)  # 6 rows are no multiple of 4
    with pytest.raises(ValueError):
        decode_attention(q, cache[0], cache[1], anc=anc)    # a table needs append mode


def _attn_args(_lib, **kw):
    base = dict(B=6, H=3, hd=8, len=4, q=16, K=16, V=16, out=16, k_new=16, v_new=16, q_sb=24, q_sh=8, k_sb=96, k_sh=32,
                k_sn=8, v_sb=96, v_sh=32, v_sn=8, kn_sb=24, kn_sh=8, vn_sb=24, vn_sh=8)
    base.update(kw)
    return _lib.DecodeAttnArgs(**base)


def test_beam_entry_points_validate_without_gpu():
    from csa_amd import _lib
    L = _lib.lib()
    err = L.csa_last_error_str
    assert L.csa_abi_version() == 10
    # csa_decode_attn_beam(args, t_dev, anc, anc_stride, kv_group, stream)
    assert L.csa_decode_attn_beam(None, 16, 16, 4, 1, None) == 1
    assert b"csa_decode_attn_beam" in err() and b"null args" in err()
    a = _attn_args(_lib)
    assert L.csa_decode_attn_beam(ctypes.byref(a), 16, None, 0, 4, None) == 1  # 6 rows, groups of 4
    assert b"csa_decode_attn_beam" in err() and b"kv_group" in err()
    assert L.csa_decode_attn_beam(ctypes.byref(a), 16, None, 0, 0, None) == 1
    assert b"kv_group" in err()
    assert L.csa_decode_attn_beam(ctypes.byref(a), 16, 16, 4, 3, None) == 1    # a table with a group
    assert b"ancestry" in err()
    assert L.csa_decode_attn_beam(ctypes.byref(a), 16, 18, 4, 1, None) == 1    # table not 4-byte aligned
    assert b"anc" in err() and b"aligned" in err()
    assert L.csa_decode_attn_beam(ctypes.byref(a), 16, 16, 3, 1, None) == 1    # table rows shorter than len
    assert b"anc" in err()
    assert L.csa_decode_attn_beam(ctypes.byref(a), 18, 16, 4, 1, None) == 1    # counter not 4-byte aligned
    assert b"t_dev" in err()
    a = _attn_args(_lib, V=20)
    assert L.csa_decode_attn_beam(ctypes.byref(a), 16, 16, 4, 1, None) == 1 and b"aligned" in err()
    a = _attn_args(_lib, k_sn=6)
    assert L.csa_decode_attn_beam(ctypes.byref(a), 16, 16, 4, 1, None) == 1 and b"multiples of 4" in err()
    a = _attn_args(_lib, q=None)
    assert L.csa_decode_attn_beam(ctypes.byref(a), 16, 16, 4, 1, None) == 1 and b"null pointer" in err()
    a = _attn_args(_lib, hd=6)
    assert L.csa_decode_attn_beam(ctypes.byref(a), 16, 16, 4, 1, None) == 2
    a = _attn_args(_lib, k_new=None, v_new=None)
    assert L.csa_decode_attn_beam(ctypes.byref(a), None, 16, 4, 1, None) == 1 and b"ancestry" in err()
    # csa_beam_row_topk(z, rows, V, W, lse, topv, topi, t_dev, t_end, stream)
    assert L.csa_beam_row_topk(None, 4, 60, 4, 16, 16, 16, None, 0, None) == 1
    assert b"csa_beam_row_topk" in err() and b"null pointer" in err()
    assert L.csa_beam_row_topk(16, 4, 60, 4, 18, 16, 16, None, 0, None) == 1 and b"misaligned" in err()
    assert L.csa_beam_row_topk(16, 4, 60, 4, 16, 16, 16, 18, 5, None) == 1 and b"misaligned" in err()
    assert L.csa_beam_row_topk(16, 4, 60, 0, 16, 16, 16, None, 0, None) == 2 and b"W must be" in err()
    assert L.csa_beam_row_topk(16, 4, 60, 9, 16, 16, 16, None, 0, None) == 2 and b"W must be" in err()
    assert L.csa_beam_row_topk(16, 4, 3, 4, 16, 16, 16, None, 0, None) == 1 and b"at least W" in err()
    assert L.csa_beam_row_topk(16, 0, 60, 4, 16, 16, 16, None, 0, None) == 0  # nothing to do, no launch
    # csa_beam_select(args, stream)
    assert L.csa_beam_select(None, None) == 1 and b"csa_beam_select" in err() and b"null args" in err()

    def sel(**kw):
        base = dict(B=2, W=4, T=6, topv=16, topi=16, lse=16, cum=16, fin=16, tokens=16, tok_stride=6, pad=16,
                    pad_stride=6, anc=16, anc_stride=6, parent=None, eos_id=3, pad_id=0, t_dev=16)
        base.update(kw)
        a = _lib.BeamSelectArgs(**base)
        return L.csa_beam_select(ctypes.byref(a), None)
    assert sel(W=9) == 2 and b"W must be" in err()
    assert sel(W=0) == 2 and sel(T=257) == 2 and sel(T=1) == 2
    for name in ("topv", "topi", "lse", "cum", "fin", "tokens", "pad", "anc", "t_dev"):
        assert sel(**{name: None}) == 1 and b"null pointer" in err(), name
    for name, bad in (("topv", 18), ("topi", 18), ("lse", 17), ("cum", 18), ("tokens", 20), ("anc", 18), ("parent", 18),
                      ("t_dev", 17)):
        assert sel(**{name: bad}) == 1 and b"misaligned" in err(), name
    assert sel(tok_stride=5) == 1 and sel(pad_stride=5) == 1 and sel(anc_stride=5) == 1 and b"stride" in err()
    assert sel(B=0) == 0  # nothing to do, no launch


def test_beam_supported_states_its_limits():
    from csa_amd import _lib
    L = _lib.lib()
    assert L.csa_beam_supported(1, 2) and L.csa_beam_supported(8, 256) and L.csa_beam_supported(4, 50)
    assert not L.csa_beam_supported(0, 50) and not L.csa_beam_supported(9, 50)
    assert not L.csa_beam_supported(4, 1) and not L.csa_beam_supported(4, 257)


def test_beam_generator_is_exported_beside_the_greedy_ones():
    from csa_amd import model
    assert issubclass(model.BeamSearchGenerator, torch.nn.Module)
    assert not issubclass(model.BeamSearchGenerator, model.GreedyGenerator)
    cache = model.BaseDecoder(model.DecoderLayer(32, 4, 64, 0.1), 1).make_cache(torch.zeros(2, 5, 32), None, 6, beam=3)
    assert cache.self_k[0].shape == (6, 4, 6, 8) and cache.memory_kv[0].shape == (2, 5, 2, 4, 8)
    assert cache.anc.shape == (6, 6) and cache.anc.dtype == torch.int32 and cache.kv_group == 3 and cache.pad.shape == (6, 6)
