"""KV-cached decoding without a GPU: BaseDecoder.step (the cached algorithm, on the SDPA / torch.max fallback of
csa_amd.decode_ops) against the full BaseDecoder.forward, and the host-side validation of the ABI v10 entry points."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("repeat_heads", [False, True])
def test_decoder_step_matches_full_pass_teacher_forced(repeat_heads):
    """Feeding positions 0..T-1 one at a time through BaseDecoder.step reproduces rows [:, t, :] of the full pass
    over the same forced tokens (PAD at positions 2 and 4 of some rows, key mask from make_std_mask) and the same
    padded source. Both sides torch fp32 on the CPU. The (B*H, T, T) mask of the full pass is make_std_mask per
    sample (repeat_interleave), or, with repeat_heads, the reference decode()'s `.repeat(num_heads, 1, 1)`, under
    which head h of sample b sees the PAD columns of sample (b * H + h) % B."""
    from csa_amd.glue import LayerNorm
    from csa_amd.model import PAD, BaseDecoder, DecoderLayer, make_std_mask
    torch.manual_seed(3)
    B, S, T, E, H = 3, 11, 7, 64, 8
    dec = BaseDecoder(DecoderLayer(E, H, 128, 0.2), 2, norm=LayerNorm(E)).eval()
    with torch.no_grad():
        for p in dec.parameters():  # non-trivial biases and norm weights too
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    tokens = torch.tensor([[1, 5, 9, 4, 7, 3, 8],
                           [1, 6, PAD, 2, PAD, 9, 4],
                           [1, 3, PAD, 8, 5, 2, 6]])
    src_mask = torch.zeros(B, S, dtype=torch.bool)
    src_mask[0, 8:] = True
    src_mask[2, 5:] = True
    memory = torch.randn(B, S, E)
    x = torch.randn(B, T, E)  # the embedded target positions
    with torch.no_grad():
        std = make_std_mask(tokens, PAD)
        tgt_mask = std.repeat(H, 1, 1) if repeat_heads else std.repeat_interleave(H, 0)
        full, _ = dec(x.permute(1, 0, 2), memory.permute(1, 0, 2), tgt_mask, memory_key_padding_mask=src_mask)
        full = full.permute(1, 0, 2)
        cache = dec.make_cache(memory, src_mask, T, repeat_heads=repeat_heads)
        cache.pad.copy_(tokens == PAD)
        for t in range(T):
            y = dec.step(x[:, t:t + 1], cache, t)
            assert y.shape == (B, 1, E)
            np.testing.assert_allclose(y[:, 0].numpy(), full[:, t].numpy(), rtol=1e-5, atol=1e-6, err_msg=f"t={t}")


@pytest.mark.parametrize("options", [{}, {"repeat_heads": True}, {"beam": 3}], ids=["plain", "repeat_heads", "beam3"])
def test_empty_cache_then_load_memory_is_make_cache(options):
    """The static cache of the captured graphs (empty_cache(S=) + load_memory) against the eager one (make_cache): the
    same fields, shapes, dtypes and None-ness, the same memory projections and mask; no mask leaves the static mask
    zeroed where make_cache keeps None."""
    from beam_ref import search_case
    m, enc, src_mask = search_case()  # E=32, H=4, two layers, B=3, S=7, a padded source row
    dec, T = m.decoder, 3
    B, S, _ = enc.shape
    assert bool(src_mask.any())
    with torch.no_grad():
        want = dec.make_cache(enc, src_mask, T, **options)
        got = dec.empty_cache(B, T, enc.device, enc.dtype, S=S, **options)
        assert all(not bool(kv.any()) for kv in got.memory_kv) and not bool(got.memory_mask.any())
        dec.load_memory(got, enc, src_mask)
    assert vars(got).keys() == vars(want).keys()
    assert got.kv_group == want.kv_group == options.get("beam", 1)
    assert (got.head_pad is None) == (want.head_pad is None) == ("repeat_heads" not in options)
    assert (got.anc is None) == (want.anc is None) == ("beam" not in options)
    for name in ("self_k", "self_v", "memory_kv", "memory_mask", "pad", "head_pad", "anc"):
        a, b = (v if isinstance(v, list) else [v] for v in (getattr(got, name), getattr(want, name)))
        assert len(a) == len(b) == (2 if name in ("self_k", "self_v", "memory_kv") else 1), name
        for x, y in zip(a, b):
            if y is not None:
                assert x.shape == y.shape and x.dtype == y.dtype and x.device == y.device, name
                assert torch.equal(x, y), name
    with torch.no_grad():
        dec.load_memory(got, enc, None)
        assert dec.make_cache(enc, None, T, **options).memory_mask is None
    assert got.memory_mask.shape == (B, S) and not bool(got.memory_mask.any())
    assert all(torch.equal(x, y) for x, y in zip(got.memory_kv, want.memory_kv))


def test_fallbacks_refuse_a_counter_outside_its_range():
    """Off the HIP path the host reads the device counter, and a step outside the op's range raises: one step below
    the range and the upper bound itself, for each op that takes a counter."""
    import beam_ref
    from csa_amd.decode_ops import argmax_rows, beam_row_topk, decode_attention, decode_embed
    from csa_amd.model import Embeddings
    counter = lambda t: torch.tensor([t], dtype=torch.int32)
    B, H, hd, cap, T, V = 2, 3, 8, 6, 5, 11
    q, kn, vn = torch.randn(B, 3, H, hd).unbind(1)
    K, Vc = torch.randn(2, B, H, cap, hd).unbind(0)
    x = torch.randn(B, V)
    ys, pad = torch.zeros(B, T, dtype=torch.long), torch.zeros(B, T, dtype=torch.uint8)
    emb = Embeddings(32, 20, 0.1, with_pos=True).eval()
    _, state, _ = beam_ref.select_states()[0]
    ops = {  # op -> (call with a step, the range's upper bound)
        "decode_attention": (lambda t: decode_attention(q, K, Vc, k_new=kn, v_new=vn, t=counter(t)), cap),
        "argmax_rows": (lambda t: argmax_rows(x, out=ys, is_pad=pad, t_dev=counter(t)), T - 1),
        "decode_embed": (lambda t: decode_embed(ys, counter(t), emb), T),
        "beam_row_topk": (lambda t: beam_row_topk(x, 4, t_dev=counter(t), t_end=T - 1), T - 1),
        "beam_select": (lambda t: beam_ref.run_select(state, t=t), state["T"] - 1),
    }
    with torch.no_grad():
        for name, (call, hi) in ops.items():
            call(hi - 1)  # the last step of the range is taken
            for t in (-1, hi):
                with pytest.raises(ValueError, match=f"{name}: step {t} outside"):
                    call(t)


def test_embedding_step_is_the_full_pass_row():
    from csa_amd.model import Embeddings
    torch.manual_seed(0)
    emb = Embeddings(32, 20, 0.1, with_pos=True).eval()
    ids = torch.randint(0, 20, (3, 6))
    with torch.no_grad():
        full = emb(ids)
        for t in range(6):
            torch.testing.assert_close(emb.step(ids[:, t:t + 1], t), full[:, t:t + 1], rtol=0, atol=0)


def test_decode_ops_fallback_matches_definition():
    """decode_attention / argmax_rows on CPU tensors: append writes row t only, masked keys drop out, the argmax lands
    in a strided column with its PAD byte."""
    from csa_amd.decode_ops import argmax_rows, decode_attention
    torch.manual_seed(1)
    B, H, hd, Tmax, t = 2, 3, 8, 6, 3
    q, kn, vn = (torch.randn(B, H, hd) for _ in range(3))
    K = torch.randn(B, H, Tmax, hd)
    V = torch.randn(B, H, Tmax, hd)
    K0, V0 = K.clone(), V.clone()
    mask = torch.zeros(B, Tmax, dtype=torch.uint8)
    mask[1, 1] = 1
    o = decode_attention(q, K, V, key_mask=mask, k_new=kn, v_new=vn, t=t)
    assert torch.equal(K[:, :, t], kn) and torch.equal(V[:, :, t], vn)
    keep = [j for j in range(Tmax) if j != t]
    assert torch.equal(K[:, :, keep], K0[:, :, keep]) and torch.equal(V[:, :, keep], V0[:, :, keep])
    s = torch.einsum("bhd,bhjd->bhj", q, K[:, :, :t + 1]) * hd ** -0.5
    s = s.masked_fill(mask[:, None, :t + 1].bool(), float("-inf"))
    ref = torch.einsum("bhj,bhjd->bhd", s.softmax(-1), V[:, :, :t + 1]).reshape(B, H * hd)
    torch.testing.assert_close(o, ref, rtol=1e-5, atol=1e-6)
    x = torch.tensor([[0.5, 2.0, 2.0], [3.0, -1.0, 0.0]])
    ys = torch.full((2, 4), 7, dtype=torch.long)
    pad = torch.zeros(2, 4, dtype=torch.uint8)
    argmax_rows(x, out=ys[:, 2], is_pad=pad[:, 2], pad_id=0)
    assert ys.tolist() == [[7, 7, 1, 7], [7, 7, 0, 7]] and pad.tolist() == [[0, 0, 0, 0], [0, 0, 1, 0]]


def test_decode_entry_points_validate_without_gpu():
    from csa_amd import _lib
    L = _lib.lib()
    assert L.csa_abi_version() == 10
    assert L.csa_decode_attn(None, None) == 1
    assert b"null args" in L.csa_last_error_str()
    assert L.csa_argmax_rows(None, 4, 16, None, 1, None, 0, 0, None, None) == 1
    assert b"csa_argmax_rows" in L.csa_last_error_str()
    a = _lib.DecodeAttnArgs(B=2, H=3, hd=8, len=0)  # len < 1
    assert L.csa_decode_attn(ctypes.byref(a), None) == 1
    a = _lib.DecodeAttnArgs(B=2, H=3, hd=6, len=4)  # unsupported head dim
    assert L.csa_decode_attn(ctypes.byref(a), None) == 2
    a = _lib.DecodeAttnArgs(B=2, H=3, hd=8, len=4, t=2, k_new=16, v_new=16)  # append: t + 1 != len
    assert L.csa_decode_attn(ctypes.byref(a), None) == 1
    assert b"len == t + 1" in L.csa_last_error_str()
    a = _lib.DecodeAttnArgs(B=2, H=3, hd=8, len=4)  # null tensors
    assert L.csa_decode_attn(ctypes.byref(a), None) == 1
    a = _lib.DecodeAttnArgs(B=2, H=3, hd=8, len=4, q=16, K=16, V=20, out=16, q_sb=24, q_sh=8, k_sb=96, k_sh=32, k_sn=8,
                            v_sb=96, v_sh=32, v_sn=8)  # V not 16-byte aligned
    assert L.csa_decode_attn(ctypes.byref(a), None) == 1
    assert b"aligned" in L.csa_last_error_str()
    a.V, a.k_sn = 16, 6  # key stride not a multiple of 4 elements
    assert L.csa_decode_attn(ctypes.byref(a), None) == 1


def test_decode_attn_supported_head_dims():
    from csa_amd import _lib
    L = _lib.lib()
    assert L.csa_decode_attn_supported(8) and L.csa_decode_attn_supported(64) and L.csa_decode_attn_supported(128)
    assert not L.csa_decode_attn_supported(6) and not L.csa_decode_attn_supported(132)
    assert not L.csa_decode_attn_supported(0)


def test_cached_generator_is_exported_beside_the_plain_one():
    from csa_amd.model import CachedGreedyGenerator, GreedyGenerator
    assert issubclass(CachedGreedyGenerator, GreedyGenerator)
    import csa_amd.decoding
    import csa_amd.model
    for name in ("DecodingConstraints", "_SteppedDecoding", "CachedGreedyGenerator", "BeamSearchGenerator",
                 "SamplingGenerator"):
        assert getattr(csa_amd.model, name) is getattr(csa_amd.decoding, name), name
