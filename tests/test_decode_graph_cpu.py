"""Device-stepped decoding without a GPU: host-side validation of the three entry points that read the step from a device
counter, the tensor-step plumbing of csa_amd.decode_ops on CPU tensors (where the counter is read on the host), and
CachedGreedyGenerator(graph=True) deferring to the eager loop on a CPU model."""
import ctypes
from types import SimpleNamespace

import pytest
import torch


def _attn_args(_lib, **kw):
    base = dict(B=2, H=3, hd=8, len=4, q=16, K=16, V=16, out=16, k_new=16, v_new=16, q_sb=24, q_sh=8, k_sb=96, k_sh=32,
                k_sn=8, v_sb=96, v_sh=32, v_sn=8, kn_sb=24, kn_sh=8, vn_sb=24, vn_sh=8)
    base.update(kw)
    return _lib.DecodeAttnArgs(**base)


def test_decode_attn_step_validates_without_gpu():
    from csa_amd import _lib
    L = _lib.lib()
    err = L.csa_last_error_str
    assert L.csa_decode_attn_step(None, 16, None) == 1
    assert b"csa_decode_attn_step" in err() and b"null args" in err()
    a = _attn_args(_lib)
    assert L.csa_decode_attn_step(ctypes.byref(a), None, None) == 1  # no counter
    assert b"csa_decode_attn_step" in err() and b"t_dev" in err()
    assert L.csa_decode_attn_step(ctypes.byref(a), 18, None) == 1    # counter not 4-byte aligned
    assert b"csa_decode_attn_step" in err() and b"t_dev" in err()
    a = _attn_args(_lib, k_new=None, v_new=None)                     # not append mode
    assert L.csa_decode_attn_step(ctypes.byref(a), 16, None) == 1
    assert b"csa_decode_attn_step" in err() and b"required" in err()
    a = _attn_args(_lib, q=None)
    assert L.csa_decode_attn_step(ctypes.byref(a), 16, None) == 1
    assert b"csa_decode_attn_step" in err() and b"null pointer" in err()
    a = _attn_args(_lib, V=20)
    assert L.csa_decode_attn_step(ctypes.byref(a), 16, None) == 1
    assert b"csa_decode_attn_step" in err() and b"aligned" in err()
    a = _attn_args(_lib, hd=6)
    assert L.csa_decode_attn_step(ctypes.byref(a), 16, None) == 2
    # a->t is ignored: no "len == t + 1" demand, and the host-step sibling still makes it
    a = _attn_args(_lib, t=0, q=None)
    assert L.csa_decode_attn_step(ctypes.byref(a), 16, None) == 1 and b"null pointer" in err()
    assert L.csa_decode_attn(ctypes.byref(a), None) == 1 and b"csa_decode_attn: " in err() and b"len == t + 1" in err()


def test_decode_embed_validates_without_gpu():
    from csa_amd import _lib
    L = _lib.lib()
    err = L.csa_last_error_str
    # (ys, ys_stride, B, T, t_dev, W, vocab, pe, max_len, gamma, beta, eps, x, E, stream)
    ok = [16, 9, 2, 9, 16, 16, 37, 16, 5000, 16, 16, 1e-5, 16, 64, None]

    def call(**kw):
        names = ["ys", "ys_stride", "B", "T", "t_dev", "W", "vocab", "pe", "max_len", "gamma", "beta", "eps", "x", "E",
                 "stream"]
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return L.csa_decode_embed(*args)
    for name in ("ys", "t_dev", "W", "gamma", "beta", "x"):
        assert call(**{name: None}) == 1, name
        assert b"csa_decode_embed" in err() and b"null pointer" in err(), name
    for name, bad in (("ys", 20), ("t_dev", 18), ("W", 24), ("pe", 24), ("gamma", 8), ("beta", 4), ("x", 40)):
        assert call(**{name: bad}) == 1, name
        assert b"csa_decode_embed" in err() and b"misaligned" in err(), name
    assert call(E=6) == 2 and b"csa_decode_embed" in err()
    assert call(E=1028) == 2
    assert call(ys_stride=8) == 1 and b"csa_decode_embed" in err()  # rows overlap
    assert call(vocab=0) == 1
    assert call(B=0) == 0  # nothing to do, no launch


def test_argmax_rows_step_validates_without_gpu():
    from csa_amd import _lib
    L = _lib.lib()
    err = L.csa_last_error_str
    # (x, rows, V, ys, ys_stride, T, pad, pad_stride, head_pad, H, pad_id, t_dev, stream)
    ok = [16, 3, 60, 16, 6, 6, 16, 6, 16, 2, 0, 16, None]

    def call(**kw):
        names = ["x", "rows", "V", "ys", "ys_stride", "T", "pad", "pad_stride", "head_pad", "H", "pad_id", "t_dev", "stream"]
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return L.csa_argmax_rows_step(*args)
    for name in ("x", "ys", "t_dev"):
        assert call(**{name: None}) == 1, name
        assert b"csa_argmax_rows_step" in err() and b"null pointer" in err(), name
    for name, bad in (("x", 18), ("ys", 20), ("t_dev", 17)):
        assert call(**{name: bad}) == 1, name
        assert b"csa_argmax_rows_step" in err() and b"misaligned" in err(), name
    assert call(V=0) == 1 and b"csa_argmax_rows_step" in err()
    assert call(ys_stride=5) == 1 and call(pad_stride=5) == 1 and call(H=0) == 1
    assert call(rows=0) == 0  # nothing to do, no launch


def test_decode_attention_with_a_cpu_tensor_step_equals_the_int_step():
    from csa_amd.decode_ops import decode_attention
    torch.manual_seed(1)
    B, H, hd, cap = 2, 3, 8, 6
    mask = torch.zeros(B, H, cap, dtype=torch.uint8)
    mask[1, :, 1] = 1
    host = torch.randn(2, B, H, cap, hd)
    dev = host.clone()
    for t in (0, 3, cap - 1):
        q, kn, vn = torch.randn(B, 3, H, hd).unbind(1)
        want = decode_attention(q, host[0], host[1], key_mask=mask, k_new=kn, v_new=vn, t=t)
        out = torch.empty(B, H * hd)
        got = decode_attention(q, dev[0], dev[1], key_mask=mask, k_new=kn, v_new=vn,
                               t=torch.tensor([t], dtype=torch.int32), out=out)
        assert got is out and torch.equal(got, want) and torch.equal(dev, host)
    q, kn, vn = torch.randn(B, 3, H, hd).unbind(1)
    with pytest.raises(ValueError):  # the host sees the value here
        decode_attention(q, dev[0], dev[1], k_new=kn, v_new=vn, t=torch.tensor([cap], dtype=torch.int32))
    with pytest.raises(ValueError):  # int64 is not the counter's type
        decode_attention(q, dev[0], dev[1], k_new=kn, v_new=vn, t=torch.tensor([1]))
    with pytest.raises(ValueError):  # a device step is an append
        decode_attention(q, dev[0], dev[1], t=torch.tensor([1], dtype=torch.int32))
    assert torch.equal(dev, host)


def test_argmax_rows_with_a_cpu_tensor_step_equals_the_eager_sequence():
    from csa_amd.decode_ops import argmax_rows
    rows, V, H, T = 3, 11, 2, 6
    x = torch.randn(rows, V, generator=torch.Generator().manual_seed(3))
    x[1, 0] = 50.0
    x[2, [7, 4]] = 60.0

    def buffers():
        return (torch.full((rows, T), 9, dtype=torch.long), torch.full((rows, T), 5, dtype=torch.uint8),
                torch.full((rows, H, T), 3, dtype=torch.uint8))
    for t in (0, 4):
        ys_e, pad_e, hp_e = buffers()
        argmax_rows(x, out=ys_e[:, t + 1], is_pad=pad_e[:, t + 1], pad_id=0)
        hp_e.view(H, rows, T)[:, :, t + 1] = pad_e[:, t + 1]
        assert ys_e[:, t + 1].tolist()[1:] == [0, 4]
        ys_d, pad_d, hp_d = buffers()
        t_dev = torch.tensor([t], dtype=torch.int32)
        assert argmax_rows(x, out=ys_d, is_pad=pad_d, pad_id=0, t_dev=t_dev, head_pad=hp_d) is ys_d
        assert torch.equal(ys_d, ys_e) and torch.equal(pad_d, pad_e) and torch.equal(hp_d, hp_e)
        ys_n, pad_n, hp_n = buffers()
        argmax_rows(x, out=ys_n, is_pad=pad_n, pad_id=0, t_dev=t_dev)
        assert torch.equal(ys_n, ys_e) and torch.equal(pad_n, pad_e) and bool((hp_n == 3).all())
    ys, pad, hp = buffers()
    with pytest.raises(ValueError):
        argmax_rows(x, out=ys, is_pad=pad, t_dev=torch.tensor([T - 1], dtype=torch.int32))
    with pytest.raises(ValueError):
        argmax_rows(x, out=ys[:, 1], is_pad=pad[:, 1], head_pad=hp)  # head_pad goes with t_dev


def test_decode_embed_with_a_cpu_tensor_step_equals_embeddings_step():
    from csa_amd.decode_ops import decode_embed
    from csa_amd.model import Embeddings
    torch.manual_seed(0)
    emb = Embeddings(32, 20, 0.1, with_pos=True).eval()
    ys = torch.randint(0, 20, (3, 9))[:, 1:7]
    with torch.no_grad():
        for t in (0, 5):
            t_dev = torch.tensor([t], dtype=torch.int32)
            want = emb.step(ys[:, t:t + 1], t)
            assert torch.equal(decode_embed(ys, t_dev, emb), want[:, 0])
            assert torch.equal(emb.step(ys, t_dev), want)
    with pytest.raises(ValueError):
        decode_embed(ys, torch.tensor([6], dtype=torch.int32), emb)
    with pytest.raises(ValueError):
        decode_embed(ys, torch.tensor([0], dtype=torch.int32), emb.train())


def test_decoder_step_with_a_cpu_counter_equals_the_int_step():
    from csa_amd.glue import LayerNorm
    from csa_amd.model import PAD, BaseDecoder, DecoderLayer
    torch.manual_seed(3)
    B, S, T, E, H = 3, 11, 5, 64, 8
    dec = BaseDecoder(DecoderLayer(E, H, 128, 0.2), 2, norm=LayerNorm(E)).eval()
    tokens = torch.tensor([[1, 5, 9, 4, 7], [1, 6, PAD, 2, PAD], [1, 3, PAD, 8, 5]])
    src_mask = torch.zeros(B, S, dtype=torch.bool)
    src_mask[2, 5:] = True
    memory, x = torch.randn(B, S, E), torch.randn(B, T, E)
    with torch.no_grad():
        host = dec.make_cache(memory, src_mask, T, repeat_heads=True)
        dev = dec.make_cache(memory, src_mask, T, repeat_heads=True)
        for c in (host, dev):
            c.pad.copy_(tokens == PAD)
        dev.head_pad.view(H, B, T).copy_(dev.pad.unsqueeze(0).expand(H, B, T))  # the counter path copies no column
        for t in range(T):
            want = dec.step(x[:, t:t + 1], host, t)
            got = dec.step(x[:, t:t + 1], dev, torch.tensor([t], dtype=torch.int32))
            assert torch.equal(got, want), t
    assert torch.equal(dev.head_pad, host.head_pad)


def test_graph_generator_on_a_cpu_model_is_the_eager_generator():
    """No CUDA model: graph=True captures nothing and returns what graph=False returns. The encoder's attention has no
    CPU path, so the encoder is replaced by a fixed memory here; the decode loop under test is untouched."""
    from csa_amd.glue import LayerNorm
    from csa_amd.model import (BaseDecoder, CachedGreedyGenerator, DecoderLayer, Embeddings, Generator)
    torch.manual_seed(5)
    B, S, E, H, V = 3, 7, 32, 4, 19
    enc = torch.randn(B, S, E)

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.tgt_embedding = Embeddings(E, V, 0.1, with_pos=True)
            self.decoder = BaseDecoder(DecoderLayer(E, H, 64, 0.2), 2, norm=LayerNorm(E))
            self.generator = Generator(V, E, 0.2)

        def process_data(self, data):
            data.src_mask = data.src_seq.eq(0)

        def encode(self, data):
            return enc, 1, None, [], []
    m = Stub().eval()
    src = torch.randint(1, 9, (B, S))
    src[1, 4:] = 0
    eager = CachedGreedyGenerator(m, 6)
    gen = CachedGreedyGenerator(m, 6, graph=True)
    want = eager(SimpleNamespace(src_seq=src))
    got = gen(SimpleNamespace(src_seq=src))
    assert got.shape == (B, 5) and torch.equal(got, want)
    assert gen.captures == 0 and eager.captures == 0 and eager.graph is False and gen.graph is True
