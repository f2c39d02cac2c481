"""Device-stepped decoding on the GPU: the kernels of one decode step reading the step index from a 4-byte device
counter (csa_decode_attn_step, csa_decode_embed, csa_argmax_rows_step) against the same calls with a host integer,
bitwise, and CachedGreedyGenerator(graph=True), which replays one captured HIP graph of that step, against the eager
cached generator and the reference fixture (tests/golden/greedy_tiny.npz)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import has_gpu
from golden_inputs import fill_params_deterministic

# the model of tests/golden/greedy_tiny.npz (tools/gen_golden.py; the same dims as test_decode_gpu.TINY)
TINY = dict(src_vocab_size=50, tgt_vocab_size=60, hidden_size=64, num_heads=8, num_layers=1, sbm_layers=2,
            use_pegen="pegen", dim_feed_forward=128, dropout=0.2, pe_dim=32, pegen_dim=128, sbm_enc_dim=512,
            clusters=[10, 12], full_att=False)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]

SENTINEL = 777.0


def _counter(v=0):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def _mask(kind, B, H, width, g):
    """(B, width) or per-head (B, H, width) uint8 key mask, about 40 % masked, key 0 live in every row."""
    shape = (B, width) if kind == "batch" else (B, H, width)
    m = (torch.rand(shape, generator=g) < 0.4).to(torch.uint8)
    m[..., 0] = 0
    return m.cuda()


# the last four: hd / 4 = 1, 3, 24 and 5 (3, 24 and 5 do not divide the wave), see test_decode_gpu.CASES
STEP_CASES = [(3, 5, 8, 70), (2, 8, 64, 130), (1, 1, 128, 66), (3, 5, 4, 70), (2, 3, 12, 130), (1, 2, 96, 66),
              (1, 5, 20, 130)]


@pytest.mark.parametrize("mask_kind", ["batch", "per_head"])
@pytest.mark.parametrize("B,H,hd,cap", STEP_CASES)
def test_device_step_attention_is_bitwise_the_host_step(B, H, hd, cap, mask_kind):
    """decode_attention with a tensor step equals the int-step call in `out` and in the whole cache, at both sides of
    the 64-key chunk boundary and at the last row; BH = 15 is not a multiple of the 4 waves of a workgroup. One counter
    tensor, one output buffer and one cache serve every step in turn: between two launches only the counter's value
    changes, as between two replays of a captured step."""
    from csa_amd.decode_ops import decode_attention
    g = torch.Generator().manual_seed(100 * cap + hd)
    mask = _mask(mask_kind, B, H, cap, g)
    cache0 = torch.randn(2, B, H, cap, hd, generator=g).cuda()
    host, dev = cache0.clone(), cache0.clone()
    t_dev, out_dev = _counter(), torch.empty(B, H * hd, device="cuda")
    for t in (0, 1, 63, 64, 65, cap - 1):
        q, kn, vn = torch.randn(B, 3, H, hd, generator=g).cuda().unbind(1)
        want = decode_attention(q, host[0], host[1], key_mask=mask, k_new=kn, v_new=vn, t=t)
        t_dev.fill_(t)
        got = decode_attention(q, dev[0], dev[1], key_mask=mask, k_new=kn, v_new=vn, t=t_dev, out=out_dev)
        assert got is out_dev
        assert torch.isfinite(want).all(), t
        assert torch.equal(got, want), t
        assert torch.equal(dev, host), t
        assert torch.equal(dev[0, :, :, t], kn) and torch.equal(dev[1, :, :, t], vn), t


def test_device_step_out_of_range_stores_nothing():
    """Counter == capacity: neither the cache nor `out` is written. K / V are allocated with capacity + 1 rows and
    declared with capacity, so even a launch without the guard would stay inside the allocation."""
    from csa_amd.decode_ops import decode_attention
    g = torch.Generator().manual_seed(4)
    B, H, hd, cap = 2, 3, 16, 70
    full = torch.randn(2, B, H, cap + 1, hd, generator=g).cuda()
    before = full.clone()
    mask = _mask("batch", B, H, cap + 1, g)
    q, kn, vn = torch.randn(B, 3, H, hd, generator=g).cuda().unbind(1)
    out = torch.full((B, H * hd), SENTINEL, device="cuda")
    decode_attention(q, full[0, :, :, :cap], full[1, :, :, :cap], key_mask=mask, k_new=kn, v_new=vn, t=_counter(cap),
                     out=out)
    assert bool((out == SENTINEL).all())
    assert torch.equal(full, before)
    # the same buffers with the counter back in range are written
    decode_attention(q, full[0, :, :, :cap], full[1, :, :, :cap], key_mask=mask, k_new=kn, v_new=vn,
                     t=_counter(cap - 1), out=out)
    assert torch.isfinite(out).all() and not bool((out == SENTINEL).any())
    assert torch.equal(full[0, :, :, cap - 1], kn) and torch.equal(full[:, :, :, cap], before[:, :, :, cap])


@pytest.mark.parametrize("t", [0, 7])
@pytest.mark.parametrize("B,E", [(1, 8), (3, 512), (64, 1024)])
def test_decode_embed_is_bitwise_embeddings_step(B, E, t):
    from csa_amd.decode_ops import decode_embed
    from csa_amd.model import Embeddings
    torch.manual_seed(E + t)
    vocab, T = 37, 9
    emb = Embeddings(E, vocab, 0.1, with_pos=True).cuda().eval()
    with torch.no_grad():
        emb.norm.weight.add_(0.1 * torch.randn_like(emb.norm.weight))
        emb.norm.bias.add_(0.1 * torch.randn_like(emb.norm.bias))
        emb.word_embeddings.weight[0].normal_()  # the padding row, zero at init
    buf = torch.randint(0, vocab, (B, T + 5), device="cuda")
    ys = buf[:, 2:2 + T]  # row stride T + 5, storage offset 2
    ys[0, t] = 0 if (B > 1 or t == 0) else vocab - 1  # both ends of the table are gathered, also with one row
    if B > 1:
        ys[B - 1, t] = vocab - 1
    with torch.no_grad():
        want = emb.step(ys[:, t:t + 1], t)
        got = decode_embed(ys, _counter(t), emb)
        again = emb.step(ys, _counter(t))
    assert got.shape == (B, E) and want.shape == (B, 1, E) and again.shape == (B, 1, E)
    assert torch.equal(got, want[:, 0]) and torch.equal(again, want)


@pytest.mark.parametrize("t", [0, 4])
@pytest.mark.parametrize("V", [60, 1023])
def test_argmax_rows_step_writes_column_t_plus_1_of_every_buffer(V, t):
    """ys / pad / the (H, B, T) head_pad layout after the device-stepped call equal the eager sequence (argmax_rows into
    column t + 1, then the copy BaseDecoder.step makes at the top of step t + 1), every other byte keeps its sentinel."""
    from csa_amd.decode_ops import argmax_rows
    rows, H, T = 3, 2, 6
    x = torch.randn(rows, V, generator=torch.Generator().manual_seed(V + t))
    x[1, 0] = 50.0                      # row 1 picks PAD (id 0)
    x[2, [41, 7, V - 1]] = 1e9          # a tie: the lowest index wins
    x = x.cuda()

    def buffers():
        return (torch.full((rows, T), 9, dtype=torch.long, device="cuda"),
                torch.full((rows, T), 5, dtype=torch.uint8, device="cuda"),
                torch.full((rows, H, T), 3, dtype=torch.uint8, device="cuda"))
    ys_e, pad_e, hp_e = buffers()
    argmax_rows(x, out=ys_e[:, t + 1], is_pad=pad_e[:, t + 1], pad_id=0)
    hp_e.view(H, rows, T)[:, :, t + 1] = pad_e[:, t + 1]
    assert ys_e[:, t + 1].tolist()[1:] == [0, 7] and pad_e[:, t + 1].tolist()[1:] == [1, 0]
    ys_d, pad_d, hp_d = buffers()
    assert argmax_rows(x, out=ys_d, is_pad=pad_d, pad_id=0, t_dev=_counter(t), head_pad=hp_d) is ys_d
    assert torch.equal(ys_d, ys_e) and torch.equal(pad_d, pad_e) and torch.equal(hp_d, hp_e)
    ys_n, pad_n, hp_n = buffers()
    argmax_rows(x, out=ys_n, is_pad=pad_n, pad_id=0, t_dev=_counter(t))  # no per-head mask
    assert torch.equal(ys_n, ys_e) and torch.equal(pad_n, pad_e) and bool((hp_n == 3).all())
    # a column outside [1, T) stores nothing
    ys_o, pad_o, hp_o = buffers()
    argmax_rows(x, out=ys_o, is_pad=pad_o, pad_id=0, t_dev=_counter(T - 1), head_pad=hp_o)
    assert bool((ys_o == 9).all()) and bool((pad_o == 5).all()) and bool((hp_o == 3).all())


@pytest.mark.parametrize("repeat_heads", [False, True])
def test_decoder_step_with_the_counter_is_bitwise_the_int_step(repeat_heads):
    """BaseDecoder.step at the production head dim (hd = 64, S = 150 with source pads, PAD target keys), teacher-forced:
    the counter path gives the int path's rows and caches bit for bit. With the counter the decoder copies no head_pad
    column (the argmax kernel writes it during decoding), so the per-head mask is filled up front here."""
    from csa_amd.glue import LayerNorm
    from csa_amd.model import PAD, BaseDecoder, DecoderLayer
    torch.manual_seed(9)
    B, S, T, E, H = 2, 150, 9, 512, 8
    dec = BaseDecoder(DecoderLayer(E, H, 2048, 0.2), 2, norm=LayerNorm(E)).cuda().eval()
    tokens = torch.tensor([[1, 4, 7, 2, 9, 5, 3, 8, 6], [1, 5, 3, PAD, 8, PAD, 4, 2, 7]], device="cuda")
    src_mask = torch.zeros(B, S, dtype=torch.bool, device="cuda")
    src_mask[0, 120:] = True
    src_mask[1, 37:] = True
    memory = torch.randn(B, S, E, device="cuda")
    x = torch.randn(B, T, E, device="cuda")
    t_dev = _counter()
    with torch.no_grad():
        host = dec.make_cache(memory, src_mask, T, repeat_heads=repeat_heads)
        dev = dec.make_cache(memory, src_mask, T, repeat_heads=repeat_heads)
        for c in (host, dev):
            c.pad.copy_(tokens == PAD)
        if repeat_heads:
            dev.head_pad.view(H, B, T).copy_(dev.pad.unsqueeze(0).expand(H, B, T))
        for t in range(T):
            want = dec.step(x[:, t:t + 1], host, t)
            t_dev.fill_(t)
            got = dec.step(x[:, t:t + 1], dev, t_dev)
            assert torch.isfinite(want).all() and torch.equal(got, want), t
    for i in range(2):
        assert torch.equal(dev.self_k[i], host.self_k[i]) and torch.equal(dev.self_v[i], host.self_v[i])
    if repeat_heads:
        assert torch.equal(dev.head_pad, host.head_pad)


def _tiny_model_and_data(z):
    """The fixture's model, and data(n): a fresh batch of its first n samples with the fixture's uniforms armed for the
    next encode (SBMAttention consumes them)."""
    from csa_amd.model import CSATrans
    seed, max_len = (int(v) for v in z["meta"])
    m = CSATrans(**TINY)
    fill_params_deterministic(m, seed)
    with torch.no_grad():
        m.generator.linear.weight.mul_(8.0)
    m = m.cuda().eval()
    full = z["src_seq"].shape[0]

    def data(n=full):
        c = lambda k, dt: torch.from_numpy(z[k][:n]).to(dt).cuda()
        for i in range(2):
            getattr(m.SBM, f"transformer_{i}").mha.attn.uniforms = torch.from_numpy(z[f"u{i}"][:n]).cuda()
        return SimpleNamespace(src_seq=c("src_seq", torch.int64), tgt_seq=None, L=c("L", torch.uint8),
                               T=c("T", torch.uint8), L_mask=c("L_mask", torch.uint8), T_mask=c("T_mask", torch.uint8))
    return m, data, max_len, full


def test_graph_generator_matches_fixture_and_eager_and_recaptures_per_shape(golden, monkeypatch):
    from csa_amd import decode_ops
    from csa_amd.model import CachedGreedyGenerator
    z = golden("greedy_tiny")
    m, data, max_len, B = _tiny_model_and_data(z)
    eager = CachedGreedyGenerator(m, max_len)
    gen = CachedGreedyGenerator(m, max_len, graph=True)
    assert eager.graph is False and gen.captures == 0
    ys_e, lp_e = eager(data(), return_logp=True)
    ys1, lp1 = gen(data(), return_logp=True)
    assert gen.captures == 1
    np.testing.assert_array_equal(ys1.cpu().numpy(), z["ys"])
    assert lp1.shape == z["step_logp"].shape
    np.testing.assert_allclose(lp1.cpu().numpy(), z["step_logp"], rtol=1e-4, atol=1e-4)
    assert torch.equal(ys1, ys_e) and torch.equal(lp1, lp_e)

    # a replayed call issues no attention launch from Python
    calls = {"hip": 0}
    hip = decode_ops._decode_attention_hip

    def counted(*a):
        calls["hip"] += 1
        return hip(*a)
    monkeypatch.setattr(decode_ops, "_decode_attention_hip", counted)
    ys2, lp2 = gen(data(), return_logp=True)
    assert calls["hip"] == 0 and gen.captures == 1
    monkeypatch.setattr(decode_ops, "_decode_attention_hip", hip)
    assert torch.equal(ys2, ys1) and torch.equal(lp2, lp1)
    assert ys2.data_ptr() != ys1.data_ptr()  # clones, not views of the static buffers

    # another batch size is another graph; the first one is kept
    ys_s, lp_s = gen(data(B - 1), return_logp=True)
    assert gen.captures == 2
    ys_se, lp_se = eager(data(B - 1), return_logp=True)
    assert ys_s.shape == (B - 1, max_len - 1) and torch.equal(ys_s, ys_se) and torch.equal(lp_s, lp_se)
    ys3, lp3 = gen(data(), return_logp=True)
    assert gen.captures == 2
    assert torch.equal(ys3, ys1) and torch.equal(lp3, lp1)


def test_graph_generator_sees_in_place_weight_updates_without_recapture(golden):
    from csa_amd.model import CachedGreedyGenerator
    z = golden("greedy_tiny")
    m, data, max_len, _ = _tiny_model_and_data(z)
    eager = CachedGreedyGenerator(m, max_len)
    gen = CachedGreedyGenerator(m, max_len, graph=True)
    before = gen(data())
    assert gen.captures == 1 and torch.equal(before, eager(data()))
    with torch.no_grad():
        m.generator.linear.bias[5] += 100.0  # in place: the same storage, token 5 now wins every step
    after = gen(data())
    assert gen.captures == 1
    assert not torch.equal(after, before) and bool((after == 5).all())
    assert torch.equal(after, eager(data()))


def test_graph_generator_keeps_at_most_four_graphs(golden):
    from csa_amd.model import CachedGreedyGenerator
    z = golden("greedy_tiny")
    m, data, _, B = _tiny_model_and_data(z)
    gen = CachedGreedyGenerator(m, 3, graph=True)
    want = {}
    for n in (B, B - 1, B - 2):
        for logp in (False, True):
            if len(want) == 5:
                break
            want[(n, logp)] = gen(data(n), return_logp=logp)
    assert gen.captures == 5 and len(gen._graphs) == gen.MAX_GRAPHS
    first = gen(data(B))  # evicted as the oldest: captured again, same ids
    assert gen.captures == 6 and len(gen._graphs) == gen.MAX_GRAPHS
    assert torch.equal(first, want[(B, False)])
