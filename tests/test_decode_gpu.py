"""KV-cached greedy decoding on the GPU: k_decode_attn and k_argmax_rows (csrc/csa_decode.hip) against torch,
BaseDecoder.step against the full pass at the production head dim, and CachedGreedyGenerator against the reference's
GreedyGenerator fixture (tests/golden/greedy_tiny.npz) and against the uncached generator."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import has_gpu
from golden_inputs import fill_params_deterministic

# the model of tests/golden/greedy_tiny.npz (tools/gen_golden.py; the same dims as test_model_gpu.TINY)
TINY = dict(src_vocab_size=50, tgt_vocab_size=60, hidden_size=64, num_heads=8, num_layers=1, sbm_layers=2,
            use_pegen="pegen", dim_feed_forward=128, dropout=0.2, pe_dim=32, pegen_dim=128, sbm_enc_dim=512,
            clusters=[10, 12], full_att=False)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]

CASES = [(2, 3, 8, 1), (2, 3, 8, 7), (1, 2, 64, 64), (1, 2, 64, 65), (2, 8, 64, 150), (1, 1, 128, 130), (1, 2, 32, 300)]
# head dims whose float4 count hd / 4 does not divide the wave (64 % (hd / 4) lanes of the P.V phase idle), and hd = 4
# (one key group per lane); test_row_kernels_gpu.py asserts that this list, STEP_CASES of test_decode_graph_gpu.py and
# ATTN_CASES of test_beam_gpu.py keep them
CASES += [(2, 3, 4, 70), (2, 3, 12, 65), (1, 5, 20, 130), (1, 2, 40, 64), (2, 2, 96, 150), (1, 3, 124, 67)]
SENTINEL = 777.0


def _masks(B, n, g):
    """(name, (B, n + 5) uint8 mask or None): the variants of one case; the row stride exceeds n on purpose."""
    out = [("none", None)]
    m = (torch.rand(B, n + 5, generator=g) < 0.4).to(torch.uint8)
    m[:, 0] = 0
    out.append(("random", m))
    if n > 64:
        m = torch.zeros(B, n + 5, dtype=torch.uint8)
        m[:, :64] = 1
        out.append(("first_chunk_masked", m))
    if n > 128:
        m = torch.zeros(B, n + 5, dtype=torch.uint8)
        m[:, 64:128] = 1
        out.append(("second_chunk_masked", m))
    return out


def _ref_attention(q, k, v, mask, n):
    """fp64 on the CPU: q (B,H,hd), k / v (B,H,n,hd), mask (B,>=n) or (B,H,>=n) uint8 or None -> (B, H*hd)."""
    q, k, v = q.double(), k.double(), v.double()
    s = torch.einsum("bhd,bhjd->bhj", q, k) * q.shape[-1] ** -0.5
    if mask is not None:
        mk = mask[..., :n].bool()
        s = s.masked_fill(mk[:, None] if mk.dim() == 2 else mk, float("-inf"))
    return torch.einsum("bhj,bhjd->bhd", s.softmax(-1), v).reshape(q.shape[0], -1)


@pytest.mark.parametrize("layout", ["memory", "cache_append"])
@pytest.mark.parametrize("B,H,hd,n", CASES)
def test_decode_attention_matches_fp64(B, H, hd, n, layout):
    from csa_amd import decode_ops
    g = torch.Generator().manual_seed(1000 * n + hd)
    packed = torch.randn(B, 3, H, hd, generator=g)  # q / k_new / v_new as views of one packed projection row
    kv = torch.randn(B, n, 2, H, hd, generator=g)   # the (B, S, 2, H, hd) memory projection
    k_all, v_all = (u.transpose(1, 2) for u in kv.unbind(2))
    for name, mask in _masks(B, n, g):
        dm = None if mask is None else mask.cuda()
        dq, dkn, dvn = packed.cuda().unbind(1)
        if layout == "memory":
            dk, dv = (u.transpose(1, 2) for u in kv.cuda().unbind(2))
            out = decode_ops.decode_attention(dq, dk, dv, key_mask=dm)
            ref = _ref_attention(packed[:, 0], k_all, v_all, mask, n)
        else:
            t, tmax = n - 1, n + 3
            cache = torch.full((2, B, H, tmax, hd), SENTINEL)
            cache[0, :, :, :t] = k_all[:, :, :t]
            cache[1, :, :, :t] = v_all[:, :, :t]
            dc = cache.cuda()
            out = decode_ops.decode_attention(dq, dc[0], dc[1], key_mask=dm, k_new=dkn, v_new=dvn, t=t)
            got = dc.cpu()
            assert torch.equal(got[0, :, :, t], packed[:, 1]) and torch.equal(got[1, :, :, t], packed[:, 2]), name
            assert torch.equal(got[:, :, :, :t], cache[:, :, :, :t]), name
            assert bool((got[:, :, :, t + 1:] == SENTINEL).all()), name
            ref = _ref_attention(packed[:, 0], torch.cat([k_all[:, :, :t], packed[:, 1, :, None]], 2),
                                 torch.cat([v_all[:, :, :t], packed[:, 2, :, None]], 2), mask, n)
        assert out.shape == (B, H * hd) and out.is_contiguous()
        np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-5, err_msg=f"{name} {layout}")


def test_decode_attention_per_head_mask_and_all_masked_row():
    """A (B, H, L) mask is read per head; one (b, h) row with every key masked gives NaN there and only there."""
    from csa_amd.decode_ops import decode_attention
    g = torch.Generator().manual_seed(5)
    B, H, hd, n = 2, 3, 16, 70
    q = torch.randn(B, H, hd, generator=g)
    k, v = torch.randn(B, H, n, hd, generator=g), torch.randn(B, H, n, hd, generator=g)
    mask = (torch.rand(B, H, n, generator=g) < 0.5).to(torch.uint8)
    mask[..., 3] = 0
    mask[1, 2] = 1  # all keys of (b=1, h=2) masked
    out = decode_attention(q.cuda(), k.cuda(), v.cuda(), key_mask=mask.cuda()).cpu().view(B, H, hd)
    ref = _ref_attention(q, k, v, mask, n).view(B, H, hd)
    assert torch.isnan(out[1, 2]).all()
    live = torch.ones(B, H, dtype=torch.bool)
    live[1, 2] = False
    np.testing.assert_allclose(out[live].numpy(), ref[live].numpy(), rtol=1e-4, atol=1e-5)
    # (B, L) mask with one sample fully masked: NaN for all of its heads, no error
    m2 = torch.zeros(B, n, dtype=torch.uint8)
    m2[0] = 1
    out = decode_attention(q.cuda(), k.cuda(), v.cuda(), key_mask=m2.cuda()).cpu().view(B, H, hd)
    assert torch.isnan(out[0]).all() and torch.isfinite(out[1]).all()


@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("V", [1, 60, 1023, 20000])
def test_argmax_rows(rows, V):
    from csa_amd.decode_ops import argmax_rows
    g = torch.Generator().manual_seed(rows * 100003 + V)
    x = (torch.randperm(rows * V, generator=g).float() - rows * V / 2).view(rows, V)  # distinct values
    mx = torch.empty(rows, device="cuda")
    got = argmax_rows(x.cuda(), maxval=mx)
    assert torch.equal(got.cpu(), x.argmax(1)) and torch.equal(mx.cpu(), x.max(1).values)
    for at in (0, V - 1):  # the maximum planted at either end
        y = x.clone()
        y[:, at] = 1e9
        assert bool((argmax_rows(y.cuda()).cpu() == at).all())
    if V >= 60:  # duplicated maxima: the lowest index wins, wherever the copies sit
        y = x.clone()
        cols = torch.tensor([V - 1, V // 2, 7, 41])
        y[:, cols] = 1e9
        assert bool((argmax_rows(y.cuda()).cpu() == 7).all())
    y = x.clone()
    y[rows // 2] = float("-inf")  # an all -inf row gives 0
    got = argmax_rows(y.cuda()).cpu()
    assert got[rows // 2] == 0
    keep = torch.arange(rows) != rows // 2
    assert torch.equal(got[keep], x.argmax(1)[keep])
    assert bool(((got >= 0) & (got < V)).all())


def test_argmax_rows_writes_one_strided_column_and_the_pad_byte():
    from csa_amd.decode_ops import argmax_rows
    rows, V, T = 5, 60, 6
    x = torch.randn(rows, V, generator=torch.Generator().manual_seed(2))
    x[1, 0] = 50.0  # rows 1 and 3 pick PAD (id 0)
    x[3, 0] = 50.0
    ys = torch.full((rows, T), 9, dtype=torch.long, device="cuda")
    pad = torch.full((rows, T), 5, dtype=torch.uint8, device="cuda")
    argmax_rows(x.cuda(), out=ys[:, 3], is_pad=pad[:, 3], pad_id=0)
    want = x.argmax(1)
    ys, pad = ys.cpu(), pad.cpu()
    assert torch.equal(ys[:, 3], want) and want[1] == 0 and want[3] == 0
    assert torch.equal(pad[:, 3], (want == 0).to(torch.uint8))
    other = [0, 1, 2, 4, 5]
    assert bool((ys[:, other] == 9).all()) and bool((pad[:, other] == 5).all())


def _tiny_model_and_data(z):
    from csa_amd.model import CSATrans
    seed, max_len = (int(v) for v in z["meta"])
    m = CSATrans(**TINY)
    fill_params_deterministic(m, seed)
    with torch.no_grad():
        m.generator.linear.weight.mul_(8.0)
    m = m.cuda().eval()
    c = lambda k, dt: torch.from_numpy(z[k]).to(dt).cuda()

    def data():
        """A fresh batch, and the fixture's uniforms armed for the next encode (SBMAttention consumes them)."""
        for i in range(2):
            getattr(m.SBM, f"transformer_{i}").mha.attn.uniforms = torch.from_numpy(z[f"u{i}"]).cuda()
        return SimpleNamespace(src_seq=c("src_seq", torch.int64), tgt_seq=None, L=c("L", torch.uint8),
                               T=c("T", torch.uint8), L_mask=c("L_mask", torch.uint8), T_mask=c("T_mask", torch.uint8))
    return m, data, max_len


def test_cached_greedy_generator_matches_reference(golden):
    """The reference's GreedyGenerator fixture (hd = 8; source rows with 0, 2 and 3 pads): same ids, and per-step
    last-position log-probabilities within the fixture test's tolerance. The fixture's smallest top-2 log-probability
    gap is 0.0446, so 1e-4 cannot flip a token."""
    from csa_amd.model import CachedGreedyGenerator
    z = golden("greedy_tiny")
    m, data, max_len = _tiny_model_and_data(z)
    ys, logp = CachedGreedyGenerator(m, max_len)(data(), return_logp=True)
    assert logp.shape == z["step_logp"].shape
    np.testing.assert_allclose(logp.cpu().numpy(), z["step_logp"], rtol=1e-4, atol=1e-4)
    np.testing.assert_array_equal(ys.cpu().numpy(), z["ys"])


def test_cached_greedy_generator_matches_uncached_and_repeats_bitwise(golden):
    from csa_amd.model import CachedGreedyGenerator, GreedyGenerator
    z = golden("greedy_tiny")
    m, data, max_len = _tiny_model_and_data(z)
    with torch.no_grad():
        plain = GreedyGenerator(m, max_len)(data())
    gen = CachedGreedyGenerator(m, max_len)
    ys1, lp1 = gen(data(), return_logp=True)
    ys2, lp2 = gen(data(), return_logp=True)
    assert torch.equal(ys1, plain) and ys1.shape == plain.shape
    assert torch.equal(ys1, ys2) and torch.equal(lp1, lp2)
    assert torch.equal(gen(data()), plain)


@pytest.mark.parametrize("repeat_heads", [False, True])
def test_decoder_step_matches_full_pass_at_production_head_dim(repeat_heads, monkeypatch):
    """hd = 64, S = 150 with source pads and PAD target keys: BaseDecoder.step, teacher-forced, against the rows of
    the full pass on the GPU, through the HIP kernel (counted) and never the SDPA fallback."""
    from csa_amd import decode_ops
    from csa_amd.glue import LayerNorm
    from csa_amd.model import PAD, BaseDecoder, DecoderLayer, make_std_mask
    calls = {"hip": 0, "ref": 0}
    hip, ref = decode_ops._decode_attention_hip, decode_ops._decode_attention_ref

    def count(name, fn):
        def wrapped(*a):
            calls[name] += 1
            return fn(*a)
        return wrapped
    monkeypatch.setattr(decode_ops, "_decode_attention_hip", count("hip", hip))
    monkeypatch.setattr(decode_ops, "_decode_attention_ref", count("ref", ref))
    torch.manual_seed(9)
    B, S, T, E, H = 2, 150, 9, 512, 8
    dec = BaseDecoder(DecoderLayer(E, H, 2048, 0.2), 2, norm=LayerNorm(E)).cuda().eval()
    tokens = torch.tensor([[1, 4, 7, 2, 9, 5, 3, 8, 6], [1, 5, 3, PAD, 8, PAD, 4, 2, 7]], device="cuda")
    src_mask = torch.zeros(B, S, dtype=torch.bool, device="cuda")
    src_mask[0, 120:] = True
    src_mask[1, 37:] = True
    memory = torch.randn(B, S, E, device="cuda")
    x = torch.randn(B, T, E, device="cuda")
    with torch.no_grad():
        std = make_std_mask(tokens, PAD)
        tgt_mask = std.repeat(H, 1, 1) if repeat_heads else std.repeat_interleave(H, 0)
        full, _ = dec(x.permute(1, 0, 2), memory.permute(1, 0, 2), tgt_mask, memory_key_padding_mask=src_mask)
        full = full.permute(1, 0, 2).cpu()
        cache = dec.make_cache(memory, src_mask, T, repeat_heads=repeat_heads)
        cache.pad.copy_(tokens == PAD)
        for t in range(T):
            y = dec.step(x[:, t:t + 1], cache, t)
            np.testing.assert_allclose(y[:, 0].cpu().numpy(), full[:, t].numpy(), rtol=1e-4, atol=1e-4, err_msg=f"t={t}")
    assert calls == {"hip": 2 * 2 * T, "ref": 0}
