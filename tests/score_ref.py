"""Oracles of the scoring feature (csa_amd/score_ops.py, csa_amd/scoring.py), fp64 on the CPU.

token_logp_ref / token_logp_grad_ref: log_softmax + gather with the ignore rules, and the analytic gradient
g * (onehot - softmax). score_loop_ref: the teacher-forced score of candidates, position by position: for every prefix
length the decoder runs in fp64 over [BOS, the candidate's first tokens] with a key mask written out entry by entry,
and the last position's log_softmax is read at the candidate's next token. Also the inputs the CPU and GPU tests share."""
import copy

import numpy as np
import torch

PAD, BOS, EOS_ID = 0, 2, 3
RTOL, ATOL = 1e-4, 1e-5  # the project's fp32 rule against fp64 (tests/test_row_kernels_gpu.py)

# the decoder side of the tiny model (tests/test_model_gpu.py TINY): hidden 64, 8 heads, 60 target words, ffn 128
TINY = dict(src_vocab_size=50, tgt_vocab_size=60, hidden_size=64, num_heads=8, num_layers=1, sbm_layers=2,
            use_pegen="pegen", dim_feed_forward=128, dropout=0.2, pe_dim=32, pegen_dim=128, sbm_enc_dim=512,
            clusters=[10, 12], full_att=False)


def scored_rows(target, V, ignore_id):
    return (target != ignore_id) & (target >= 0) & (target < V)


def token_logp_ref(logits, target, ignore_id=PAD):
    """logits (rows, V) any float dtype, target (rows) int64 -> (rows) fp64; 0 in ignored rows."""
    z = logits.detach().double().cpu()
    t = target.cpu()
    ok = scored_rows(t, z.shape[1], ignore_id)
    lp = torch.log_softmax(z, -1).gather(1, torch.where(ok, t, torch.zeros_like(t))[:, None])[:, 0]
    return torch.where(ok, lp, torch.zeros_like(lp))


def token_logp_grad_ref(logits, target, g, ignore_id=PAD):
    """d (sum_r g_r logp_r) / d logits in fp64: g_r (onehot(t_r) - softmax(z_r)); zeros in ignored rows whatever g_r."""
    z = logits.detach().double().cpu()
    t = target.cpu()
    ok = scored_rows(t, z.shape[1], ignore_id)
    onehot = torch.zeros_like(z)
    onehot[ok, t[ok]] = 1.0
    dz = g.detach().double().cpu()[:, None] * (onehot - torch.exp(torch.log_softmax(z, -1)))
    dz[~ok] = 0.0
    return dz


def assert_same_kind_and_close(got, want, what, rtol=RTOL, atol=ATOL):
    """Non-finite entries must match in kind (NaN, +inf, -inf at the same places); the finite ones compare."""
    got = np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    want = np.asarray(want.detach().cpu() if isinstance(want, torch.Tensor) else want, dtype=np.float64)
    assert got.shape == want.shape, what
    for kind, f in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        assert np.array_equal(f(got), f(want)), f"{what}: {kind} pattern differs"
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=rtol, atol=atol, err_msg=what)


def outside(a, b, rtol=RTOL, atol=ATOL):
    """True when a leaves the tolerance around b somewhere: what a decisive fixture shows of a wrong answer."""
    a, b = (np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64) for x in (a, b))
    return not np.allclose(a, b, rtol=rtol, atol=atol)


# ---- kernel inputs ----

KINDS = ("plain", "shift_pos", "shift_neg", "neg_inf_cols", "ignored", "neg_inf_target", "out_of_range", "nan_row",
         "all_neg_inf")


def kernel_ignore_id(V):
    """PAD, except for one-column rows, whose only target is column 0."""
    return PAD if V > 1 else -1


def kernel_case(rows, V, kinds=None, seed=0):
    """(logits (rows, V) fp32, target (rows) int64, g (rows) fp32) for ignore_id = kernel_ignore_id(V): row i is of kind
    kinds[i % len(kinds)]. plain: randn * 3; shift_pos / shift_neg: that plus / minus 1e4 (a missing max subtraction
    overflows or underflows); neg_inf_cols: -inf at a third of the columns, never the target; neg_inf_target: -inf at
    the target; ignored: target ignore_id and g NaN; out_of_range: target V or -3 and g NaN; nan_row: a NaN at a
    non-target column (plain when V = 1); all_neg_inf."""
    kinds = KINDS if kinds is None else kinds
    gen = torch.Generator().manual_seed(1000003 * seed + 1009 * rows + V)
    z = torch.randn(rows, V, generator=gen) * 3.0
    t = torch.randint(1, V, (rows,), generator=gen) if V > 1 else torch.zeros(rows, dtype=torch.int64)
    g = torch.randn(rows, generator=gen)
    for i in range(rows):
        k = kinds[i % len(kinds)]
        if k == "shift_pos":
            z[i] += 1e4
        elif k == "shift_neg":
            z[i] -= 1e4
        elif k == "neg_inf_cols":
            z[i, torch.arange(V) % 3 == (int(t[i]) + 1) % 3] = float("-inf")
        elif k == "neg_inf_target":
            z[i, t[i]] = float("-inf")
        elif k == "ignored":
            t[i], g[i] = kernel_ignore_id(V), float("nan")
        elif k == "out_of_range":
            t[i], g[i] = (V if i % 2 == 0 else -3), float("nan")
        elif k == "nan_row" and V > 1:
            z[i, (int(t[i]) + 1) % V] = float("nan")
        elif k == "all_neg_inf":
            z[i] = float("-inf")
    return z, t, g


# ---- the scorer ----

def decoder_stub(seed=5, gen_scale=4.0, E=64, H=8, V=60, ffn=128, layers=4):
    """Target embedding + decoder + generator of the tiny CSATrans, without the encoder (which has no CPU path)."""
    from csa_amd.glue import LayerNorm
    from csa_amd.model import BaseDecoder, DecoderLayer, Embeddings, Generator
    torch.manual_seed(seed)

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.tgt_embedding = Embeddings(E, V, 0.2, with_pos=True)
            self.decoder = BaseDecoder(DecoderLayer(E, H, ffn, 0.2, "gelu"), layers, norm=LayerNorm(E))
            self.generator = Generator(V, E, 0.2)
    m = Stub().eval()
    with torch.no_grad():
        m.generator.linear.weight.mul_(gen_scale)
    return m


def scorer_case(B=3, G=2, T=7, S=9, E=64, V=60, seed=11):
    """enc (B, S, E), src_mask (B, S) and candidates (B, G, T) with ragged EOS positions, PAD after them except in one
    row that carries non-PAD ids after its EOS (they must not be scored), and a PAD emitted before the EOS in another
    (it is scored, and masks a key). Row 0's EOS comes first, at position 1, so its decoder input holds PAD from column 3
    on: in the reference head mask those columns fall on the heads of the other rows, which still score positions
    beyond them, so the two head-mask modes differ on this batch."""
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(B, S, E, generator=g)
    src_mask = torch.zeros(B, S, dtype=torch.bool)
    src_mask[1, S - 3:] = True
    cand = torch.randint(4, V, (B * G, T), generator=g)
    eos_at = [1, T - 1, 3, None, 4, 2]
    for r in range(B * G):
        e = eos_at[r % len(eos_at)]
        if e is not None:
            cand[r, e] = EOS_ID
            cand[r, e + 1:] = PAD
    cand[4, 5:] = torch.tensor([17, 23][:T - 5])  # ids after row 4's EOS at position 4
    cand[1, 2] = PAD                               # a PAD before row 1's EOS
    return enc, src_mask, cand.view(B, G, T)


def scored_positions(cand, eos_id):
    """(R, T) bool, token by token: with an eos_id everything up to and including its first occurrence, without one
    every non-PAD token."""
    R, T = cand.shape
    out = torch.zeros(R, T, dtype=torch.bool)
    for r in range(R):
        for t in range(T):
            if eos_id is None:
                out[r, t] = cand[r, t] != PAD
            else:
                out[r, t] = True
                if cand[r, t] == eos_id:
                    break
    return out


def score_loop_ref(model, enc, src_mask, cand, eos_id, head_mask, dec_in=None, scored=None):
    """cand (B, G, T) or (B, T) ids -> namespace-free tuple (tokens (R, T) fp64, logp (R) fp64, length (R) int) with
    R = B * G rows in candidate order. The decoder side of `model` is copied to the CPU in fp64 and run once per
    position t over the prefix [BOS, cand[:t]] (or dec_in[:, :t + 1] when given, as validation does). The key mask of
    query i, key j of row r, head h is: j > i, or the token at column j of row r ("own") / of row (r * H + h) % R
    ("reference") is PAD."""
    cand3 = cand if cand.dim() == 3 else cand[:, None]
    B, G, T = cand3.shape
    R = B * G
    c = cand3.reshape(R, T).cpu()
    m = copy.deepcopy(model).cpu().double().eval()
    H = m.decoder.layers[0].self_attn.num_heads
    mem = enc.detach().cpu().double().repeat_interleave(G, 0).permute(1, 0, 2)
    mm = None if src_mask is None else src_mask.cpu().repeat_interleave(G, 0)
    if dec_in is None:
        dec_in = torch.full((R, T), PAD, dtype=torch.int64)
        for r in range(R):
            dec_in[r, 0] = BOS
            for t in range(1, T):
                dec_in[r, t] = c[r, t - 1]
    else:
        dec_in = dec_in.cpu()
    scored = scored_positions(c, eos_id) if scored is None else scored.cpu()
    tokens = torch.zeros(R, T, dtype=torch.float64)
    with torch.no_grad():
        for t in range(T):
            n = t + 1
            mask = torch.zeros(R * H, n, n, dtype=torch.bool)
            for r in range(R):
                for h in range(H):
                    src = r if head_mask == "own" else (r * H + h) % R
                    for j in range(n):
                        mask[r * H + h, :, j] = bool(dec_in[src, j] == PAD)
                        mask[r * H + h, :j, j] = True
            dec, _ = m.decoder(m.tgt_embedding(dec_in[:, :n]).permute(1, 0, 2), mem, tgt_mask=mask,
                               memory_key_padding_mask=mm)
            lp = torch.log_softmax(m.generator.linear(dec.permute(1, 0, 2)[:, -1]), -1)
            for r in range(R):
                if scored[r, t]:
                    tokens[r, t] = lp[r, c[r, t]]
    return tokens, tokens.sum(-1), scored.sum(-1)
