"""Oracle of sampled decoding (csa_amd.decode_ops.sample_rows, csa_amd.decoding.SamplingGenerator), test infrastructure only.

sample_rows_np restates the rule of include/csa_hip.h (csa_sample_rows) in fp64 on top of oracle/philox.py: the
temperature product alone is formed in fp32, as specified; the sets, the softmax masses, the Gumbel noise and the noisy
scores are fp64. Beside the tokens and log-probabilities it returns how close each decision was, so that a fixture can
be shown to be decisive before anything is compared:

  draw     the best and second-best noisy scores of a row differ by <= DRAW_WINDOW * max(1, |best|): logf to 2 ulp
           twice on |g| <= 16.6 plus the fp32 add is <= 6e-6 per score, 1.2e-5 for two, below 2^-16 = 1.53e-5;
  nucleus  some class boundary has |G - top_p| <= NUCLEUS_WINDOW: worst-case fp32 summation (per-thread chains of
           <= 128 terms at V = 32768, the reduction tree, exp to 2 ulp) is <= 144 * 2^-24 = 8.6e-6. The maximal
           class is no boundary: its G is an exact 0 in every implementation.

Top-k is an exact fp32 comparison and has no window. sampling_ref is the uncached generator: every step re-runs
BaseDecoder.forward over all rows so far (make_std_mask per row, the memory repeated num_samples times)."""
from types import SimpleNamespace

import numpy as np
import torch

from beam_ref import BOS, EOS_ID, PAD, search_case, stub_model  # noqa: F401 (shared fixtures)
from oracle import philox

RNG_SAMPLE = 7
DRAW_WINDOW = 2.0 ** -16
NUCLEUS_WINDOW = 2.0 ** -16
M32 = 0xFFFFFFFF


def gumbel_np(rows, V, t, seed, offset=0):
    """g (rows, V) fp64 = -log(-log u), u = ((w >> 9) + 0.5) 2^-23, w = word j & 3 of Philox4x32-7 with counter
    {j >> 2, r, t, (7 << 28) ^ lo32(offset)} and key (lo32(seed), hi32(seed))."""
    j = np.arange(V).reshape(1, V)
    r = np.arange(rows).reshape(rows, 1)
    words = philox.philox4x32(j >> 2, r, int(t) & M32, ((RNG_SAMPLE << 28) ^ (int(offset) & M32)) & M32,
                              int(seed) & M32, (int(seed) >> 32) & M32)
    sel = np.broadcast_to(j & 3, (rows, V))
    w = np.choose(sel, [np.broadcast_to(x, (rows, V)) for x in words])
    u = ((w >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert u.min() > 0.0 and u.max() < 1.0
    return -np.log(-np.log(u))


def filter_np(z, temperature=1.0, top_k=0, top_p=1.0):
    """Steps 1-3 of the rule, which do not depend on the step or the seed: y (rows, V) fp32, the kept set (rows, V)
    bool, lse (rows,) fp64 over it and nuc_gap (rows,), the smallest |G - top_p| over the class boundaries of each row
    (inf without the top-p rule or without a second class)."""
    z = np.asarray(z, dtype=np.float32)
    rows, V = z.shape
    inv = np.float32(1.0) / np.float32(temperature)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (z * inv).astype(np.float32)
        cand = y > -np.inf  # neither -inf nor NaN
    yc = np.where(cand, y, -np.inf).astype(np.float64)
    order = np.argsort(-yc, axis=1, kind="stable")
    srt = np.take_along_axis(yc, order, axis=1)
    keep = cand.copy()
    if top_k > 0:
        theta = srt[:, min(int(top_k), V) - 1]
        on = cand.sum(1) > top_k
        keep &= ~on[:, None] | (yc >= theta[:, None])
    nuc_gap = np.full(rows, np.inf)
    if top_p < 1.0:
        p32 = np.float64(np.float32(top_p))
        ks = np.take_along_axis(keep, order, axis=1)  # a prefix of each sorted row
        m = srt[:, :1]
        with np.errstate(invalid="ignore"):
            e = np.where(ks, np.exp(srt - np.where(np.isfinite(m), m, 0.0)), 0.0)
        Z = e.sum(1, keepdims=True)
        p = e / np.where(Z > 0, Z, 1.0)
        before = np.cumsum(p, axis=1) - p
        start = np.ones((rows, V), dtype=bool)
        start[:, 1:] = srt[:, 1:] != srt[:, :-1]
        G = np.maximum.accumulate(np.where(start, before, -1.0), axis=1)  # of the class's first entry
        keep_sorted = ks & (G < p32)
        boundary = ks & start
        boundary[:, 0] = False
        nuc_gap = np.where(boundary, np.abs(G - p32), np.inf).min(axis=1)
        k3 = np.zeros_like(keep)
        np.put_along_axis(k3, order, keep_sorted, axis=1)
        keep = k3
    with np.errstate(divide="ignore", invalid="ignore"):
        yk = np.where(keep, yc, -np.inf)
        m = yk.max(axis=1)
        ms = np.where(np.isfinite(m), m, 0.0)
        lse = np.where(np.isfinite(m), ms + np.log(np.exp(yk - ms[:, None]).sum(axis=1)), -np.inf)
    return SimpleNamespace(y=y, keep=keep, lse=lse, nuc_gap=nuc_gap)


def draw_np(f, g, fin=None, eos_id=None, pad_id=PAD):
    """Steps 4-6 on a filter_np result and the noise g: tok (rows,) int64, logp (rows,) fp64, fin (rows,) uint8 after
    the step and draw_gap (rows,), (best - second best noisy score) / max(1, |best|), inf for a row that draws from
    fewer than two entries or is finished."""
    rows, V = f.y.shape
    fin = np.zeros(rows, dtype=np.uint8) if fin is None else np.asarray(fin, dtype=np.uint8)
    score = np.where(f.keep, f.y.astype(np.float64) + g, -np.inf)
    tok = score.argmax(axis=1)  # the first maximal entry
    has = f.keep.any(axis=1)
    tok = np.where(has, tok, 0)
    best = np.take_along_axis(score, tok[:, None], axis=1)[:, 0]
    rest = score.copy()
    np.put_along_axis(rest, tok[:, None], -np.inf, axis=1)
    with np.errstate(invalid="ignore"):
        gap = (best - rest.max(axis=1)) / np.maximum(1.0, np.abs(best))
        logp = np.where(has, np.take_along_axis(f.y.astype(np.float64), tok[:, None], axis=1)[:, 0] - f.lse, -np.inf)
    gap = np.where(has & np.isfinite(rest.max(axis=1)), gap, np.inf)
    done = fin != 0
    tok = np.where(done, pad_id, tok).astype(np.int64)
    logp = np.where(done, 0.0, logp)
    gap = np.where(done, np.inf, gap)
    new_fin = done | ((tok == eos_id) if eos_id is not None else False)
    return SimpleNamespace(tok=tok, logp=logp, fin=new_fin.astype(np.uint8), draw_gap=gap,
                           nuc_gap=np.where(done, np.inf, f.nuc_gap))


def sample_rows_np(z, t, seed, offset=0, temperature=1.0, top_k=0, top_p=1.0, fin=None, eos_id=None, pad_id=PAD):
    """The whole rule for one step: see filter_np and draw_np."""
    z = np.asarray(z, dtype=np.float32)
    return draw_np(filter_np(z, temperature, top_k, top_p), gumbel_np(z.shape[0], z.shape[1], t, seed, offset), fin,
                   eos_id, pad_id)


def undecided(r):
    """(draws, boundaries) of a draw_np result that the windows leave open."""
    return int((r.draw_gap <= DRAW_WINDOW).sum()), int((r.nuc_gap <= NUCLEUS_WINDOW).sum())


def assert_decisive(r, what=""):
    """Fails (never skips) unless no draw and no class boundary of the oracle lies inside its window."""
    d, n = undecided(r)
    assert d == 0 and n == 0, (f"{what}: {d} undecided draws (smallest gap {r.draw_gap.min():.3e}), {n} undecided "
                               f"boundaries (smallest {r.nuc_gap.min():.3e})")


def sampling_ref(model, enc, src_mask, T, num_samples=1, seed=0, temperature=1.0, top_k=0, top_p=1.0, eos_id=EOS_ID):
    """model: anything with tgt_embedding, decoder (BaseDecoder) and generator.linear, in eval mode. Returns a
    namespace: ids and logp (B, T-1), or (B, S, T-1) for num_samples = S > 1, fin (T-1, R) finished flags after each
    step and draw_gap / nuc_gap, the smallest of the run."""
    from csa_amd.model import make_std_mask
    B, S = enc.shape[0], num_samples
    R, dev = B * S, enc.device
    H = model.decoder.layers[0].self_attn.num_heads
    mem = enc.repeat_interleave(S, 0).permute(1, 0, 2)
    mm = None if src_mask is None else src_mask.repeat_interleave(S, 0)
    ys = torch.full((R, 1), BOS, dtype=torch.long, device=dev)
    fin = np.zeros(R, dtype=np.uint8)
    logps, fins, draw_gap, nuc_gap = [], [], np.inf, np.inf
    with torch.no_grad():
        for t in range(T - 1):
            tgt_mask = make_std_mask(ys, PAD).repeat_interleave(H, 0)
            dec, _ = model.decoder(model.tgt_embedding(ys).permute(1, 0, 2), mem, tgt_mask, memory_key_padding_mask=mm)
            z = model.generator.linear(dec.permute(1, 0, 2)[:, -1]).float().cpu().numpy()
            r = sample_rows_np(z, t, seed, 0, temperature, top_k, top_p, fin, eos_id)
            ys = torch.cat([ys, torch.from_numpy(r.tok).to(dev).view(R, 1)], dim=1)
            fin = r.fin
            logps.append(r.logp)
            fins.append(fin.copy())
            draw_gap, nuc_gap = min(draw_gap, r.draw_gap.min()), min(nuc_gap, r.nuc_gap.min())
    shape = (B, T - 1) if S == 1 else (B, S, T - 1)
    return SimpleNamespace(ids=ys[:, 1:].cpu().reshape(shape), logp=np.stack(logps, axis=1).reshape(shape),
                           fin=np.stack(fins), draw_gap=np.array([draw_gap]), nuc_gap=np.array([nuc_gap]))


# ---- the launch classes and filters of the kernel test (tests/test_sample_gpu.py), decisive by assert_decisive ----

FILTERS = {"none": dict(), "k5": dict(top_k=5), "p0.7": dict(top_p=0.7), "k40_p0.9": dict(top_k=40, top_p=0.9)}
KERNEL_T = 8            # columns of the token buffer in the kernel tests: steps 0, 3 and T - 2 = 6
KERNEL_STEPS = (0, 3, KERNEL_T - 2)
KERNEL_ROWS = (1, 3, 70)
KERNEL_SEED = 0x5EED0000C0DE  # both key words in use; chosen on this oracle alone (see kernel_logits)


KERNEL_VS = (1, 19, 255, 256, 257, 1024, 1028, 4099, 32768)
LOGIT_SEEDS = {1: 0, 19: 0, 255: 0, 256: 0, 257: 1, 1024: 0, 1028: 0, 4099: 0, 32768: 0}


def kernel_logits(V, rows=max(KERNEL_ROWS), data_seed=None):
    """(rows, V) fp32 logits of a launch class: normal(0, 6) with a few -inf entries and, from V = 19 up, a duplicated
    maximum in row 0 and a duplicated 5th-largest value in row 1 (ties at the top-k threshold and a tie class at the
    nucleus boundary candidates). data_seed defaults to the class's entry of LOGIT_SEEDS, the first seed for which the
    oracle is decisive on every filter and step of the kernel test."""
    g = np.random.default_rng(1000 * (LOGIT_SEEDS[V] if data_seed is None else data_seed) + V)
    z = (6.0 * g.standard_normal((rows, V))).astype(np.float32)
    if V >= 19:
        z[:, 7] = -np.inf
        z[2, ::3] = -np.inf
        z[0, [3, 11]] = z[0].max()
        fifth = np.sort(z[1])[-5]
        z[1, [4, 13]] = fifth
    return z


# ---- shared by tests/test_sample_cpu.py and tests/test_sample_gpu.py ----

# (num_samples, parameters, seed) of the generator runs on search_case(), B = 3, S = 7, T = 8. The seeds were chosen on
# the oracle alone: among 1..39, the run with the widest smallest gap (0.108, 0.0123, 0.0359, 0.0079) of those in which
# a row finishes before the last step and (num_samples = 3) two samples of one AST differ
FILTERED = dict(temperature=0.8, top_k=6, top_p=0.9)
GENERATOR_CASES = [(1, {}, 21), (1, FILTERED, 6), (3, {}, 39), (3, FILTERED, 16)]
GENERATOR_IDS = ["s1", "s1_filtered", "s3", "s3_filtered"]

RTOL, ATOL = 1e-4, 1e-5  # the suite's tolerance, for the log-probabilities


def run_op(z, t, seed, fin=None, device="cpu", logp=True, T=None, shift=False, **kw):
    """sample_rows on fresh poisoned buffers -> (tokens, pad column, logp column, fin) as numpy, plus the buffers."""
    from csa_amd.decode_ops import sample_rows
    rows, V = z.shape
    T = KERNEL_T if T is None else T
    zt = torch.from_numpy(np.ascontiguousarray(z)).to(device)
    if shift:  # the same rows, their base moved by one float off the 16-byte boundary
        buf = torch.empty(rows * V + 1, dtype=torch.float32, device=device)
        buf[1:] = zt.flatten()
        zt = buf[1:].view(rows, V)
    ys = torch.full((rows, T), 99, dtype=torch.long, device=device)
    pad = torch.full((rows, T), 7, dtype=torch.uint8, device=device)
    f = torch.from_numpy(np.zeros(rows, dtype=np.uint8) if fin is None else np.array(fin, dtype=np.uint8)).to(device)
    lp = torch.full((rows, T - 1), 5.0, device=device) if logp else None
    s = seed - (1 << 64) if seed >= 1 << 63 else seed
    sample_rows(zt, ys, pad, f, torch.tensor([t], dtype=torch.int32, device=device),
                torch.tensor([s, 0], dtype=torch.int64, device=device), logp=lp, **kw)
    col = min(max(t + 1, 0), T - 1)
    return SimpleNamespace(tok=ys[:, col].cpu().numpy(), pad=pad[:, col].cpu().numpy(),
                           logp=None if lp is None else lp[:, min(max(t, 0), T - 2)].cpu().numpy(), fin=f.cpu().numpy(),
                           ys=ys.cpu(), pads=pad.cpu(), logps=None if lp is None else lp.cpu())


def assert_matches(got, want, what):
    np.testing.assert_array_equal(got.tok, want.tok, err_msg=what)
    np.testing.assert_array_equal(got.pad, (want.tok == PAD).astype(np.uint8), err_msg=what)
    np.testing.assert_array_equal(got.fin, want.fin, err_msg=what)
    np.testing.assert_allclose(got.logp, want.logp, rtol=RTOL, atol=ATOL, err_msg=what)


def hand_rows():
    """V = 12. Row 0: distinct values. Row 1: three entries tied at the second-largest value. Row 2: -inf entries and a
    NaN. Row 3: all -inf. Row 4: probabilities .4, .2, .2, .1, .1 (two tie classes). Row 5: two candidates only."""
    V, ninf = 12, -np.inf
    z = np.full((6, V), ninf, dtype=np.float32)
    z[0] = np.array([0.3, -1.2, 2.5, 0.9, -0.4, 1.7, -2.2, 0.1, 1.1, -0.8, 2.1, 0.6], dtype=np.float32)
    z[1] = np.array([0.2, 1.5, -0.7, 2.0, 1.5, 0.4, -1.0, 1.5, 0.0, -0.3, 0.9, -2.0], dtype=np.float32)
    z[2] = np.array([ninf, 0.5, ninf, 1.25, np.nan, -0.75, ninf, 2.0, ninf, 0.25, ninf, ninf], dtype=np.float32)
    z[4, [1, 4, 6, 9, 10]] = np.log(np.array([4.0, 2.0, 2.0, 1.0, 1.0])).astype(np.float32)
    z[5, [3, 8]] = [0.5, -0.5]
    return z
