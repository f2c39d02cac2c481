"""The fp64 oracle, the case builders and the error bounds of the full-sequence decoder attention
(csa_amd/seq_attn_ops.py, csrc/csa_seqattn.hip), shared by tests/test_seq_attn_cpu.py and tests/test_seq_attn_gpu.py.

oracle(): out[r, i, h*hd:(h+1)*hd] = sum_j softmax_j(scale * q[r,h,i] . K[r // G,h,j] + m(r,h,i,j)) * V[r // G,h,j] in
float64, the mask built entry by entry in plain loops over (r, h, j): key j is masked for query i when causal and j > i,
or when the key mask holds a non-zero byte at column j of row r // G ("own") or row (r * H + h) % R ("reference").
Its gradients come from fp64 autograd.

The error metric is max|x - x64| / max|x64| per tensor (out, dq, dk, dv). The bound of a case is FOUR TIMES the error
of the parent's path on the same inputs: F.scaled_dot_product_attention in fp32 on the CPU with the explicit -inf mask
and expanded K/V, and its autograd (baseline()). The factor covers a summation order that legitimately differs (4-wide
MFMA k-steps, tile-wise online-softmax rescaling, P recomputed from lse in the backward). BASELINE below holds those
errors as measured on the CPU by `python tests/seq_attn_ref.py`, which prints the table; the bounds follow from it and
were not adjusted to any kernel result.

A tensor whose fp64 reference is identically zero has no relative error. That happens for dq and dk with ONE visible key
(S = 1, or T = S = 1 causal): the softmax is 1 whatever q and k are, and ds = p * (dp - D) cancels exactly in real
arithmetic, dp = dO . V and D = dO . O being the same hd-term sum. In fp32 the two are rounded in different orders, each
within hd * eps * sum_d|dO_d V_d| of the true value, so |ds| <= 2 * hd * eps * max sum_d|dO_d V_d| (the maximum over
every query and key), and a dq / dk element is scale times at most T such terms times a q or k element. zero_bound() is that figure, the absolute bound of such a
tensor; BASELINE holds None for it."""
import torch
import torch.nn.functional as F

FACTOR = 4.0
EPS32 = 2.0 ** -24


def case(name, R, H, hd, T, S, G=1, causal=False, mode="own", mask=None, packed=False, seed=0):
    return dict(name=name, R=R, H=H, hd=hd, T=T, S=S, G=G, causal=causal, mode=mode, mask=mask, packed=packed, seed=seed)


def _edge_cases():
    """Cross-attention, T and S at 1 and around the 16-wide query and key tiles of the kernel, and 50 / 150 once."""
    out = []
    for hd, H in ((8, 8), (64, 2)):
        for T, S in ((1, 17), (17, 1), (15, 16), (16, 15), (16, 16), (17, 33), (33, 17)):
            out.append(case(f"cross_hd{hd}_T{T}_S{S}", 2, H, hd, T, S, seed=len(out)))
        out.append(case(f"cross_hd{hd}_T50_S150", 2, H, hd, 50, 150, mask="memory", seed=len(out)))
    return out


def _causal_cases():
    """Causal self-attention in both mask modes, a PAD column before a row's end, R = 6 against H = 8 (R not a multiple
    of H: the reference mode's (r * H + h) % R walks every row)."""
    out = []
    for hd in (8, 64):
        for mode in ("own", "reference"):
            for T in ((1, 15, 16, 17, 33) if mode == "own" else (17,)):
                out.append(case(f"causal_{mode}_hd{hd}_T{T}", 6, 8, hd, T, T, causal=True, mode=mode, mask="pad",
                                seed=100 + len(out)))
    return out


def _group_cases():
    """Cross-attention with a group, B = 2, a memory mask that covers the whole key tile 16..31 and leaves a ragged tail."""
    out = []
    for hd, H in ((8, 8), (64, 2)):
        for G in (1, 2, 3):
            out.append(case(f"group_hd{hd}_G{G}", 2 * G, H, hd, 17, 40, G=G, mask="memory", seed=200 + len(out)))
    return out


def _packed_cases():
    """q / k / v as views of packed (B, T, 3, H, hd) and (B, S, 2, H, hd) buffers."""
    out = []
    for hd, H in ((8, 8), (64, 2)):
        out.append(case(f"packed_self_hd{hd}", 3, H, hd, 17, 17, causal=True, mask="pad", packed=True, seed=300 + len(out)))
        out.append(case(f"packed_cross_hd{hd}", 4, H, hd, 17, 33, G=2, mask="memory", packed=True, seed=300 + len(out)))
    return out


CASES = {c["name"]: c for c in _edge_cases() + _causal_cases() + _group_cases() + _packed_cases()}
CPU_CASES = ("causal_own_hd8_T17", "causal_reference_hd8_T17", "group_hd8_G1", "group_hd8_G2", "group_hd8_G3")


def build(c):
    """-> (q (R,H,T,hd), k, v (R/G,H,S,hd), key_mask uint8 or None, dout (R,T,H*hd)), fp32 on the CPU, N(0, 1). With
    c["packed"], q / k / v are the strided views of one packed projection buffer."""
    g = torch.Generator().manual_seed(7919 * c["seed"] + 13)
    R, H, hd, T, S, G = (c[n] for n in ("R", "H", "hd", "T", "S", "G"))
    B = R // G
    if c["packed"] and c["causal"]:
        buf = torch.randn(R, T, 3, H, hd, generator=g)
        q, k, v = (buf[:, :, i].transpose(1, 2) for i in range(3))
    elif c["packed"]:
        q = torch.randn(R, T, H, hd, generator=g).transpose(1, 2)
        buf = torch.randn(B, S, 2, H, hd, generator=g)
        k, v = (buf[:, :, i].transpose(1, 2) for i in range(2))
    else:
        q, k, v = torch.randn(R, H, T, hd, generator=g), torch.randn(B, H, S, hd, generator=g), torch.randn(B, H, S, hd, generator=g)
    mask = None
    if c["mask"] == "pad":  # (R, T): trailing PAD of ragged length, and one PAD column before the end; never column 0
        mask = torch.zeros(R, T, dtype=torch.uint8)
        for r in range(R):
            n = T - (r * 5) % max(T // 2, 1)
            mask[r, n:] = 1
            if n > 3:
                mask[r, 1 + (r + 1) % (n - 2)] = 1
    elif c["mask"] == "memory":  # (B, S): b = 0 loses the whole key tile 16..31 and a tail, the others a ragged tail
        mask = torch.zeros(B, S, dtype=torch.uint8)
        for b in range(B):
            mask[b, S - 3 - 2 * b:] = 1
        if S > 32:
            mask[0, 16:32] = 1
    dout = torch.randn(R, T, H * hd, generator=g)
    return q, k, v, mask, dout


def mask_entries(c, mask, wrong=None):
    """(R, H, T, S) bool, True = masked, written out entry by entry. wrong: a deliberately wrong rule for the decisiveness
    checks ("no_causal", "other_mode")."""
    R, H, T, S, G = (c[n] for n in ("R", "H", "T", "S", "G"))
    mode = c["mode"]
    if wrong == "other_mode":
        mode = "reference" if mode == "own" else "own"
    dead = torch.zeros(R, H, T, S, dtype=torch.bool)
    for r in range(R):
        for h in range(H):
            row = r // G if mode == "own" else (r * H + h) % R
            for j in range(S):
                if mask is not None and row < mask.shape[0] and bool(mask[row, j] != 0):
                    dead[r, h, :, j] = True
                if c["causal"] and wrong != "no_causal":
                    dead[r, h, :j, j] = True
    return dead


def oracle(c, q, k, v, mask, dout, wrong=None):
    """fp64 -> (out, dq, dk, dv). wrong: None, or one of "group_mod" (K/V row r % G instead of r // G; for B == G), "no_causal",
    "other_mode", "one_member" (dk / dv of the group's first row alone instead of the sum)."""
    R, H, T, hd, G = (c[n] for n in ("R", "H", "T", "hd", "G"))
    q64, k64, v64 = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    rows = torch.arange(R) % G if wrong == "group_mod" else torch.arange(R) // G
    ke, ve = k64[rows], v64[rows]
    s = (q64 @ ke.transpose(-1, -2)) * float(hd) ** -0.5
    s = s.masked_fill(mask_entries(c, mask, wrong), float("-inf"))
    out = (torch.softmax(s, -1) @ ve).transpose(1, 2).reshape(R, T, H * hd)
    g = dout.double()
    if wrong == "one_member":
        dq, = torch.autograd.grad(out, q64, g, retain_graph=True)
        first = torch.zeros(R, 1, 1)
        first[::G] = 1.0
        dk, dv = torch.autograd.grad(out, (k64, v64), g * first)
    else:
        dq, dk, dv = torch.autograd.grad(out, (q64, k64, v64), g)
    return out.detach(), dq, dk, dv


def sdpa_parent(c, q, k, v, mask, dout):
    """The parent's path in fp32 on the tensors' device: SDPA with the explicit -inf mask and expanded K/V, its
    autograd summing dk / dv over the group."""
    R, H, T, hd, S, G = (c[n] for n in ("R", "H", "T", "hd", "S", "G"))
    q32, k32, v32 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    dead = mask_entries(c, mask).to(q.device)
    m = torch.zeros(dead.shape, dtype=torch.float32, device=q.device).masked_fill_(dead, float("-inf"))
    out = F.scaled_dot_product_attention(q32, k32.repeat_interleave(G, 0), v32.repeat_interleave(G, 0), m)
    out = out.transpose(1, 2).reshape(R, T, H * hd)
    dq, dk, dv = torch.autograd.grad(out, (q32, k32, v32), dout)
    return out.detach(), dq, dk, dv


def rel_err(x, x64):
    """max|x - x64| / max|x64|, or None where the reference is identically zero. NaN anywhere gives inf."""
    x = x.detach().double().cpu()
    d = (x - x64).abs().max().item()
    den = x64.abs().max().item()
    if d != d:
        return float("inf")
    return None if den == 0.0 else d / den


def zero_bound(c, q, k, v, dout):
    """The absolute bound of a dq / dk whose reference is identically zero (module docstring)."""
    R, H, hd, T, G = (c[n] for n in ("R", "H", "hd", "T", "G"))
    g = dout.view(R, T, H, hd).transpose(1, 2).abs().double()
    ds = 2 * hd * EPS32 * (g @ v.repeat_interleave(G, 0).abs().double().transpose(-1, -2)).max().item()
    return FACTOR * float(hd) ** -0.5 * T * ds * max(q.abs().max().item(), k.abs().max().item())


def check(c, got, inputs, ref=None, what=""):
    """Asserts the four tensors of `got` within the case's bounds of the fp64 oracle; prints each figure first.
    -> the errors."""
    q, k, v, mask, dout = inputs
    ref = oracle(c, q, k, v, mask, dout) if ref is None else ref
    errs = []
    for name, x, x64, base in zip(("out", "dq", "dk", "dv"), got, ref, BASELINE[c["name"]]):
        e = rel_err(x, x64)
        if e is None:
            e = (x.detach().double().cpu() - x64).abs().max().item()
            bound = zero_bound(c, q, k, v, dout)
            assert base is None, (c["name"], name)
        else:
            bound = FACTOR * base
        print(f"{what}{c['name']:28s} {name:3s} err {e:.3e} bound {bound:.3e}")
        errs.append((name, e, bound))
    for name, e, bound in errs:
        assert e <= bound, f"{what}{c['name']} {name}: {e:.3e} > {bound:.3e}"
    return errs


def fully_masked_case():
    """causal_own_hd64_T17 with column 0 of row 2 PAD as well: query 0 of row 2 sees no key in any head (the fp64
    softmax of its all -inf row is NaN too), every other query of the batch still sees one. -> (case, inputs)"""
    c = dict(CASES["causal_own_hd64_T17"], name="fully_masked_row")
    q, k, v, mask, dout = build(c)
    mask = mask.clone()
    mask[2, 0] = 1
    return c, (q, k, v, mask, dout)


def finite_err(x, x64, same_nan=True):
    """rel_err over the entries where the reference is finite; same_nan: x must be NaN exactly where it is not."""
    x = x.detach().double().cpu()
    nan = torch.isnan(x64)
    assert not same_nan or torch.equal(torch.isnan(x), nan), "NaN pattern differs"
    return ((x - x64)[~nan].abs().max() / x64[~nan].abs().max()).item()


# forward error of the parent's path on fully_masked_case(), finite entries (measured as BASELINE is)
BASELINE_FULLY_MASKED_OUT = 2.167e-07


def measure_baseline(c):
    inputs = build(c)
    ref = oracle(c, *inputs)
    return tuple(rel_err(x, x64) for x, x64 in zip(sdpa_parent(c, *inputs), ref))


# max|x - x64| / max|x64| of F.scaled_dot_product_attention in fp32 on the CPU and its autograd: (out, dq, dk, dv) per
# case; None: the reference is identically zero (zero_bound). The bound of a case is FACTOR times its row.
BASELINE = {
    "cross_hd8_T1_S17": (1.941e-07, 1.772e-07, 7.696e-08, 1.890e-07),
    "cross_hd8_T17_S1": (0.000e+00, None, None, 1.611e-07),
    "cross_hd8_T15_S16": (1.528e-07, 3.084e-07, 4.066e-07, 4.656e-07),
    "cross_hd8_T16_S15": (3.592e-07, 2.595e-07, 1.629e-07, 1.543e-07),
    "cross_hd8_T16_S16": (1.471e-07, 3.284e-07, 1.515e-07, 2.438e-07),
    "cross_hd8_T17_S33": (1.630e-07, 4.482e-07, 3.571e-07, 2.592e-07),
    "cross_hd8_T33_S17": (2.430e-07, 1.982e-07, 2.776e-07, 2.681e-07),
    "cross_hd8_T50_S150": (2.926e-07, 5.945e-07, 6.952e-07, 4.581e-07),
    "cross_hd64_T1_S17": (1.448e-07, 1.900e-07, 2.163e-07, 1.296e-07),
    "cross_hd64_T17_S1": (0.000e+00, None, None, 8.132e-08),
    "cross_hd64_T15_S16": (4.037e-07, 3.525e-07, 2.801e-07, 3.968e-07),
    "cross_hd64_T16_S15": (3.057e-07, 5.202e-07, 3.838e-07, 2.677e-07),
    "cross_hd64_T16_S16": (1.973e-07, 3.208e-07, 4.426e-07, 2.177e-07),
    "cross_hd64_T17_S33": (4.689e-07, 4.377e-07, 2.861e-07, 3.472e-07),
    "cross_hd64_T33_S17": (2.438e-07, 2.305e-07, 3.007e-07, 3.097e-07),
    "cross_hd64_T50_S150": (4.288e-07, 6.760e-07, 7.150e-07, 6.102e-07),
    "causal_own_hd8_T1": (0.000e+00, None, None, 0.000e+00),
    "causal_own_hd8_T15": (1.392e-07, 2.363e-07, 3.970e-07, 1.394e-07),
    "causal_own_hd8_T16": (1.301e-07, 4.091e-07, 2.111e-07, 1.370e-07),
    "causal_own_hd8_T17": (1.563e-07, 3.074e-07, 2.993e-07, 1.169e-07),
    "causal_own_hd8_T33": (1.589e-07, 3.107e-07, 2.014e-07, 2.891e-07),
    "causal_reference_hd8_T17": (1.045e-07, 2.136e-07, 2.992e-07, 1.265e-07),
    "causal_own_hd64_T1": (0.000e+00, None, None, 0.000e+00),
    "causal_own_hd64_T15": (3.605e-07, 3.405e-07, 4.442e-07, 3.496e-07),
    "causal_own_hd64_T16": (2.541e-07, 3.492e-07, 3.977e-07, 2.739e-07),
    "causal_own_hd64_T17": (2.167e-07, 3.783e-07, 3.715e-07, 2.052e-07),
    "causal_own_hd64_T33": (2.710e-07, 4.494e-07, 4.501e-07, 2.600e-07),
    "causal_reference_hd64_T17": (2.011e-07, 4.729e-07, 4.397e-07, 2.060e-07),
    "group_hd8_G1": (2.198e-07, 8.633e-07, 5.597e-07, 3.940e-07),
    "group_hd8_G2": (2.127e-07, 3.237e-07, 2.921e-07, 5.012e-07),
    "group_hd8_G3": (2.774e-07, 4.152e-07, 3.518e-07, 4.247e-07),
    "group_hd64_G1": (6.377e-07, 3.708e-07, 4.513e-07, 4.316e-07),
    "group_hd64_G2": (4.046e-07, 4.080e-07, 5.417e-07, 2.420e-07),
    "group_hd64_G3": (3.098e-07, 6.107e-07, 3.629e-07, 2.264e-07),
    "packed_self_hd8": (1.060e-07, 2.066e-07, 2.589e-07, 1.343e-07),
    "packed_cross_hd8": (2.502e-07, 1.032e-06, 4.536e-07, 2.952e-07),
    "packed_self_hd64": (1.235e-07, 4.884e-07, 5.462e-07, 1.700e-07),
    "packed_cross_hd64": (4.917e-07, 5.454e-07, 5.951e-07, 4.400e-07),
}


if __name__ == "__main__":
    torch.manual_seed(0)
    for name, c in CASES.items():
        row = ", ".join("None" if e is None else f"{e:.3e}" for e in measure_baseline(c))
        print(f'    "{name}": ({row}),')
    c, inputs = fully_masked_case()
    print("BASELINE_FULLY_MASKED_OUT =", f"{finite_err(sdpa_parent(c, *inputs)[0], oracle(c, *inputs)[0], same_nan=False):.3e}")
