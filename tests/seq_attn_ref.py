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
tensor; BASELINE holds None for it. The same holds with one visible key among many masked ones (mask "last_only").

Wide logits (qscale: scale * s with a standard deviation of 8). The backward recomputes p = exp(scale * s - lse) from ONE
fp32 lse, where the parent keeps the probabilities of its forward: lse is rounded to within EPS32 * |lse|, so every p of
a row carries a common relative error of up to EPS32 * |lse| that the parent's does not. A gradient element is a sum of
terms each proportional to one p (dq = scale * sum_j ds_ij k_j, dk = scale * sum_i ds_ij q_i, dv = sum_i p_ij dO_i, with
ds = p * (dp - D)), so its error from this source is at most EPS32 * max|lse| times the sum of the terms' absolute
values. lse_bound() evaluates that in fp64, relative to max|x64| as the metric is. check() prints it beside every wide
case's gradient errors. It is NOT part of the bound: at these logits the parent's own error grows as much (its gradient
rows are 5e-7 to 4e-6) and the kernels stay within FACTOR times it, so the rule above holds unchanged; the term is kept
as the yardstick should a wider case need it.

The rows of BASELINE after "packed_cross_hd64" (long_, group4_ / group2_, heads, mask_, wide_, layout_) were added with
their cases, from the same script's output on the CPU."""
import torch
import torch.nn.functional as F

FACTOR = 4.0
EPS32 = 2.0 ** -24


def case(name, R, H, hd, T, S, G=1, causal=False, mode="own", mask=None, packed=False, seed=0, qscale=None,
         key_order=None, dout=None):
    """qscale: q is multiplied by it (wide logits). key_order: "ascending" / "descending" sorts the keys (and values) of
    each (b, h) by their score against query 0 of row b * G. dout: "row" = one (H*hd) row expanded over (R, T)."""
    return dict(name=name, R=R, H=H, hd=hd, T=T, S=S, G=G, causal=causal, mode=mode, mask=mask, packed=packed, seed=seed,
                qscale=qscale, key_order=key_order, dout=dout)


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


def _long_cases():
    """Many tiles: T at and below the supported maximum of 256 (16 query and key tiles, the causal trip counts over all
    of them), S beyond 256 (19 key tiles), T = S = 241 (ragged last tile on both sides)."""
    out = []
    for hd in (8, 64):
        for T in (255, 256):
            out.append(case(f"long_causal_hd{hd}_T{T}", 2, 2, hd, T, T, causal=True, mask="pad", seed=400 + len(out)))
        out.append(case(f"long_cross_hd{hd}_T256_S17", 2, 2, hd, 256, 17, seed=400 + len(out)))
        out.append(case(f"long_cross_hd{hd}_T17_S300", 2, 2, hd, 17, 300, mask="memory", seed=400 + len(out)))
    out.append(case("long_causal_reference_hd64_T256", 3, 2, 64, 256, 256, causal=True, mode="reference", mask="pad",
                    seed=400 + len(out)))
    out.append(case("long_cross_hd64_T241_S241", 2, 2, 64, 241, 241, seed=400 + len(out)))
    return out


def _group4_cases():
    """The production group G = 4 with a third AST (B = 3, kb = 2), three query tiles; in mode "reference" the mask is
    (R, S) with rows that all differ, so every member of a group reads another row inside the key side's group loop
    (G = 2: H = 2, the row depends on the head; G = 4: H = 1, to keep R * H small)."""
    out = []
    for hd in (8, 64):
        out.append(case(f"group4_own_hd{hd}", 12, 1, hd, 33, 40, G=4, mask="memory", seed=500 + len(out)))
        out.append(case(f"group4_reference_hd{hd}", 12, 1, hd, 33, 40, G=4, mode="reference", mask="memory",
                        seed=500 + len(out)))
        out.append(case(f"group2_reference_hd{hd}", 6, 2, hd, 33, 40, G=2, mode="reference", mask="memory",
                        seed=500 + len(out)))
    return out


def _odd_head_cases():
    """H = 3 with R = 5 (mode "reference": (r * 3 + h) % 5 walks every row) and H = R = 1."""
    out = []
    for hd in (8, 64):
        out.append(case(f"heads3_hd{hd}", 5, 3, hd, 17, 33, mode="reference", mask="memory", seed=600 + len(out)))
        out.append(case(f"heads1_hd{hd}", 1, 1, hd, 17, 33, mask="memory", seed=600 + len(out)))
    return out


def _mask_cases():
    """Where the masked keys lie: the first key tiles wholly masked ("prefix": the online softmax starts on tiles with
    no visible key and recovers), every second key, and one visible key at the very end."""
    out = []
    for hd in (8, 64):
        out.append(case(f"mask_prefix_hd{hd}", 4, 2, hd, 17, 40, G=2, mask="prefix", seed=700 + len(out)))
        out.append(case(f"mask_alternate_hd{hd}", 4, 2, hd, 17, 33, G=2, mask="alternate", seed=700 + len(out)))
        out.append(case(f"mask_last_only_hd{hd}", 2, 2, hd, 17, 33, mask="last_only", seed=700 + len(out)))
    return out


WIDE_QSCALE = 8.0  # scale * s of N(0, 1) operands has a standard deviation of 1: 8 with q multiplied by this


def _wide_cases():
    """Logits with a standard deviation of 8, the keys sorted by their score against query 0: ascending, the running
    maximum rises in every tile and alpha = exp(m - m_new) sinks below fp32's resolution of what follows; descending,
    the later tiles' probabilities do."""
    out = []
    for hd in (8, 64):
        for order in ("ascending", "descending"):
            out.append(case(f"wide_cross_{order}_hd{hd}", 2, 2, hd, 17, 150, qscale=WIDE_QSCALE, key_order=order,
                            seed=800 + len(out)))
            out.append(case(f"wide_causal_{order}_hd{hd}", 2, 2, hd, 33, 33, causal=True, mask="pad", qscale=WIDE_QSCALE,
                            key_order=order, seed=800 + len(out)))
    return out


def _layout_cases():
    """The small cases the layout tests hand over in other forms; "row": the upstream gradient is one row, expanded."""
    out = []
    for hd in (8, 64):
        for dout in (None, "row"):
            tag = f"hd{hd}" + ("_doutrow" if dout else "")
            out.append(case(f"layout_cross_{tag}", 4, 2, hd, 17, 33, G=2, mask="memory", dout=dout, seed=900 + len(out)))
            out.append(case(f"layout_causal_{tag}", 2, 2, hd, 17, 17, causal=True, mask="pad", dout=dout, seed=900 + len(out)))
    return out


OLD_CASES = _edge_cases() + _causal_cases() + _group_cases() + _packed_cases()
NEW_CASES = _long_cases() + _group4_cases() + _odd_head_cases() + _mask_cases() + _wide_cases() + _layout_cases()
CASES = {c["name"]: c for c in OLD_CASES + NEW_CASES}
assert len(CASES) == len(OLD_CASES) + len(NEW_CASES)
CPU_CASES = ("causal_own_hd8_T17", "causal_reference_hd8_T17", "group_hd8_G1", "group_hd8_G2", "group_hd8_G3",
             "mask_prefix_hd8", "mask_alternate_hd8", "mask_last_only_hd8", "mask_last_only_hd64",
             "group4_reference_hd8", "group2_reference_hd8", "group2_reference_hd64", "heads3_hd8",
             "wide_cross_ascending_hd8", "layout_cross_hd8_doutrow")


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
    if c.get("qscale") is not None:
        q = q * c["qscale"]
    if c.get("key_order") is not None:
        score = torch.einsum("bhd,bhsd->bhs", q[::G, :, 0].double(), k.double())
        idx = score.argsort(-1, descending=c["key_order"] == "descending")[..., None].expand(B, H, S, hd)
        k, v = k.gather(2, idx), v.gather(2, idx)
    mask = None
    rows = R if c["mode"] == "reference" else B  # the mask rows the rule can read
    if c["mask"] == "pad":  # (R, T): trailing PAD of ragged length, and one PAD column before the end; never column 0
        mask = torch.zeros(R, T, dtype=torch.uint8)
        for r in range(R):
            n = T - (r * 5) % max(T // 2, 1)
            mask[r, n:] = 1
            if n > 3:
                mask[r, 1 + (r + 1) % (n - 2)] = 1
    elif c["mask"] == "memory":  # (rows, S): row 0 loses the whole key tile 16..31 and a tail, the others a ragged tail
        mask = torch.zeros(rows, S, dtype=torch.uint8)
        for b in range(rows):
            mask[b, S - 3 - 2 * b:] = 1
        if S > 32:
            mask[0, 16:32] = 1
    elif c["mask"] == "prefix":  # keys 0..31 of row 0 and 0..15 of the others: whole leading key tiles, the tail visible
        mask = torch.zeros(rows, S, dtype=torch.uint8)
        mask[0, :32] = 1
        mask[1:, :16] = 1
    elif c["mask"] == "alternate":  # every second key, rows starting on alternating parity
        mask = torch.zeros(rows, S, dtype=torch.uint8)
        for b in range(rows):
            mask[b, b % 2::2] = 1
    elif c["mask"] == "last_only":  # one visible key, the last: p = 1, l = 1, out is that V row
        mask = torch.ones(rows, S, dtype=torch.uint8)
        mask[:, S - 1] = 0
    elif c["mask"] is not None:
        raise ValueError(c["mask"])
    if c.get("dout") == "row":
        dout = torch.randn(1, 1, H * hd, generator=g).expand(R, T, H * hd)
    else:
        dout = torch.randn(R, T, H * hd, generator=g)
    return q, k, v, mask, dout


def mask_entries(c, mask, wrong=None):
    """(R, H, T, S) bool, True = masked, written out entry by entry. wrong: a deliberately wrong rule for the decisiveness
    checks ("no_causal", "other_mode", "mask_row0": every row reads row 0 of the key mask)."""
    R, H, T, S, G = (c[n] for n in ("R", "H", "T", "S", "G"))
    mode = c["mode"]
    if wrong == "other_mode":
        mode = "reference" if mode == "own" else "own"
    dead = torch.zeros(R, H, T, S, dtype=torch.bool)
    for r in range(R):
        for h in range(H):
            row = r // G if mode == "own" else (r * H + h) % R
            row = 0 if wrong == "mask_row0" else row
            for j in range(S):
                if mask is not None and row < mask.shape[0] and bool(mask[row, j] != 0):
                    dead[r, h, :, j] = True
                if c["causal"] and wrong != "no_causal":
                    dead[r, h, :j, j] = True
    return dead


def oracle(c, q, k, v, mask, dout, wrong=None):
    """fp64 -> (out, dq, dk, dv). wrong: None, or one of "group_mod" (K/V row r % B instead of r // G: the candidates
    interleaved instead of blocked), "no_causal", "other_mode", "mask_row0", "one_member" (dk / dv of the group's first
    row alone instead of the sum)."""
    R, H, T, hd, G = (c[n] for n in ("R", "H", "T", "hd", "G"))
    q64, k64, v64 = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    rows = torch.arange(R) % (R // G) if wrong == "group_mod" else torch.arange(R) // G
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


def lse_bound(c, q, k, v, mask, dout):
    """The relative-error term of recomputing p = exp(scale * s - lse) from one fp32 lse (module docstring), from fp64
    quantities alone: EPS32 * max|lse| * (largest sum of absolute terms of a gradient element) / max|gradient|.
    -> {"dq": .., "dk": .., "dv": ..}"""
    R, H, T, hd, S, G = (c[n] for n in ("R", "H", "T", "hd", "S", "G"))
    B, scale = R // G, float(hd) ** -0.5
    q64, g = q.double(), dout.double().reshape(R, T, H, hd).transpose(1, 2)
    ke, ve = k.double().repeat_interleave(G, 0), v.double().repeat_interleave(G, 0)
    s = ((q64 @ ke.transpose(-1, -2)) * scale).masked_fill(mask_entries(c, mask), float("-inf"))
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    dsum = ((p @ ve) * g).sum(-1, keepdim=True)
    ds = (p * (g @ ve.transpose(-1, -2) - dsum)).abs()
    over_group = lambda t: t.view(B, G, H, S, hd).sum(1)  # dk / dv sum over the rows of a group
    terms = dict(dq=scale * (ds @ ke.abs()), dk=over_group(scale * (ds.transpose(-1, -2) @ q64.abs())),
                 dv=over_group(p.transpose(-1, -2) @ g.abs()))
    x64 = dict(zip(("out", "dq", "dk", "dv"), oracle(c, q, k, v, mask, dout)))
    return {n: EPS32 * lse.abs().max().item() * t.max().item() / x64[n].abs().max().item() for n, t in terms.items()}


def check(c, got, inputs, ref=None, what=""):
    """Asserts the four tensors of `got` within the case's bounds of the fp64 oracle; prints each figure first.
    -> the errors."""
    q, k, v, mask, dout = inputs
    ref = oracle(c, q, k, v, mask, dout) if ref is None else ref
    wide = lse_bound(c, q, k, v, mask, dout) if c.get("qscale") is not None else {}
    errs = []
    for name, x, x64, base in zip(("out", "dq", "dk", "dv"), got, ref, BASELINE[c["name"]]):
        e = rel_err(x, x64)
        note = ""
        if e is None:
            e = (x.detach().double().cpu() - x64).abs().max().item()
            bound = zero_bound(c, q, k, v, dout)
            assert base is None, (c["name"], name)
        else:
            bound = FACTOR * base
            if name in wide:  # wide logits: printed beside the error; the kernels stay within FACTOR * base without it
                note = f" (lse term {wide[name]:.3e}, not in the bound)"
        print(f"{what}{c['name']:28s} {name:3s} err {e:.3e} bound {bound:.3e}{note}")
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
    "long_causal_hd8_T255": (1.436e-07, 6.205e-07, 6.428e-07, 4.687e-07),
    "long_causal_hd8_T256": (2.687e-07, 6.285e-07, 3.417e-07, 5.288e-07),
    "long_cross_hd8_T256_S17": (2.313e-07, 2.790e-07, 3.214e-07, 3.221e-07),
    "long_cross_hd8_T17_S300": (6.828e-07, 6.167e-07, 1.382e-07, 4.301e-07),
    "long_causal_hd64_T255": (2.076e-07, 3.932e-07, 4.471e-07, 5.034e-07),
    "long_causal_hd64_T256": (1.557e-07, 2.402e-07, 4.628e-07, 3.837e-07),
    "long_cross_hd64_T256_S17": (4.970e-07, 3.255e-07, 3.176e-07, 2.413e-07),
    "long_cross_hd64_T17_S300": (7.560e-07, 5.772e-07, 4.101e-07, 8.587e-07),
    "long_causal_reference_hd64_T256": (2.376e-07, 5.283e-07, 4.284e-07, 2.971e-07),
    "long_cross_hd64_T241_S241": (5.536e-07, 7.225e-07, 9.082e-07, 5.836e-07),
    "group4_own_hd8": (1.969e-07, 4.071e-07, 2.744e-07, 1.698e-07),
    "group4_reference_hd8": (3.048e-07, 4.866e-07, 1.607e-07, 1.886e-07),
    "group2_reference_hd8": (1.971e-07, 4.922e-07, 2.599e-07, 3.126e-07),
    "group4_own_hd64": (3.679e-07, 5.136e-07, 5.119e-07, 2.987e-07),
    "group4_reference_hd64": (3.865e-07, 3.877e-07, 3.576e-07, 2.641e-07),
    "group2_reference_hd64": (4.679e-07, 3.636e-07, 2.128e-07, 3.670e-07),
    "heads3_hd8": (2.494e-07, 6.461e-07, 4.751e-07, 2.563e-07),
    "heads1_hd8": (3.051e-07, 2.613e-07, 1.493e-07, 1.220e-07),
    "heads3_hd64": (3.661e-07, 4.048e-07, 4.368e-07, 3.261e-07),
    "heads1_hd64": (2.710e-07, 3.397e-07, 2.924e-07, 3.485e-07),
    "mask_prefix_hd8": (1.221e-07, 2.990e-07, 2.171e-07, 1.129e-07),
    "mask_alternate_hd8": (1.633e-07, 3.460e-07, 2.647e-07, 2.502e-07),
    "mask_last_only_hd8": (0.000e+00, None, None, 1.451e-07),
    "mask_prefix_hd64": (3.237e-07, 3.103e-07, 2.544e-07, 2.282e-07),
    "mask_alternate_hd64": (4.519e-07, 3.370e-07, 3.167e-07, 2.885e-07),
    "mask_last_only_hd64": (0.000e+00, None, None, 1.379e-07),
    "wide_cross_ascending_hd8": (4.766e-07, 2.414e-06, 1.615e-06, 3.556e-06),
    "wide_causal_ascending_hd8": (4.192e-07, 1.798e-06, 1.717e-06, 2.127e-06),
    "wide_cross_descending_hd8": (5.077e-07, 3.729e-06, 3.383e-06, 2.701e-06),
    "wide_causal_descending_hd8": (5.925e-07, 6.066e-07, 9.221e-07, 8.490e-07),
    "wide_cross_ascending_hd64": (1.340e-06, 2.146e-06, 1.570e-06, 1.597e-06),
    "wide_causal_ascending_hd64": (9.216e-07, 1.980e-06, 1.884e-06, 5.157e-07),
    "wide_cross_descending_hd64": (2.545e-06, 2.006e-06, 2.878e-06, 1.432e-06),
    "wide_causal_descending_hd64": (9.961e-07, 1.073e-06, 9.244e-07, 5.545e-07),
    "layout_cross_hd8": (1.166e-07, 3.395e-07, 3.026e-07, 4.235e-07),
    "layout_causal_hd8": (1.977e-07, 1.056e-07, 1.155e-07, 1.498e-07),
    "layout_cross_hd8_doutrow": (2.487e-07, 3.180e-07, 1.985e-07, 1.024e-07),
    "layout_causal_hd8_doutrow": (8.704e-08, 1.403e-07, 1.402e-07, 1.235e-07),
    "layout_cross_hd64": (3.790e-07, 3.633e-07, 3.652e-07, 3.781e-07),
    "layout_causal_hd64": (2.972e-07, 2.937e-07, 5.235e-07, 1.610e-07),
    "layout_cross_hd64_doutrow": (3.451e-07, 8.648e-07, 4.234e-07, 1.064e-07),
    "layout_causal_hd64_doutrow": (1.428e-07, 3.912e-07, 3.737e-07, 1.439e-07),
}


if __name__ == "__main__":
    torch.manual_seed(0)
    for name, c in CASES.items():
        row = ", ".join("None" if e is None else f"{e:.3e}" for e in measure_baseline(c))
        print(f'    "{name}": ({row}),')
    for name, c in CASES.items():
        if c["qscale"] is not None:
            print("# lse term", name, ", ".join(f"{n} {e:.3e}" for n, e in lse_bound(c, *build(c)).items()))
    c, inputs = fully_masked_case()
    print("BASELINE_FULLY_MASKED_OUT =", f"{finite_err(sdpa_parent(c, *inputs)[0], oracle(c, *inputs)[0], same_nan=False):.3e}")
