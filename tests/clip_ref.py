"""fp64 oracle and case builders of global gradient-norm clipping in the fused AdamW step (k_grad_sumsq,
k_grad_norm_finish and the clipped k_adamw of csrc/csa_optim.hip; csa_amd.train.AdamW(max_grad_norm=...)).
Used by test_grad_clip_cpu.py, which needs no GPU, and by test_grad_clip_gpu.py.

The oracle: the fp64 L2 norm over every gradient of the step, taken on the UNSCALED gradients (under a
GradScaler: sqrt(sum g^2) / scale), torch.nn.utils.clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)),
then elementwise_ref.adamw64 on g * inv_scale * coef. A non-finite norm skips the step (the state is returned
as it was, coefficient 0) where torch would write NaN into every parameter.

Tolerances. Parameters and moments keep the AdamW ones (elementwise_ref.ADAMW_RTOL 1e-5, ADAMW_ATOL 1e-7,
ADAMW_ATOL_V 1e-12): the clipped step adds one fp32 multiply per gradient, one rounding of 6e-8 relative. The
norm and the coefficient: NORM_RTOL = 1e-6 against fp64. The device accumulates exact fp64 squares of fp32
values over fewer than 2^24 terms (relative error below 2^24 * 1.1e-16 = 2e-9), the cast of the norm to fp32
leaves 6e-8, and the coefficient's fp32 add and divide leave 6e-8 each.

Every test of a clipped step starts from the NON-ZERO optimizer state of elementwise_ref.adamw_case(): from a
zero state Adam's m / sqrt(v) does not change under a constant scale of the gradient, so a test from a zero
state would pass with no clipping at all."""
import math

import numpy as np

import elementwise_ref as ref

NORM_RTOL = 1e-6
CLIP_EPS = 1e-6                         # clip_grad_norm_'s
MAX_NORMS = (1.0, 50.0)                 # clipping active on adamw_case() (global norm 554.13)
MAX_NORM_INACTIVE = 1e4                 # above that norm: coefficient exactly 1
CLIP_MUTANTS = ("no_clip", "per_tensor", "scaled_norm", "unclamped")
FINISH_PASSES_N = 257 * 4096 + 5        # 258 chunks: the finish kernel's strided loop passes its 256 lanes twice


def sumsq64(grads):
    return float(sum(np.square(np.asarray(g, dtype=np.float64)).sum() for g in grads))


def global_norm64(grads, scale=1.0):
    """L2 norm over all of `grads` (as the optimizer is handed them), divided by the GradScaler's scale."""
    return math.sqrt(sumsq64(grads)) / float(scale)


def clip_coef64(norm, max_norm, clamp=True):
    c = float(max_norm) / (norm + CLIP_EPS)
    return min(1.0, c) if clamp else c


def clipped_step64(state, grads, t, correct_bias, max_norm, scale=None, mutant=None):
    """One clipped AdamW step in fp64, the optimizer's t-th: state = [(p, m, v)] per tensor, grads as the
    optimizer is handed them (scaled by `scale` under a GradScaler; the update then unscales by
    fl32(1 / scale) as GradScaler.unscale_ does) -> (new state, norm, coefficient). `mutant` names a wrong
    variant (CLIP_MUTANTS): no clipping; each tensor clipped by its own norm; the norm taken on the scaled
    gradients (unscale forgotten); the coefficient not clamped at 1."""
    inv = 1.0 if scale is None else ref.inv_scale32(scale)
    norm = global_norm64(grads, 1.0 if scale is None or mutant == "scaled_norm" else scale)
    if not math.isfinite(norm):
        return list(state), norm, 0.0
    coef = clip_coef64(norm, max_norm, clamp=mutant != "unclamped")
    out = []
    for s, g in zip(state, grads):
        c = coef
        if mutant == "no_clip":
            c = 1.0
        elif mutant == "per_tensor":
            c = clip_coef64(global_norm64([g], 1.0 if scale is None else scale), max_norm)
        out.append(ref.adamw64(*s, g, t, correct_bias, inv_scale=inv * c, **_hp()))
    return out, norm, coef


def _hp():
    hp = dict(ref.ADAMW_HP)
    return dict(lr=hp["lr"], weight_decay=hp["weight_decay"], betas=hp["betas"], eps=hp["eps"])


def clipped_steps64(case, grads_per_step, correct_bias, max_norm, scale=None, t0=ref.ADAMW_STEP0):
    """Several clipped steps from the case's state -> ([p], [m], [v]) per tensor, [norm per step], [coef per step]."""
    state = [(p, m, v) for p, m, v in zip(case["p"], case["m"], case["v"])]
    norms, coefs = [], []
    for k, grads in enumerate(grads_per_step):
        state, n, c = clipped_step64(state, grads, t0 + 1 + k, correct_bias, max_norm, scale)
        norms.append(n)
        coefs.append(c)
    return [[s[j] for s in state] for j in range(3)], norms, coefs


def outside_fraction(got_p, want_p):
    """Share of all parameter elements whose |got - want| exceeds the AdamW tolerance around `want`."""
    bad = total = 0
    for g, w in zip(got_p, want_p):
        bad += int((np.abs(g - w) > ref.ADAMW_ATOL + ref.ADAMW_RTOL * np.abs(w)).sum())
        total += w.size
    return bad / total


def chunk_tables(sizes, chunk=4096):
    """Host tables of csa_grad_sumsq for tensors of `sizes` elements: chunk -> tensor (int32), first chunk per
    tensor (int64), chunk count; stated here on its own, not taken from csa_amd.train."""
    owner, start, n = [], [], 0
    for t, s in enumerate(sizes):
        start.append(n)
        k = -(-s // chunk)
        owner += [t] * k
        n += k
    return np.array(owner, dtype=np.int32), np.array(start, dtype=np.int64), n


def chunk_sumsq64(grads, chunk=4096):
    """The per-chunk fp64 sums of squares, in the order of the tables above."""
    out = []
    for g in grads:
        g = np.asarray(g, dtype=np.float64)
        out += [float(np.square(g[i:i + chunk]).sum()) for i in range(0, g.size, chunk)]
    return np.array(out, dtype=np.float64)
