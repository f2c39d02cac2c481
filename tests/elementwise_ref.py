"""Oracles and case builders of the three elementwise train-step kernels: k_res_drop and k_gelu_drop
(csrc/csa_glue.hip) and k_adamw (csrc/csa_optim.hip). Used by test_elementwise_train_cpu.py, which
checks that the cases decide what they are built to decide, and by test_elementwise_train_gpu.py, which
runs the kernels against them.

  residual + dropout   numpy fp32, op for op (the kernel is compared bitwise):
                         scale = fl32(1 / fl32(1 - fl32(p)))
                         y     = x + where(keep, fl32(o * scale), fl32(0 * o))
                         d_o   = where(keep, fl32(dy * scale), fl32(0 * dy))
  GELU + dropout       fp64: gelu = h/2 (1 + erf(h / sqrt 2)), gelu' = cdf + h pdf, times mask and scale
  AdamW                fp64, the op order of the reference optimizer (script/optimizer.py:49-106), with
                       the GradScaler unscale by fl32(1 / scale) in front; its wrong variants as mutants

Keep masks are oracle/philox.py's (res_keep, ffn_keep, keep_threshold); flat_u16 exposes the raw 16-bit
draws under them, one Philox call per group of 8 elements, so that a test can look at the threshold's
neighbours."""
import functools
import math

import numpy as np
import torch

from oracle import philox

RES_STREAM, FFN_STREAM = philox.RNG_RES_DROP, philox.RNG_FFN_DROP

# ---- launch geometry of both dropout kernels (csa_glue.hip res_launch / ffn_launch) ----
LAUNCH_LINE = "const unsigned blocks = (unsigned)std::min<int64_t>((groups + 255) / 256, 256 * 16);"
STRIDE_LINE = "g < groups; g += (int64_t)gridDim.x * 256) {"
GROUP, WG, MAX_WGS = 8, 256, 256 * 16


def drop_launch(n):
    """(groups of 8 elements, workgroups of 256 threads, passes of the grid-stride loop) for n elements."""
    groups = (n + GROUP - 1) // GROUP
    blocks = min((groups + WG - 1) // WG, MAX_WGS)
    return groups, blocks, -(-groups // (blocks * WG)) if blocks else 0


N_SINGLE = list(range(1, 9))                                # one group, tail lengths 1..7 and a full one
N_SEVERAL = [GROUP * WG * 3 + r for r in range(8)]          # r > 0: the ragged group alone in a 4th workgroup
N_WRAP = GROUP * WG * MAX_WGS + GROUP * 300 + 5             # 8,391,013: a second pass of 301 groups, the last ragged
N_KEY = GROUP * WG * 3 + 5                                  # the size of the seed / offset cases

SEED_HI = 2 ** 63 + 0x0123456789ABCDEF                      # bit 31 of the key's high word set
SEEDS = [0, 2 ** 32 - 1, 2 ** 32, SEED_HI, 2 ** 64 - 1]
OFFSETS = [0, 1, 0x0FFFFFFF, 0xDEADBEEF]
P_THR = [(1e-5, 1), (0.2, 13108), (0.25, 16384), (0.5, 32768), (0.99999, 65536)]  # (p, ceil(fl32(p) * 65536))
SEED_THR, OFFSET_THR = SEED_HI, 1

PAD = 64                                                    # floats behind the output that must stay as they were
SENTINEL = np.float32(-123.456)


def flat_u16(n, seed, offset, stream):
    """(n,) uint16: the raw 16-bit draw of memory element i on `stream`, which res_keep / ffn_keep compare
    with the threshold: u16 (i & 7) of philox({lo32(i >> 3), hi32(i >> 3), 0, (stream << 28) ^ lo32(offset)},
    seed). Cached (read-only): the large cases share one stream per (seed, offset)."""
    return _flat_u16(int(n), int(seed), int(offset), int(stream))


@functools.lru_cache(maxsize=4)
def _flat_u16(n, seed, offset, stream):
    g = np.arange((n + 7) // 8, dtype=np.uint64).reshape(-1, 1)
    words = philox.philox4x32(g & philox.MASK32, g >> np.uint64(32), 0,
                              ((stream << 28) ^ (offset & 0xFFFFFFFF)) & 0xFFFFFFFF,
                              seed & 0xFFFFFFFF, seed >> 32)
    u = philox.u16_of(words, np.arange(8).reshape(1, 8)).astype(np.uint16).reshape(-1)[:n].copy()
    u.setflags(write=False)
    return u


def keep_of(u16, p):
    """keep <=> u16 >= ceil(fl32(p) * 65536); the threshold 65536 keeps nothing."""
    return u16.astype(np.uint32) >= np.uint32(philox.keep_threshold(p))


def drop_scale(p):
    """The kernels' fp32 scale: 1.f / (1.f - p)."""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def res_fwd(x, o, keep, p):
    with np.errstate(all="ignore"):
        return x + np.where(keep, o * drop_scale(p), np.float32(0) * o)


def res_bwd(dy, keep, p):
    with np.errstate(all="ignore"):
        return np.where(keep, dy * drop_scale(p), np.float32(0) * dy)


def image(values):
    """The int32 image of an output buffer that holds `values` followed by PAD untouched sentinels."""
    buf = np.full(values.size + PAD, SENTINEL, dtype=np.float32)
    buf[:values.size] = values
    return buf.view(np.int32)


FLT_MAX = np.finfo(np.float32).max
SPECIALS = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-40, -1e-40, FLT_MAX, -FLT_MAX], dtype=np.float32)


def res_special_case(keep, rng):
    """x, o (fp32, keep.size) of ordinary values with every pair (x special, o special) placed once at a kept
    and once at a dropped position, read from the mask; the last element (the ragged tail) is special too."""
    n = keep.size
    x, o = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
    pairs = [(a, b) for a in SPECIALS for b in SPECIALS]
    kept, dropped = np.flatnonzero(keep), np.flatnonzero(~keep)
    assert kept.size >= len(pairs) and dropped.size >= len(pairs)
    for idx in (kept[:len(pairs)], dropped[:len(pairs)]):
        x[idx] = [a for a, _ in pairs]
        o[idx] = [b for _, b in pairs]
    x[n - 1], o[n - 1] = np.float32(1e-40), np.float32(-np.inf)
    return x, o


@functools.lru_cache(maxsize=1)
def wrap_inputs():
    """Two read-only fp32 arrays of N_WRAP ordinary values, shared by the stride-wrap cases."""
    rng = np.random.default_rng(20)
    a, b = rng.standard_normal(N_WRAP, dtype=np.float32), rng.standard_normal(N_WRAP, dtype=np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


# ---- GELU + dropout in fp64 ----

def gelu64(h):
    h = torch.as_tensor(np.asarray(h, dtype=np.float64))
    return (h * 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))).numpy()


def gelu_d64(h):
    h = torch.as_tensor(np.asarray(h, dtype=np.float64))
    cdf = 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)
    return (cdf + h * pdf).numpy()


def _scale64(p):
    return float(drop_scale(p)) if p > 0 else 1.0


def gelu_fwd64(h, keep, p):
    with np.errstate(all="ignore"):
        z = gelu64(h)
        return np.where(keep, z * _scale64(p), 0.0 * z)


def gelu_bwd64(dy, h, keep, p):
    with np.errstate(all="ignore"):
        dy = np.asarray(dy, dtype=np.float64)
        return np.where(keep, dy * _scale64(p), 0.0 * dy) * gelu_d64(h)


GELU_FINITE_SPECIALS = [0.0, -0.0, 1e-40, -1e-40, 1e-30, -1e-30, 40.0, -40.0, 88.0, -88.0]


def gelu_values(rng):
    """[-14, 14] in 2^16 steps plus the finite special values, shuffled: 65546 fp32 values (a ragged tail of 2)."""
    h = np.concatenate([np.linspace(-14.0, 14.0, 2 ** 16), GELU_FINITE_SPECIALS]).astype(np.float32)
    rng.shuffle(h)
    return h


def mask_visible_values(n, rng):
    """h = +-[1, 3] and dy = +-[0.5, 2]: gelu(h), gelu'(h) and dy are far from 0, so an output element is an
    exact 0 exactly where the mask dropped it."""
    sign = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)
    h = (sign() * rng.uniform(1.0, 3.0, n)).astype(np.float32)
    dy = (sign() * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    return h, dy


# ---- AdamW in fp64 ----

ADAMW_HP = dict(lr=0.05, weight_decay=0.3, betas=(0.8, 0.95), eps=1e-3)
ADAMW_STEP0 = 3                                  # the state is that of an optimizer after 3 steps
ADAMW_SIZES = [1, 3, 4, 4095, 0, 4096, 4097, 10005, 3 * 4096 + 7, 2 * 4096]
ADAMW_RTOL, ADAMW_ATOL, ADAMW_ATOL_V = 1e-5, 1e-7, 1e-12
GRAD_SCALE = 3073.0
MUTANTS = ["eps_in_root", "decay_pre_update", "decay_in_grad", "no_bias_correction", "betas_swapped"]


def adamw64(p, m, v, g, t, correct_bias, mutant=None, inv_scale=1.0, lr=0.05, weight_decay=0.3,
            betas=(0.8, 0.95), eps=1e-3):
    """One step of the reference AdamW in fp64, its t-th: (p, m, v) -> new (p, m, v). g is the gradient as
    the optimizer is handed it; inv_scale = fl32(1 / grad_scale) under a GradScaler. `mutant` names one
    wrong variant (MUTANTS)."""
    p, m, v = (np.asarray(a, dtype=np.float64) for a in (p, m, v))
    g = np.asarray(g, dtype=np.float64) * float(inv_scale)
    b1, b2 = betas if mutant != "betas_swapped" else betas[::-1]
    decay = lr * weight_decay
    if mutant == "decay_in_grad":                # L2 regularisation instead of the decoupled decay
        g = g + weight_decay * p
    m = m * b1 + (1.0 - b1) * g
    v = v * b2 + (1.0 - b2) * g * g
    den = np.sqrt(v + eps * eps) if mutant == "eps_in_root" else np.sqrt(v) + eps
    step = lr
    if correct_bias and mutant != "no_bias_correction":
        step = step * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    if mutant == "decay_pre_update":
        return p - step * m / den - decay * p, m, v
    q = p - step * m / den
    if mutant != "decay_in_grad":
        q = q - decay * q
    return q, m, v


def adamw_grads(signs, rng):
    """Gradients of magnitude 1e-2 .. 10 (log-uniform) with the given signs."""
    return [(sg * 10.0 ** rng.uniform(-2.0, 1.0, sg.size)).astype(np.float32) for sg in signs]


def adamw_case(sizes=ADAMW_SIZES, seed=7, steps=4):
    """Parameters, a non-zero optimizer state and `steps` gradients per tensor, all fp32. The state is a
    plausible one (exp_avg_sq of the order of exp_avg^2), so that the update is a sizeable fraction of
    many parameters: what makes the decay's place and the eps's place visible at the test's tolerance.
    An element's gradient has a random sign and keeps it over the steps, its magnitude is drawn anew each
    step. With signs drawn anew, 0.8 m + 0.2 g would now and then cancel terms of size 2 (ulp 2.4e-7) to
    nearly 0, where fp32 itself cannot hold exp_avg to the absolute tolerance of 1e-7 over four steps; in
    the first step the state (|m| < 1.3) and the gradient have unrelated signs, so cancellation is there."""
    rng = np.random.default_rng(seed)
    p = [(0.2 * rng.standard_normal(n)).astype(np.float32) for n in sizes]
    m = [(0.3 * rng.standard_normal(n) * 10.0 ** rng.uniform(-2.0, 0.0, n)).astype(np.float32) for n in sizes]
    v = [(a.astype(np.float64) ** 2 * rng.uniform(0.5, 2.0, a.size)).astype(np.float32) + np.float32(1e-12)
         for a in m]
    signs = [np.where(rng.random(n) < 0.5, -1.0, 1.0) for n in sizes]
    return dict(p=p, m=m, v=v, g=[adamw_grads(signs, rng) for _ in range(steps)])


def scaled_grads(grads, scale=GRAD_SCALE):
    """What backward leaves under GradScaler: fl32(g * scale)."""
    return [(g * np.float32(scale)).astype(np.float32) for g in grads]


def inv_scale32(scale=GRAD_SCALE):
    return float(np.float32(1.0 / float(np.float32(scale))))
