"""Oracle of the decoding constraints (csa_amd.decode_ops.constrain_rows, csa_amd.decoding.DecodingConstraints), test
infrastructure only.

constrain_np restates the rule of include/csa_hip.h (csa_constrain_rows) as plain Python loops over the rows and the
positions of each row's history, with sets of token ids: no tensor op of the torch fallback appears in it. The penalty is
one numpy fp32 division or product per distinct token, correctly rounded as the rule asks, so the kernel and the
fallback are compared with it BITWISE (the int32 image of the whole logits array, NaN payloads and the sign of zero
included). Beside the array it counts the columns it banned and penalised, so a fixture can be shown to exercise a rule
before anything is compared."""
from types import SimpleNamespace

import numpy as np
import torch

from beam_ref import BOS, EOS_ID, PAD, search_case  # noqa: F401 (shared fixtures)


def constrain_np(z, ys, t, fin=None, repetition_penalty=1.0, no_repeat_ngram=0, min_length=0, eos_id=None, suppress=()):
    """-> namespace z (the constrained copy), banned and penalised (columns written by each rule, over all rows)."""
    z = np.array(z, dtype=np.float32, copy=True)
    rows, V = z.shape
    T = ys.shape[1]
    theta = np.float32(repetition_penalty)
    n = int(no_repeat_ngram)
    out = SimpleNamespace(z=z, banned=0, penalised=0)
    if not 0 <= t < T - 1:
        return out
    for r in range(rows):
        if fin is not None and fin[r]:
            continue
        h = [int(x) for x in ys[r, :t + 1]]
        L = len(h)
        banned = set()
        if n >= 1:
            for i in range(0, L - n + 1):
                same = True
                for k in range(n - 1):
                    if h[i + k] != h[L - (n - 1) + k]:
                        same = False
                if same:
                    banned.add(h[i + n - 1])
        if eos_id is not None and eos_id >= 0 and t < min_length:
            banned.add(int(eos_id))
        for s in suppress:
            banned.add(int(s))
        if theta != np.float32(1.0):
            seen = set()
            for v in h:
                if v in seen or not 0 <= v < V:
                    continue
                seen.add(v)
                x = z[r, v]
                with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                    z[r, v] = np.float32(x / theta) if x > 0 else np.float32(x * theta)
                out.penalised += 1
        for v in banned:
            if 0 <= v < V:
                z[r, v] = -np.inf
                out.banned += 1
    return out


def bits(a):
    """The int32 image of an fp32 array (numpy or torch): what `bitwise` compares."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the rule sets and launch classes shared by tests/test_constrain_cpu.py and tests/test_constrain_gpu.py ----

NGRAM = 3  # the n of the crossed cases: steps n - 2 and n - 1 are the last without and the first with a full n-gram
SUPPRESS = (1, 4, 17, 300, 50002, 10 ** 6, 2 ** 31 - 1)  # in and out of range, whatever V is


def rules(V):
    """name -> keyword arguments of constrain_rows / constrain_np: each rule alone and all together. The EOS of the
    length rule is the last column, so it exists for every V."""
    eos = V - 1
    each = {"penalty": dict(repetition_penalty=1.3),
            "penalty_below_one": dict(repetition_penalty=0.7),
            "ngram1": dict(no_repeat_ngram=1),
            "ngram2": dict(no_repeat_ngram=2),
            "ngram3": dict(no_repeat_ngram=NGRAM),
            "min_length": dict(min_length=NGRAM - 1, eos_id=eos),
            "suppress": dict(suppress=SUPPRESS)}
    each["all"] = dict(repetition_penalty=1.3, no_repeat_ngram=NGRAM, min_length=NGRAM - 1, eos_id=eos, suppress=SUPPRESS)
    return each


def steps(T, n=NGRAM):
    """The valid ones of t = 0, 1, n - 2, n - 1, T - 2."""
    return sorted({t for t in (0, 1, n - 2, n - 1, T - 2) if 0 <= t < T - 1})


KERNEL_ROWS = (1, 3, 70)
KERNEL_VS = (1, 19, 257, 1028, 50003)
KERNEL_TS = (2, 7, 256, 257, 1024)


def kernel_case(V, T, rows=max(KERNEL_ROWS), seed=0):
    """(z, ys, fin_some): z (rows, V) fp32 normal(0, 3) with zeros of both signs, -inf, +inf and NaN entries; ys (rows, T)
    int64 histories over a 3-symbol alphabet of in-range ids per row (so n-grams really repeat; for V < 3 the spare
    symbols are out of range), about one position in ten replaced by an id outside [0, V) (-1, V, V + 7, 2^40); fin_some
    (rows,) uint8 with every third row finished. The columns a step does not read hold valid ids as well: a kernel that
    read past t would ban or penalise what the oracle does not."""
    g = np.random.default_rng(7919 * seed + 31 * V + T)
    z = (3.0 * g.standard_normal((rows, V))).astype(np.float32)
    special = np.array([0.0, -0.0, -np.inf, np.inf, np.nan], dtype=np.float32)
    hit = g.random((rows, V)) < 0.15
    z[hit] = special[g.integers(0, len(special), size=int(hit.sum()))]
    ys = np.empty((rows, T), dtype=np.int64)
    outside = np.array([-1, V, V + 7, 2 ** 40], dtype=np.int64)
    for r in range(rows):
        alphabet = g.permutation(V)[:3] if V >= 3 else np.arange(3)
        ys[r] = alphabet[g.integers(0, 3, size=T)]
        off = g.random(T) < 0.1
        ys[r, off] = outside[g.integers(0, len(outside), size=int(off.sum()))]
    ys[:, 0] = BOS
    fin = (np.arange(rows) % 3 == 1).astype(np.uint8)
    return z, ys, fin


def run_op(z, ys, t, device="cpu", form="dev", fin=None, layout="plain", suppress=(), **kw):
    """constrain_rows on a fresh copy of z -> the int32 image of the WHOLE buffer the rows live in, and the image the
    same buffer would have had the rows been left alone. layout "shifted": the base moved by one float off the 16-byte
    boundary and the rows V + 3 apart, the gaps poisoned; form "host": t as an int instead of the device counter."""
    from csa_amd.decode_ops import constrain_rows
    rows, V = z.shape
    zt = torch.from_numpy(np.array(z, dtype=np.float32)).to(device)  # a copy: the op works in place
    if layout == "shifted":
        buf = torch.full((rows * (V + 3) + 1,), 77.0, dtype=torch.float32, device=device)
        view = buf[1:].view(rows, V + 3)[:, :V]
        view.copy_(zt)
    else:
        buf = zt
        view = zt
    before = bits(buf)
    yt = torch.from_numpy(np.array(ys, dtype=np.int64)).to(device)
    ft = None if fin is None else torch.from_numpy(np.array(fin, dtype=np.uint8)).to(device)
    st = torch.tensor(list(suppress), dtype=torch.int64).to(torch.int32).to(device) if len(suppress) else None
    step = int(t) if form == "host" else torch.tensor([t], dtype=torch.int32, device=device)
    out = constrain_rows(view, yt, step, fin=ft, suppress=st, **kw)
    assert out is view
    assert np.array_equal(yt.cpu().numpy(), ys)  # the token buffer is only read
    return bits(buf), before


def expected(want_z, rows, V, layout):
    """The int32 image that run_op returns when the rows hold want_z."""
    if layout != "shifted":
        return bits(want_z[:rows])
    buf = np.full(rows * (V + 3) + 1, 77.0, dtype=np.float32)
    buf[1:].reshape(rows, V + 3)[:, :V] = want_z[:rows]
    return bits(buf)


# ---- the generator runs (tiny model of beam_ref.search_case, B = 3, S = 7) ----

GEN_T = 12
GEN_MIN_LENGTH = 5


def output_faults(ids, n, min_length, suppress, eos=EOS_ID):
    """What a (rows, T - 1) output shows of what the constraints forbid, counted over rows: (n-grams occurring twice in
    BOS + the tokens up to the first EOS, rows whose first EOS comes before min_length tokens, suppressed ids)."""
    ids = np.asarray(ids).reshape(-1, np.asarray(ids).shape[-1])
    repeats = early = listed = 0
    for row in ids:
        seq = [BOS]
        for tok in row:
            seq.append(int(tok))
            if tok == eos:
                break
        grams = [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]
        repeats += len(grams) - len(set(grams))
        where = [i for i, tok in enumerate(row) if tok == eos]
        early += 1 if where and where[0] < min_length else 0
        listed += sum(1 for tok in row if int(tok) in suppress)
    return repeats, early, listed


GEN_SEED = 20   # of search_case: chosen on the CPU among 1..29, the unconstrained run of EVERY generator below shows all
GEN_SUPPRESS = (5, 11)  # three faults (a repeated bigram, an EOS before GEN_MIN_LENGTH tokens, a suppressed id)


def constraints(**kw):
    from csa_amd.model import DecodingConstraints
    base = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=GEN_MIN_LENGTH, suppress_ids=GEN_SUPPRESS,
                eos_id=EOS_ID)
    base.update(kw)
    return DecodingConstraints(**base)


def generator_case(seed=GEN_SEED, device="cpu"):
    m, enc, src_mask = search_case(seed=seed, device=device)
    m.process_data = lambda data: setattr(data, "src_mask", src_mask)
    m.encode = lambda data: (enc, 1, None, [], [])
    return m, enc, src_mask


def make(kind, m, **kw):
    from csa_amd.model import BeamSearchGenerator, CachedGreedyGenerator, SamplingGenerator
    if kind == "greedy":
        return CachedGreedyGenerator(m, GEN_T, **kw)
    if kind == "beam":
        return BeamSearchGenerator(m, GEN_T, 3, eos_id=EOS_ID, **kw)
    return SamplingGenerator(m, GEN_T, num_samples=2, eos_id=EOS_ID, **kw)


def run(kind, gen, enc, src_mask, **kw):
    if kind == "greedy":
        return gen(SimpleNamespace(), **kw)
    if kind == "beam":
        return gen.search(enc, src_mask, **kw)
    return gen.sample(enc, src_mask, seed=GEN_SEED, **kw)
