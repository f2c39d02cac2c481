"""bf16 mode (CSA_DTYPE_BF16) and dense train mode against an operand-exact oracle: the correctness bar.

Reference: oracle/closed_form.py with bf16=True, the fp64 closed form with exactly the operands the bf16 kernels
round rounded where they round them (audited against csrc/csa_sbm.hip: the sites are named in the oracle). What
is left between such an oracle and an honest kernel is fp32 accumulation and the sporadic bf16 roundings that
fp32 error flips, which closed_form.emulation_budget() measures from the oracle alone (the same code in fp32
against fp64 arithmetic, same graph, dropout masks and side of every ReLU tie). Tolerance per tensor class = 4 x the LARGEST budget over every
case of this file (the GPU's summation order and exp2 differ from the CPU's fp32, and a handful of cases
undersample the flips), floored at the fp32 suite's 1e-4; a tensor passes when both its element metric
(|got - ref| <= tol |ref| + tol max|ref|) and its relative Frobenius error are within it. No figure here was
taken from GPU output. tests/test_bf16_budget_cpu.py recomputes the budget of the N <= 64 cases and fails if a
constant drifts below 4 x what it finds.

Measured budget (oracle only, CPU; the larger of the element metric and the relative Frobenius error per class;
expA: largest absolute difference; ties = ReLU tie elements of the case, closed_form.TIE_FACTOR):

  case                                                  X         expA         dQKV layer.weight  proj.weight    proj.bias  ties
  eval (2, 2, 45, 64, 5)                          1.3e-07      7.4e-08      7.2e-07      3.7e-07      2.2e-05        8e-06     0
  eval (1, 2, 150, 96, 16)                        2.4e-07      7.6e-06      5.7e-05      3.3e-05      0.00011      9.9e-05     0
  eval (1, 2, 33, 64, 16)                           2e-07      8.2e-05      1.4e-07      1.3e-06        4e-05      5.8e-06     0
  eval (2, 2, 64, 64, 1)                          1.4e-07      6.6e-06      3.8e-07      5.7e-06      8.4e-06        3e-06     0
  train (2, 2, 150, 64, 10) proj_p=0.1            1.4e-07      1.8e-06        4e-06      2.5e-05      3.5e-05      2.5e-05     0
  train (1, 2, 45, 96, 5) proj_p=0.1              2.1e-07        8e-06      4.2e-08      2.7e-07      2.6e-06      5.7e-07     0
  train (1, 2, 45, 96, 5) proj_p=0.0              2.1e-07      9.5e-08      4.4e-08      2.6e-07        3e-07      1.2e-07     0
  dead (6, 2, 150, 64, 10) eval                     2e-07      1.3e-05      7.9e-05      9.5e-06      6.4e-05      3.9e-05     2
  dead (6, 2, 150, 64, 10) train                  2.3e-07      5.6e-05        2e-05      4.7e-05      8.5e-05      6.2e-05     1
  dead (6, 2, 100, 96, 16) eval                   1.5e-07      1.1e-05      3.8e-06      5.7e-05       0.0002      0.00011     0
  dead (6, 2, 100, 96, 16) train                  1.4e-07      3.2e-05       0.0011      1.8e-05      0.00034      0.00013     0
  dead (2, 1, 2080, 64, 10) eval                  1.5e-07      1.4e-05      9.3e-06      5.3e-06      1.2e-05        8e-06     1
  no-edge rows sbm_n150                           1.5e-07        3e-05      1.9e-06      0.00012      4.5e-05      2.6e-05     1
  degenerate sbm_n150                             1.6e-07        3e-05      1.5e-05      0.00017      0.00038      0.00012     1
  maps (2, 2, 37, 64, 10) eval                    1.8e-07      7.4e-08      9.7e-07      8.4e-07      3.2e-05      0.00011     0
  maps (2, 2, 37, 64, 10) train                   1.6e-07        1e-06      9.7e-06      1.3e-05       0.0003      0.00025     0
  maps (1, 2, 33, 96, 16) eval                    1.9e-07        1e-07      1.4e-07      7.2e-07        1e-05      7.4e-06     0
  maps (1, 2, 33, 96, 16) train                   1.5e-07      9.4e-08      3.5e-08      4.1e-07      2.7e-07        1e-07     0
  long (1, 1, 1024, 64, 16)                       0.00016      1.1e-05      0.00019      0.00026      0.00043       0.0015     0
  dense train (2, 2, 150, 64)                     3.1e-05            -        6e-05            -            -            -     -
  dense train (1, 2, 45, 96)                      1.3e-07            -      7.1e-08            -            -            -     -
  dense dead                                      0.00018            -      0.00019            -            -            -     -
  dense dattn                                     1.2e-07            -      7.3e-08            -            -            -     -
  largest                                        1.81e-04     8.24e-05     1.14e-03     2.56e-04     4.31e-04     1.49e-03
  TOL = max(4 x largest, 1e-4), rounded up        7.3e-04      3.3e-04      4.6e-03      1.1e-03      1.8e-03      6.0e-03

The fully masked AST test (7, 2, 64, 64, 10) is not part of the table: it compares four tensors of its live ASTs at
these constants. The sampled graph is compared with the oracle's own sampling on expA of the emulation; a draw within
TOL["expA"] of clamp(expA) is a tie (check_graph). The ReLU-tie rule (test_sbm_gpu._match_oracle_up_to_relu_ties)
applies to every comparison: at most 4 tie elements per case, as counted above.
"""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from csa_amd._lib import CSA_SCHED_CONCURRENT, CSA_SCHED_IN_ORDER
from oracle import closed_form, philox
from test_sbm_gpu import _dead_tile_masks, _match_oracle_up_to_relu_ties, _rand_case, _run_module

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]

RTOL, ATOL = 1e-4, 1e-5  # the fp32 suite's tolerance (dense fp32 train mode below)
FLOOR = 1e-4
# 4 x the largest emulation_budget value of the class over the cases below, floored at FLOOR (table above)
TOL = {"X": 7.3e-4, "expA": 3.3e-4, "dQKV": 4.6e-3, "layer.weight": 1.1e-3, "proj.weight": 1.8e-3, "proj.bias": 6.0e-3}
SEED, OFFSET, ATTN_P = (0x1234567 << 32) | 0x89ABCDE, 77, 0.2
PARAM_NAMES = ["layer.weight", "proj.0.weight", "proj.0.bias", "proj.3.weight", "proj.3.bias", "proj.6.weight",
               "proj.6.bias"]


def tol_class(name):
    if name in ("X", "expA"):
        return name
    if name in ("Q", "K", "V"):
        return "dQKV"
    if name == "layer.weight":
        return "layer.weight"
    return "proj.weight" if name.endswith("weight") else "proj.bias"


# ---------------------------------------------------------------------------------------------------------
# cases: everything the oracle needs (kw: keyword arguments of closed_form.sbm_fwd_bwd / dense_fwd_bwd) and
# everything the GPU run needs. Built on the CPU only (the budget test and the budget table use them too).
# ---------------------------------------------------------------------------------------------------------
def _attn_keep_mult(B, H, N, seed, offset, attn_p, M=None):
    keep = philox.attn_keep(B, H, N, N if M is None else M, seed, offset, attn_p)
    return keep, torch.from_numpy(keep / (1.0 - np.float32(attn_p)))


def sbm_case(shape, seed, train=False, mask=None, proj_p=0.1, maps=False, M=None):
    """shape = (B, H, N, d, k); M keys (M = N when absent)."""
    B, H, N, d, k = shape
    M = N if M is None else M
    Q, K, V, rmask, u, dX, dsp, params = _rand_case(B, H, N, d, k, seed=seed, M=M)
    mask = rmask if mask is None else mask
    kw = dict(Q=Q, K=K, V=V, mask=mask, params=params, u=u, num_clusters=k, dX=dX, dsparsity=dsp)
    c = dict(shape=shape, train=train, proj_p=proj_p if train else 0.0, attn_p=ATTN_P if train else 0.0, kw=kw)
    if train:
        c["keep"], kw["attn_keep"] = _attn_keep_mult(B, H, N, SEED, OFFSET, ATTN_P, M)
        kw["attn_p"] = ATTN_P
        if proj_p > 0:
            ks = 1.0 / (1.0 - np.float32(proj_p))
            kw["proj_keep"] = {f"{s}{l}": torch.from_numpy(philox.proj_keep(B, H, M if s == "k" else N, d, SEED, OFFSET,
                                                                            proj_p, l, int(s == "k")) * ks)
                               for s in "qk" for l in (0, 1)}
        c["u16"] = philox.attn_uniforms(B, H, N, M, SEED, OFFSET, philox.RNG_STE)
        kw["u"] = torch.from_numpy((c["u16"].astype(np.float64) + 0.5) / 65536.0)  # the oracle's own sampling
    if maps:
        g = torch.Generator().manual_seed(seed + 1)
        kw["dgraph"] = 1e-3 * torch.randn(B, H, N, M, generator=g)
        kw["dattn"] = torch.randn(B, H, N, M, generator=g)
    return c


def dense_case(shape, seed, train=False, mask=None, with_dattn=False, M=None):
    """shape = (B, H, N, d); M keys (M = N when absent)."""
    B, H, N, d = shape
    M = N if M is None else M
    g = torch.Generator().manual_seed(seed)
    Q = torch.randn(B, H, N, d, generator=g)
    K, V = (torch.randn(B, H, M, d, generator=g) for _ in range(2))
    dX = torch.randn(B, H, N, d, generator=g)
    if mask is None:
        mask = torch.zeros(B, M)
        mask[B - 1, M - M // 4:] = 1.0
    kw = dict(Q=Q, K=K, V=V, mask=mask, dX=dX)
    c = dict(shape=shape, train=train, attn_p=ATTN_P if train else 0.0, kw=kw)
    if train:
        c["keep"], kw["attn_keep"] = _attn_keep_mult(B, H, N, SEED, OFFSET, ATTN_P, M)
        kw["attn_p"] = ATTN_P
    if with_dattn:
        kw["dattn"] = torch.randn(B, H, N, M, generator=g)
    return c


EVAL_SHAPES = [(2, 2, 45, 64, 5), (1, 2, 150, 96, 16), (1, 2, 33, 64, 16), (2, 2, 64, 64, 1)]
TRAIN_CASES = [((2, 2, 150, 64, 10), 0.1), ((1, 2, 45, 96, 5), 0.1), ((1, 2, 45, 96, 5), 0.0)]
DEAD_SHAPES = [(6, 2, 150, 64, 10), (6, 2, 100, 96, 16)]
DEAD_LONG = (2, 1, 2080, 64, 10)
MAP_SHAPES = [(2, 2, 37, 64, 10), (1, 2, 33, 96, 16)]
LONG_SHAPE = (1, 1, 1024, 64, 16)
DENSE_TRAIN_SHAPES = [(2, 2, 150, 64), (1, 2, 45, 96)]
DENSE_DEAD_SHAPE = (6, 2, 150, 64)
DENSE_DATTN_SHAPE = (2, 2, 37, 64)


def eval_case(shape):
    return sbm_case(shape, seed=sum(shape))


def train_case(shape, proj_p):
    return sbm_case(shape, seed=3 * sum(shape), train=True, proj_p=proj_p)


def dead_case(shape, train):
    B, H, N, d, k = shape
    return sbm_case(shape, seed=97 + N, train=train, mask=_dead_tile_masks(B, N))


def map_case(shape, train):
    return sbm_case(shape, seed=5 * sum(shape), train=train, maps=True)


def dense_train_case(shape):
    return dense_case(shape, seed=sum(shape), train=True)


def dense_dead_case():
    B, H, N, d = DENSE_DEAD_SHAPE
    return dense_case(DENSE_DEAD_SHAPE, seed=55, mask=_dead_tile_masks(B, N))


def dense_dattn_case():
    return dense_case(DENSE_DATTN_SHAPE, seed=56, with_dattn=True)


def _golden_case(z, Qn=None, Kn=None, u=None):
    B, H, N, d, k = (int(v) for v in z["meta"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    params = {kk[2:]: t(v) for kk, v in z.items() if kk.startswith("p:")}
    kw = dict(Q=t(z["Q"] if Qn is None else Qn), K=t(z["K"] if Kn is None else Kn), V=t(z["V"]), mask=t(z["mask"]),
              params=params, u=t(z["u"] if u is None else u), num_clusters=k, dX=t(z["dX"]), dsparsity=t(z["dsparsity"]))
    return dict(shape=(B, H, N, d, k), train=False, proj_p=0.0, attn_p=0.0, kw=kw)


NO_EDGE_ROWS = [3, 40, 41, 77, 149]


def no_edge_case(z):
    """test_sbm_rows_without_edges_match_oracle's construction: u = 1 never samples."""
    u = z["u"].copy()
    u[:, :, NO_EDGE_ROWS, :] = 1.0
    return _golden_case(z, u=u)


DEGEN_I, DEGEN_J = 40, 77


def degenerate_case(z):
    """test_sbm_degenerate_normaliser_rows_match_oracle's construction (Q_i = K_j = t 1 with key j unsampled and
    every other key of row i sampled, so n_i < eps and rho_i = gamma_i: rec[3] != 0 in k_attn_bwd_qr), with t
    bisected under the bf16-ROUNDED scores the bf16 kernels see: t itself and every other operand of q_i . k
    rounded to bf16, so that n stays below 1e-12 in the emulation too."""
    B, H, N, d, k = (int(v) for v in z["meta"])
    R = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).double().numpy()
    Qn, Kn, u = z["Q"].copy(), z["K"].copy(), z["u"].copy()
    i, j = DEGEN_I, DEGEN_J
    valid = z["mask"] == 0
    assert valid[:, j].all()
    Rs = lambda t: float(torch.tensor(float(t), dtype=torch.float32).to(torch.bfloat16))
    Kr = R(Kn)

    def mass(t):
        tr = Rs(t)
        kk = Kr.copy()
        kk[:, :, j, :] = tr
        s = tr * kk.sum(-1) / np.sqrt(d)  # q_i = tr 1
        s = np.where(valid[:, None, :], s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        p[:, :, j] = 0.0
        return p.sum(-1)

    lo, hi = 0.5, 6.0  # n(t) falls as t grows
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if mass(mid).max() > 1e-13 else (lo, mid)
    t = Rs(hi)
    if mass(t).max() > 1e-13:  # rounding hi to bf16 went down a step: take the next bf16 value up
        t = Rs(t * (1 + 2.0 ** -7))
    n = mass(t)
    assert n.max() <= 1e-13 and n.min() > 1e-18, (n.max(), n.min())
    Qn[:, :, i, :], Kn[:, :, j, :] = t, t
    u[:, :, i, :] = 0.0
    u[:, :, i, j] = 1.0
    return _golden_case(z, Qn=Qn, Kn=Kn, u=u)


# ---------------------------------------------------------------------------------------------------------
# GPU runs through torch.ops.csa.* (explicit seed / offset, precision and schedule)
# ---------------------------------------------------------------------------------------------------------
def _weights(params):
    return (params["layer.weight"].cuda(), [params[f"proj.{i}.weight"].cuda() for i in (0, 3, 6)],
            [params[f"proj.{i}.bias"].cuda() for i in (0, 3, 6)])


def run_sbm_gpu(c, bf16=True, maps=True, schedule=CSA_SCHED_IN_ORDER, zero_maps=False, uniforms=None):
    """uniforms: host (B, H, N, M) draws handed to the forward whatever the mode (train mode with them is the
    HAS_U && DROP instantiation of k_attn_fwd); None: the case's own in eval mode, the kernel's Philox draws in train."""
    kw = c["kw"]
    k = kw["num_clusters"]
    cw, pw, pb = _weights(kw["params"])
    q, kk, v, mk = (kw[n].float().contiguous().cuda() for n in ("Q", "K", "V", "mask"))
    uu = None if c["train"] else kw["u"].float().cuda()
    if uniforms is not None:
        uu = uniforms.float().cuda()
    X, sp, state = torch.ops.csa.sbm_fwd(q, kk, v, mk, cw, pw, pb, uu, k, SEED, OFFSET, c["attn_p"], c["proj_p"],
                                         False, bf16, False)
    graph, _ = torch.ops.csa.sbm_maps(q, kk, v, mk, state, k, False)
    dg = kw["dgraph"].cuda() if maps and "dgraph" in kw else None
    da = kw["dattn"].cuda() if maps and "dattn" in kw else None
    if zero_maps:
        dg = da = torch.zeros_like(graph)
    g = torch.ops.csa.sbm_bwd(q, kk, v, mk, cw, pw, pb, k, c["attn_p"], c["proj_p"], SEED, OFFSET, False, state, X,
                              kw["dX"].cuda(), kw["dsparsity"].cuda(), dg, bf16, False, da, schedule)
    torch.cuda.synchronize()
    got = {"X": X.cpu(), "sparsity": sp.cpu(), "graph": graph.cpu()}
    got.update({n: t.cpu() for n, t in zip(["Q", "K", "V"] + PARAM_NAMES, g)})
    return got


def run_dense_gpu(c, bf16):
    kw = c["kw"]
    q, kk, v, mk = (kw[n].cuda() for n in ("Q", "K", "V", "mask"))
    X, _, state = torch.ops.csa.sbm_fwd(q, kk, v, mk, None, [], [], None, 0, SEED, OFFSET, c["attn_p"], 0.0, True,
                                        bf16, False)
    da = kw["dattn"].cuda() if "dattn" in kw else None
    g = torch.ops.csa.sbm_bwd(q, kk, v, mk, None, [], [], 0, c["attn_p"], 0.0, SEED, OFFSET, True, state, X,
                              kw["dX"].cuda(), None, None, bf16, False, da, CSA_SCHED_IN_ORDER)
    torch.cuda.synchronize()
    got = {"X": X.cpu()}
    got.update({n: t.cpu() for n, t in zip(["Q", "K", "V"], g)})
    return got


def close_emu(got, ref, name, label=""):
    """Both metrics of emulation_budget against the class's committed tolerance; prints the figures first."""
    tol = TOL[tol_class(name)]
    m, f = closed_form.elem_metric(got, ref), closed_form.fro_metric(got, ref)
    print(f"bf16-paths {label} {name}: element metric {m:.3g} Frobenius {f:.3g} (tol {tol:.3g})")
    assert m <= tol, f"{label} {name}: element metric {m:.3g} > {tol:.3g}"
    assert f <= tol, f"{label} {name}: relative Frobenius error {f:.3g} > {tol:.3g}"


def check_graph(c, got, ref):
    """The GPU's sampled graph equals the oracle's own sampling (expA of the bf16 emulation) away from ties. The fp32
    suite calls a draw within 1e-6 of clamp(expA) a tie: fp32 rounding of expA. In bf16 mode an honest kernel's expA is
    only within the emulation budget of the oracle's (one flipped bf16 rounding of an MLP activation moves a whole
    row of expA by ~1e-5: measured from the oracle alone, table above), so a tie is a draw within TOL["expA"]
    (absolute, 4 x the largest budget) -- and at most 1e-4 of the draws may differ at all."""
    expA = ref["expA"]
    band = TOL["expA"]
    if c["train"]:
        want = philox.ste_graph(expA.numpy(), c["u16"])
        thr = np.clip(expA.numpy(), 0.01, 0.99) * 65536.0
        diff = want != got["graph"].numpy().astype(bool)
        assert np.all(np.abs(c["u16"][diff] - thr[diff]) < 0.5 + band * 65536.0), f"{int(diff.sum())} graph flips away from ties"
        assert diff.mean() < 1e-4
    else:
        u = c["kw"]["u"].double()
        p = expA.clamp(0.01, 0.99)
        diff = (u < p) != got["graph"].bool()
        assert bool(torch.all((u - p).abs()[diff] < band)), f"{int(diff.sum())} graph flips away from ties"
        assert float(diff.double().mean()) < 1e-4


def check_sbm(c, got, label):
    """Graph, sparsity, X, dQ / dK / dV and every parameter gradient against closed_form(bf16=True) on the GPU's
    graph, under the ReLU-tie rule. Rows of an AST without a valid key are 0/0 in the reference: left out."""
    kw = c["kw"]
    live = kw["mask"].sum(1) < kw["mask"].shape[1]

    def run_oracle(ov):
        return closed_form.sbm_fwd_bwd(**kw, graph_override=got["graph"], bf16=True, relu_override=ov)

    def check(ref, rg):
        check_graph(c, got, ref)
        np.testing.assert_allclose(got["sparsity"].numpy(), ref["sparsity"].numpy(), rtol=1e-6)
        close_emu(got["X"][live], ref["X"][live], "X", label)
        for n in ("Q", "K", "V"):
            close_emu(got[n][live], rg[n][live], n, label)
        assert torch.all(got["K"][~live] == 0) and torch.all(got["V"][~live] == 0)
        if bool(live.all()):
            for n in PARAM_NAMES:
                close_emu(got[n], rg[n], n, label)

    nt = _match_oracle_up_to_relu_ties(run_oracle, check)
    print(f"bf16-paths {label}: {nt} ReLU tie element(s)")


def check_dense(c, got, bf16, label):
    kw = c["kw"]
    live = kw["mask"].sum(1) < kw["mask"].shape[1]
    ref, rg = closed_form.dense_fwd_bwd(**kw, bf16=bf16)
    if c["train"]:
        assert 0.75 < c["keep"].mean() < 0.85
    pairs = [("X", got["X"], ref["X"])] + [(n, got[n], rg[n]) for n in ("Q", "K", "V")]
    for n, a, r in pairs:
        if bf16:
            close_emu(a[live], r[live], n, label)
        else:
            np.testing.assert_allclose(a[live].numpy(), r[live].numpy(), rtol=RTOL, atol=ATOL, err_msg=n)
    assert torch.all(got["K"][~live] == 0) and torch.all(got["V"][~live] == 0)


# ---------------------------------------------------------------------------------------------------------
# SBM, bf16
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EVAL_SHAPES)
def test_bf16_eval_padded_shapes_match_emulation(shape):
    """Eval mode through the module (host uniforms, padded ASTs): partial last tile, k < 8, k = 16 (KPH 8), d = 96."""
    c = eval_case(shape)
    kw = c["kw"]
    X, sp, graph, dQ, dK, dV, grads = _run_module(kw["Q"], kw["K"], kw["V"], kw["mask"], kw["u"], kw["dX"],
                                                  kw["dsparsity"], kw["params"], kw["num_clusters"], bf16=True)
    got = {"X": X, "sparsity": sp, "graph": graph, "Q": dQ, "K": dK, "V": dV}
    got.update({n: grads[n] for n in PARAM_NAMES})
    check_sbm(c, got, f"eval{shape}")


@pytest.mark.parametrize("shape,proj_p", TRAIN_CASES)
def test_bf16_train_mode_matches_emulation_with_regenerated_masks(shape, proj_p):
    """Train mode end to end in bf16: k_attn_fwd<DROP, BF>, k_attn_bwd_kv<DROP, BF>, k_attn_bwd_qr<DROP> (the saved
    Rbits keep words) and k_proj_fwd_l<BF, PD> (proj_p = 0.1: the bf16 frag_chain's S4N / 2 side() calls must
    generate all NC DropWords; proj_p = 0: PD = false) against the emulation under the regenerated Philox masks."""
    c = train_case(shape, proj_p)
    assert 0.75 < c["keep"].mean() < 0.85
    if proj_p > 0:
        assert all(0.85 < float((t > 0).double().mean()) < 0.95 for t in c["kw"]["proj_keep"].values())
    check_sbm(c, run_sbm_gpu(c), f"train{shape} proj_p={proj_p}")


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("shape", DEAD_SHAPES)
def test_bf16_dead_key_tiles_match_emulation(shape, train):
    """The light paths of fully masked key tiles in bf16 (forward after the live tiles, k_attn_bwd_kv's masked key
    blocks, k_attn_bwd_qr over dead tiles), eval and train mode; the graph keeps sampled edges at padded keys."""
    c = dead_case(shape, train)
    got = run_sbm_gpu(c)
    assert float(got["graph"][:, :, :, 64:].sum()) > 0
    check_sbm(c, got, f"dead{shape} train={train}")


def test_bf16_dead_key_tiles_past_the_dead_tile_record():
    """N = 2080: 65 key tiles, past the 64-tile dead-tile record (every tile runs the full path), eval mode."""
    c = dead_case(DEAD_LONG, False)
    check_sbm(c, run_sbm_gpu(c), f"dead{DEAD_LONG}")


@pytest.mark.parametrize("bf16", [False, True])
def test_fully_masked_ast_gives_finite_x_and_zero_dk_dv(bf16):
    """An AST whose every key is masked (0/0 = NaN in the reference, sbm_attn.py:61-62): the kernels return a finite
    X (zero: k_attn_fwd's Z == 0 branch, with lse = +inf so that the backward's P is 0) and exactly zero dK / dV for
    it in both precisions, and the other ASTs of the batch are unaffected."""
    shape = (7, 2, 64, 64, 10)
    B, H, N, d, k = shape
    c = sbm_case(shape, seed=97 + N, mask=_dead_tile_masks(B, N))
    # no sparsity gradient: with one, dK of the masked AST carries that term's STE gradient of the edges sampled at its
    # (padded) keys, ~1e-9 here, and nothing else
    c["kw"]["dsparsity"] = torch.zeros_like(c["kw"]["dsparsity"])
    got = run_sbm_gpu(c, bf16=bf16)
    live = c["kw"]["mask"].sum(1) < N
    assert int((~live).sum()) == 1
    assert bool(torch.isfinite(got["X"][~live]).all())
    assert torch.all(got["K"][~live] == 0) and torch.all(got["V"][~live] == 0)

    def check(ref, rg):
        for n, a, r in [("X", got["X"], ref["X"])] + [(n, got[n], rg[n]) for n in ("Q", "K", "V")]:
            if bf16:
                close_emu(a[live], r[live], n, "fully-masked")
            else:
                np.testing.assert_allclose(a[live].numpy(), r[live].numpy(), rtol=RTOL, atol=ATOL, err_msg=n)

    _match_oracle_up_to_relu_ties(lambda ov: closed_form.sbm_fwd_bwd(**c["kw"], graph_override=got["graph"], bf16=bf16,
                                                                     relu_override=ov), check)


def test_bf16_rows_without_edges_match_emulation(golden):
    c = no_edge_case(golden("sbm_n150"))
    got = run_sbm_gpu(c)
    assert not got["graph"][:, :, NO_EDGE_ROWS, :].any() and not got["X"][:, :, NO_EDGE_ROWS, :].any()
    check_sbm(c, got, "no-edge rows")


def test_bf16_degenerate_normaliser_rows_match_emulation(golden):
    """rho = gamma != 0 (rec[3] of k_attn_rowprep) in k_attn_bwd_qr and k_attn_bwd_kv<BF>."""
    c = degenerate_case(golden("sbm_n150"))
    B, H, N, d, k = c["shape"]
    i, j = DEGEN_I, DEGEN_J
    got = run_sbm_gpu(c)
    g = got["graph"]
    assert not g[:, :, i, j].any() and g[:, :, i, :].sum() == B * H * (N - 1) and got["X"][:, :, i, :].abs().max() > 0
    ref, _ = closed_form.sbm_fwd_bwd(**c["kw"], graph_override=g, bf16=True)
    assert 0 < float(ref["n"][:, :, i].max()) < 1e-12  # degenerate under the bf16-rounded scores too
    check_sbm(c, got, "degenerate normaliser")


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("shape", MAP_SHAPES)
def test_bf16_map_gradients_match_emulation(shape, train):
    """Upstream dgraph / dattn in bf16 (k_attn_rowprep's gx, the DG = true instantiations of k_attn_bwd_qr and
    k_attn_bwd_kv, their ldz reads), eval and train mode; and zero dgraph / dattn give the training path's
    gradients (the two paths sum gamma in different orders: fp32 rounding apart, as the fp32 suite allows)."""
    c = map_case(shape, train)
    got = run_sbm_gpu(c)
    check_sbm(c, got, f"maps{shape} train={train}")
    g0 = run_sbm_gpu(c, maps=False)
    g1 = run_sbm_gpu(c, zero_maps=True)
    for n in ["Q", "K", "V"] + PARAM_NAMES:
        np.testing.assert_allclose(g1[n].numpy(), g0[n].numpy(), rtol=1e-4,
                                   atol=1e-5 * max(1.0, float(g0[n].abs().max())), err_msg=n)
    assert not torch.equal(got["Q"], g0["Q"])  # the upstream map gradients did reach dQ


def test_bf16_long_ast_matches_emulation():
    """N = 1024: k_attn_fwd and k_attn_bwd_qr take their > 64 KB dynamic-LDS branch."""
    c = eval_case(LONG_SHAPE)
    check_sbm(c, run_sbm_gpu(c), f"long{LONG_SHAPE}")


@pytest.mark.parametrize("shape", [(8, 8, 150, 64, 10), (4, 8, 150, 96, 10)])
def test_bf16_concurrent_backward_schedule_bit_identical(shape):
    """k_proj_bwd_s<D, true> kinds 1 and 2 (CSA_SCHED_CONCURRENT) against kind 3 (CSA_SCHED_IN_ORDER), train mode:
    bitwise identical outputs, the bf16 counterpart of test_concurrent_backward_schedule_bit_identical."""
    c = sbm_case(shape, seed=41 + shape[3], train=True)
    a = run_sbm_gpu(c, schedule=CSA_SCHED_IN_ORDER)
    b = run_sbm_gpu(c, schedule=CSA_SCHED_CONCURRENT)
    assert a.keys() == b.keys() and len(a) == 13
    for n in a:
        assert torch.equal(a[n], b[n]), n


def test_bf16_forward_only_state_gives_the_same_outputs():
    from csa_amd import ops
    B, H, N, d, k = 4, 8, 150, 64, 10
    Q, K, V, mask, u, _, _, params = _rand_case(B, H, N, d, k, seed=19)
    cw = params["layer.weight"].cuda().requires_grad_()
    proj = []
    for i in (0, 3, 6):
        proj += [params[f"proj.{i}.weight"].cuda().requires_grad_(), params[f"proj.{i}.bias"].cuda().requires_grad_()]
    q, kk, v, mk, uu = (t.cuda() for t in (Q, K, V, mask, u))
    ref = ops.sbm_attention(q, kk, v, mk, cw, proj, k, uniforms=uu, bf16=True)
    f32 = ops.sbm_attention(q, kk, v, mk, cw, proj, k, uniforms=uu, bf16=False)
    assert not torch.equal(ref[0].detach(), f32[0].detach())  # the bf16 forward ran
    for ctx in (torch.no_grad, torch.inference_mode):
        with ctx():
            assert ops._fwd_only(q, cw, *proj)
            got = ops.sbm_attention(q, kk, v, mk, cw, proj, k, uniforms=uu, bf16=True)
        for a, b in zip(ref, got):
            assert torch.equal(a.detach(), b)


def test_bf16_unsupported_cluster_count_raises():
    """bf16 SBM attention exists for k <= 16: k = 20 raises CSA_UNSUPPORTED_SHAPE (no silent fp32 fallback); fp32
    runs the same call; the dense bf16 path has no clusters and ignores k."""
    c = sbm_case((1, 2, 37, 64, 20), seed=9)
    with pytest.raises(RuntimeError, match=r"CSA_UNSUPPORTED_SHAPE: bf16 SBM attention is instantiated for k <= 16"):
        run_sbm_gpu(c, bf16=True)
    assert bool(torch.isfinite(run_sbm_gpu(c, bf16=False)["X"]).all())
    kw = c["kw"]
    q, kk, v, mk = (kw[n].cuda() for n in ("Q", "K", "V", "mask"))
    outs = [torch.ops.csa.sbm_fwd(q, kk, v, mk, None, [], [], None, kd, SEED, OFFSET, 0.0, 0.0, True, True, False)[0]
            for kd in (0, 20)]
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


# ---------------------------------------------------------------------------------------------------------
# dense (FullAttention, BASELINE config 4), both precisions
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", DENSE_TRAIN_SHAPES)
def test_dense_train_mode_matches_oracle(shape, bf16):
    """DENSE = true, DROP = true of k_attn_fwd, k_attn_bwd_kv and k_attn_bwd_qg (fp32) / k_attn_bwd_qr (bf16): the
    dense kernels draw the attention-dropout stream of the SBM ones (philox_tile / RNG_ATTN_DROP, the same
    counters), so the keep mask is philox.attn_keep; fp32 against dense_fwd_bwd at 1e-4 / 1e-5, bf16 against
    dense_fwd_bwd(bf16=True)."""
    c = dense_train_case(shape)
    check_dense(c, run_dense_gpu(c, bf16), bf16, f"dense-train{shape}")


def test_dense_bf16_dead_key_tiles_match_emulation():
    c = dense_dead_case()
    check_dense(c, run_dense_gpu(c, True), True, "dense-dead")


def test_dense_bf16_attn_gradient_matches_emulation():
    c = dense_dattn_case()
    check_dense(c, run_dense_gpu(c, True), True, "dense-dattn")
