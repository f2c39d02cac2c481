"""Rectangular attention: N queries against M != N keys, through every SBM and dense kernel, fp32 and bf16.

The C ABI (include/csa_hip.h) gives the SBM and dense entry points separate N and M, and csrc/csa_sbm.hip sizes and
indexes the query side (Qh, dQh, stats, brow, NQB) and the key side (Kh, T, dT, NKB, Mpad) apart; every other test
of the suite runs with N = M, where an index expression that takes one for the other is invisible. Here the two
differ in every case, so such a swap lands on the wrong element (or past a buffer) and the result leaves the oracle.

Shapes are (B, H, N, M, d, k) (dense: (B, H, N, M, d)), seed = sum(shape), each the smallest at which a path differs:
NQB < NKB and NQB > NKB with ragged last tiles, one query row, one key (rows without an edge), d = 96, k in 17..32,
KT = 2 and 4 (k_proj_fwd, grid NQB + NKB), M > 256 (the key-mask tail loop), NKB = 65 past the dead-tile record, and
many query blocks over one key block. Reference: oracle/closed_form.py in fp64 on the GPU's sampled graph, under the
ReLU-tie rule of test_sbm_gpu._match_oracle_up_to_relu_ties, at the fp32 suite's 1e-4 / 1e-5; the sampled graph may
differ from the oracle's own sampling only at fp32 ties and in fewer than 1e-4 of the draws. Train mode regenerates
the kernels' Philox streams with oracle/philox.py over (N, M) and rows = N (Q MLP) / M (K MLP).
tests/test_sbm_rect_cpu.py pins the reference side of every case here on the CPU (the two oracles agree, at most 4
ReLU tie elements per case, a case with no-edge rows, a case with a fully valid mask).

bf16 mode against closed_form.sbm_fwd_bwd(bf16=True) with the metrics of tests/test_bf16_paths_gpu.py. Tolerance per
tensor class = the larger of that file's TOL and 4 x the LARGEST emulation budget over the bf16 cases of this file,
floored at 1e-4. Measured budget (closed_form.emulation_budget, oracle only, CPU; the larger of the element metric
and the relative Frobenius error per class; expA: largest absolute difference; ties = ReLU tie elements):

  case                                                    X         expA         dQKV layer.weight  proj.weight    proj.bias  ties
  eval (2, 2, 45, 70, 64, 5)                        1.2e-07      1.2e-05      4.4e-05      0.00013       0.0007      0.00041     0
  eval (2, 2, 70, 33, 64, 10)                       1.7e-07      6.6e-08      1.7e-06        5e-07      1.2e-05      5.6e-06     0
  eval (1, 2, 40, 150, 96, 16)                      1.8e-07      1.2e-07        2e-07      7.5e-07      2.1e-05      3.8e-06     0
  eval (1, 2, 100, 1, 64, 10)                             0      6.1e-08       0.0006      2.8e-05      0.00066      0.00037     0
  train (2, 2, 70, 33, 64, 10)                      1.5e-07      6.8e-08      3.2e-07      8.7e-07      1.4e-05      9.4e-06     0
  train + maps (1, 2, 40, 150, 96, 16)              2.2e-07      1.2e-07      1.9e-07        8e-07      1.1e-05        1e-05     0
  dead (1, 1, 40, 2080, 64, 10)                     2.2e-07      5.1e-05      7.7e-05      1.9e-05      2.4e-05      3.8e-05     0
  dense train (2, 2, 45, 70, 64)                    1.4e-07            -      2.7e-07            -            -            -     -
  largest                                          2.20e-07     5.15e-05     5.97e-04     1.30e-04     6.96e-04     4.09e-04
  4 x largest                                      8.80e-07     2.06e-04     2.39e-03     5.20e-04     2.78e-03     1.64e-03
  TOL of test_bf16_paths_gpu.py                    7.30e-04     3.30e-04     4.60e-03     1.10e-03     1.80e-03     6.00e-03
  TOL here (the larger, rounded up)                 7.3e-04      3.3e-04      4.6e-03      1.1e-03      2.8e-03      6.0e-03

Only proj.weight exceeds the other file's constant. (With the key masks of _dead_tile_masks, B = 1 has ONE valid key:
every attention gradient cancels there and the budget of what is left of proj.weight is 2.6e-3, which would put 1e-2
on every case; the dead-tile case of this file therefore masks the first, the third and the tail tiles, rect_case.)

No figure here was taken from GPU output. tests/test_sbm_rect_cpu.py recomputes the budget of the cases with
N, M <= 150 and fails if a constant drifts below 4 x what it finds.
"""
import numpy as np
import pytest
import torch

import test_bf16_paths_gpu as T
from conftest import has_gpu
from csa_amd._lib import CSA_SCHED_CONCURRENT, CSA_SCHED_IN_ORDER
from oracle import closed_form, philox
from test_bf16_paths_gpu import (OFFSET, PARAM_NAMES, SEED, check_dense, check_sbm, dense_case, run_dense_gpu,
                                 run_sbm_gpu, sbm_case)
from test_sbm_gpu import ATOL, RTOL, _dead_tile_masks, _match_oracle_up_to_relu_ties, _run_module

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]

# max(T.TOL, 4 x the largest emulation_budget value of the class over the bf16 cases below, 1e-4) (table above)
TOL = {"X": 7.3e-4, "expA": 3.3e-4, "dQKV": 4.6e-3, "layer.weight": 1.1e-3, "proj.weight": 2.8e-3, "proj.bias": 6.0e-3}

# ---------------------------------------------------------------------------------------------------------
# cases (built on the CPU only: tests/test_sbm_rect_cpu.py uses them too)
# ---------------------------------------------------------------------------------------------------------
EVAL_SHAPES = [(2, 2, 45, 70, 64, 5),     # NQB 2 < NKB 3, ragged last tiles on both sides, 16-wide cluster products
               (2, 2, 70, 33, 64, 10),    # NQB 3 > NKB 2
               (1, 2, 1, 100, 64, 10),    # one query row
               (1, 2, 100, 1, 64, 10),    # one key: every row has 0 or 1 edge
               (1, 3, 40, 150, 96, 20),   # d = 96, k in 17..32
               (1, 2, 96, 31, 64, 64),    # KT = 2 (k_proj_fwd, grid NQB + NKB), M < 32 < N
               (1, 1, 33, 300, 64, 128),  # KT = 4, M > 256 (the key-mask tail loop past KB_UNROLL)
               (1, 1, 40, 2080, 64, 10),  # NKB = 65 > TDEAD_TILES with NQB = 2
               (1, 1, 300, 20, 96, 32)]   # many query blocks over one key block, d = 96
TRAIN_SHAPES = [(2, 2, 70, 33, 64, 10), (1, 2, 40, 150, 96, 5)]
MAP_SHAPE = (2, 2, 37, 70, 64, 10)
DEAD_SHAPES = [(6, 2, 40, 150, 64, 10), (2, 1, 40, 2080, 64, 10)]
DENSE_SHAPES = [(2, 2, 45, 70, 64), (1, 2, 100, 1, 96), (2, 2, 70, 33, 64)]
SCHED_SHAPES = [(4, 8, 45, 150, 64, 10), (4, 8, 150, 45, 96, 10)]  # G_K != G_Q
LAYOUT_SHAPE = (2, 2, 45, 70, 64, 10)
BF16_EVAL_SHAPES = [(2, 2, 45, 70, 64, 5), (2, 2, 70, 33, 64, 10), (1, 2, 40, 150, 96, 16), (1, 2, 100, 1, 64, 10)]
BF16_TRAIN_SHAPE = (2, 2, 70, 33, 64, 10)
BF16_MAP_SHAPE = (1, 2, 40, 150, 96, 16)
BF16_DEAD_SHAPE = (1, 1, 40, 2080, 64, 10)
BF16_DENSE_SHAPE = (2, 2, 45, 70, 64)


def rect_case(shape, train=False, maps=False, dead=False):
    """dead=True: the key masks of _dead_tile_masks(B, M). dead="tail" (for B = 1, where _dead_tile_masks leaves ONE
    valid key: every attention gradient cancels to zero there, and what is left of the parameter gradients is so
    small that its emulation budget is 2.6e-3): the case's random suffix padding (at least M / 3 valid keys, so whole
    tail tiles are masked) with the first key tile and the third masked as well."""
    B, H, N, M, d, k = shape
    c = sbm_case((B, H, N, d, k), seed=sum(shape), train=train, maps=maps, M=M,
                 mask=_dead_tile_masks(B, M) if dead is True else None)
    if dead == "tail":
        mask = c["kw"]["mask"]
        mask[:, :32] = 1.0
        mask[:, 64:96] = 1.0
        assert bool((mask[:, -32:] == 1).all()) and bool(((mask == 0).sum(1) > 32).all())
    return c


def rect_dense_case(shape, with_dattn=True):
    """Train mode (attention dropout), by default with an upstream gradient of the attn map."""
    B, H, N, M, d = shape
    return dense_case((B, H, N, d), seed=sum(shape), train=True, with_dattn=with_dattn, M=M)


def fp32_cases():
    """(label, case) of every fp32 SBM case of this file that is compared with the oracle."""
    cases = [(f"eval{s}", rect_case(s)) for s in EVAL_SHAPES]
    cases += [(f"train{s}", rect_case(s, train=True)) for s in TRAIN_SHAPES]
    cases += [(f"maps{MAP_SHAPE} train={tr}", rect_case(MAP_SHAPE, train=tr, maps=True)) for tr in (False, True)]
    cases += [(f"dead{s} train={tr}", rect_case(s, train=tr, dead=True)) for s in DEAD_SHAPES for tr in (False, True)]
    return cases


def bf16_cases():
    """(label, case) of every bf16 case of this file: the cases TOL is derived from."""
    cases = [(f"eval{s}", rect_case(s)) for s in BF16_EVAL_SHAPES]
    cases += [(f"train{BF16_TRAIN_SHAPE}", rect_case(BF16_TRAIN_SHAPE, train=True)),
              (f"train+maps{BF16_MAP_SHAPE}", rect_case(BF16_MAP_SHAPE, train=True, maps=True)),
              (f"dead{BF16_DEAD_SHAPE}", rect_case(BF16_DEAD_SHAPE, dead="tail")),
              (f"dense train{BF16_DENSE_SHAPE}", rect_dense_case(BF16_DENSE_SHAPE, with_dattn=False))]
    return cases


@pytest.fixture
def rect_tol(monkeypatch):
    """check_sbm / check_dense / check_graph of test_bf16_paths_gpu under this file's constants."""
    monkeypatch.setattr(T, "TOL", TOL)


# ---------------------------------------------------------------------------------------------------------
# fp32 comparison
# ---------------------------------------------------------------------------------------------------------
def check_graph_fp32(c, graph, expA):
    """The GPU's graph equals the oracle's own sampling on its fp64 expA except at fp32 ties (eval: a host uniform
    within 1e-6 of clamp(expA); train: a 16-bit draw within 0.5 of clamp(expA) 65536), in fewer than 1e-4 of the draws.
    A train-mode case that carries host_uniforms (the forward was handed kw["u"]) obeys the eval rule."""
    if c["train"] and not c.get("host_uniforms"):
        want = philox.ste_graph(expA.numpy(), c["u16"])
        thr = np.clip(expA.numpy(), 0.01, 0.99) * 65536.0
        diff = want != graph.numpy().astype(bool)
        assert np.all(np.abs(c["u16"][diff] - thr[diff]) < 0.5), f"{int(diff.sum())} graph flips away from ties"
    else:
        u = c["kw"]["u"].double()
        p = expA.clamp(0.01, 0.99)
        diff = ((u < p) != graph.bool()).numpy()
        assert bool(torch.all((u - p).abs()[torch.from_numpy(diff)] < 1e-6)), f"{int(diff.sum())} graph flips away from fp32 ties"
    assert diff.mean() < 1e-4, f"{int(diff.sum())} of {diff.size} draws differ"


def check_fp32(c, got, label, attn=None):
    """Graph, sparsity, X, dQ / dK / dV and the seven parameter gradients (and the attn map when given) against the
    fp64 closed form on the GPU's graph at 1e-4 / 1e-5, under the ReLU-tie rule. ASTs without a valid key are 0/0 in
    the reference: left out, with their dK / dV exactly zero; parameter gradients only when every AST has one."""
    kw = c["kw"]
    B, H, N, d, k = c["shape"]
    M = kw["K"].shape[2]
    graph = got["graph"]
    assert graph.shape == (B, H, N, M) and got["K"].shape == got["V"].shape == (B, H, M, d)
    assert got["X"].shape == got["Q"].shape == (B, H, N, d)
    live = kw["mask"].sum(1) < M
    np.testing.assert_allclose(got["sparsity"].numpy(), graph.sum((0, 2, 3)).numpy() / (B * N * M), rtol=1e-6)
    assert torch.all(got["K"][~live] == 0) and torch.all(got["V"][~live] == 0)

    def run_oracle(ov):
        return closed_form.sbm_fwd_bwd(**kw, graph_override=graph, relu_override=ov)

    def check(ref, rg):
        check_graph_fp32(c, graph, ref["expA"])
        np.testing.assert_allclose(got["sparsity"].numpy(), ref["sparsity"].numpy(), rtol=1e-6)
        np.testing.assert_allclose(got["X"][live].numpy(), ref["X"][live].numpy(), rtol=RTOL, atol=ATOL, err_msg="X")
        if attn is not None:
            np.testing.assert_allclose(attn[live].numpy(), ref["attn"][live].numpy(), rtol=RTOL, atol=ATOL, err_msg="attn")
        for n in ("Q", "K", "V"):
            np.testing.assert_allclose(got[n][live].numpy(), rg[n][live].numpy(), rtol=RTOL, atol=ATOL, err_msg="d" + n)
        if bool(live.all()):
            for n in PARAM_NAMES:
                np.testing.assert_allclose(got[n].numpy(), rg[n].numpy(), rtol=RTOL, atol=ATOL, err_msg=n)

    nt = _match_oracle_up_to_relu_ties(run_oracle, check)
    print(f"rect {label}: {nt} ReLU tie element(s)")


def _maps(c, bf16=False):
    """(graph, attn) of a forward of the case through torch.ops.csa.sbm_fwd / sbm_maps."""
    kw = c["kw"]
    k = kw["num_clusters"]
    cw, pw, pb = T._weights(kw["params"])
    q, kk, v, mk = (kw[n].float().contiguous().cuda() for n in ("Q", "K", "V", "mask"))
    uu = None if c["train"] else kw["u"].float().cuda()
    _, _, state = torch.ops.csa.sbm_fwd(q, kk, v, mk, cw, pw, pb, uu, k, SEED, OFFSET, c["attn_p"], c["proj_p"], False,
                                        bf16, False)
    graph, attn = torch.ops.csa.sbm_maps(q, kk, v, mk, state, k, False)
    return graph.cpu(), attn.cpu()


def _assert_same(a, b):
    assert a.keys() == b.keys() and len(a) == 13
    for n in a:
        assert torch.equal(a[n], b[n]), n


# ---------------------------------------------------------------------------------------------------------
# SBM, fp32
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EVAL_SHAPES)
def test_rect_shapes_match_oracle(shape):
    """Eval mode through the SBMAttention module (host uniforms, padded keys), forward and backward."""
    c = rect_case(shape)
    kw = c["kw"]
    X, sp, graph, dQ, dK, dV, grads = _run_module(kw["Q"], kw["K"], kw["V"], kw["mask"], kw["u"], kw["dX"],
                                                  kw["dsparsity"], kw["params"], kw["num_clusters"])
    got = {"X": X, "sparsity": sp, "graph": graph, "Q": dQ, "K": dK, "V": dV}
    got.update({n: grads[n] for n in PARAM_NAMES})
    check_fp32(c, got, f"eval{shape}")


@pytest.mark.parametrize("shape", TRAIN_SHAPES)
def test_rect_train_mode_matches_oracle_with_regenerated_masks(shape):
    """Train mode (attn_p 0.2, proj_p 0.1): the attention-dropout and STE streams regenerated over (N, M), the
    projection dropout over N rows for the Q MLP and M rows for the K MLP."""
    c = rect_case(shape, train=True)
    assert 0.75 < c["keep"].mean() < 0.85
    assert all(0.85 < float((t > 0).double().mean()) < 0.95 for t in c["kw"]["proj_keep"].values())
    check_fp32(c, run_sbm_gpu(c, bf16=False), f"train{shape}")


@pytest.mark.parametrize("train", [False, True])
def test_rect_maps_and_map_gradients_match_oracle(train):
    """sbm_maps returns (B, H, N, M) maps; upstream dgraph / dattn of that shape reach k_attn_gx, k_attn_rowprep
    and the DG instantiations of the backward kernels."""
    B, H, N, M, d, k = MAP_SHAPE
    c = rect_case(MAP_SHAPE, train=train, maps=True)
    assert c["kw"]["dgraph"].shape == c["kw"]["dattn"].shape == (B, H, N, M)
    graph, attn = _maps(c)
    got = run_sbm_gpu(c, bf16=False)
    assert attn.shape == (B, H, N, M) and torch.equal(graph, got["graph"])
    check_fp32(c, got, f"maps{MAP_SHAPE} train={train}", attn=attn)
    assert not torch.equal(got["Q"], run_sbm_gpu(c, bf16=False, maps=False)["Q"])  # the map gradients reached dQ


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("shape", DEAD_SHAPES)
def test_rect_dead_key_tiles_match_oracle(shape, train):
    """Fully masked 32-key tiles (the light paths) with NQB != NKB; M = 2080 has 65 key tiles, past the dead-tile
    record, over 2 query blocks. The graph keeps sampled edges at padded keys."""
    c = rect_case(shape, train=train, dead=True)
    got = run_sbm_gpu(c, bf16=False)
    assert float(got["graph"][:, :, :, 64:].sum()) > 0
    check_fp32(c, got, f"dead{shape} train={train}")


@pytest.mark.parametrize("with_dattn", [False, True])
@pytest.mark.parametrize("shape", SCHED_SHAPES)
def test_rect_concurrent_backward_schedule_bit_identical(shape, with_dattn):
    """CSA_SCHED_CONCURRENT against CSA_SCHED_IN_ORDER in train mode where the key-item and query-item workgroup
    groups of k_proj_bwd_s differ in size (G_K != G_Q): every output bitwise equal."""
    c = rect_case(shape, train=True, maps=with_dattn)
    c["kw"].pop("dgraph", None)
    _assert_same(run_sbm_gpu(c, bf16=False, schedule=CSA_SCHED_IN_ORDER),
                 run_sbm_gpu(c, bf16=False, schedule=CSA_SCHED_CONCURRENT))


@pytest.mark.parametrize("train", [False, True])
def test_rect_two_runs_bitwise_identical(train):
    c = rect_case((2, 2, 70, 33, 64, 10), train=train)
    _assert_same(run_sbm_gpu(c, bf16=False), run_sbm_gpu(c, bf16=False))


def test_rect_strided_views_equal_contiguous_run():
    """Q the head-major view of a (B, N, H, d) buffer, K and V the two head-major views of one packed
    (B, M, 2, H, d) buffer: K / V strides differ from Q's, packed_qkv is false, and every output equals the
    contiguous run's bit for bit."""
    from csa_amd import ops
    B, H, N, M, d, k = LAYOUT_SHAPE
    c = rect_case(LAYOUT_SHAPE)
    kw = c["kw"]
    cw, pw, pb = T._weights(kw["params"])
    mk, uu, dX, dsp = (kw[n].cuda() for n in ("mask", "u", "dX", "dsparsity"))
    qbuf = kw["Q"].transpose(1, 2).contiguous().cuda()  # (B, N, H, d)
    kvbuf = torch.stack([kw["K"].transpose(1, 2), kw["V"].transpose(1, 2)], 2).contiguous().cuda()  # (B, M, 2, H, d)
    qv, kv, vv = qbuf.transpose(1, 2), kvbuf[:, :, 0].transpose(1, 2), kvbuf[:, :, 1].transpose(1, 2)
    assert qv.stride() == (N * H * d, d, H * d, 1) and kv.stride() == vv.stride() == (M * 2 * H * d, d, 2 * H * d, 1)
    assert not ops.packed_qkv(qv, kv, vv)
    outs = []
    for q, kk, v in ((qv, kv, vv), tuple(kw[n].cuda() for n in ("Q", "K", "V"))):
        X, sp, state = torch.ops.csa.sbm_fwd(q, kk, v, mk, cw, pw, pb, uu, k, SEED, OFFSET, 0.0, 0.0, False)
        graph, attn = torch.ops.csa.sbm_maps(q, kk, v, mk, state, k, False)
        g = torch.ops.csa.sbm_bwd(q, kk, v, mk, cw, pw, pb, k, 0.0, 0.0, SEED, OFFSET, False, state, X, dX, dsp, None)
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in [X, sp, graph, attn] + list(g)])
    assert len(outs[0]) == len(outs[1]) == 14
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_rect_forward_only_state_gives_the_same_outputs():
    """CSA_FLAG_FWD_ONLY (forward under no_grad): the same X, sparsity and maps as the grad-enabled forward."""
    from csa_amd import ops
    c = rect_case((2, 2, 45, 70, 64, 10))
    kw = c["kw"]
    cw = kw["params"]["layer.weight"].cuda().requires_grad_()
    proj = []
    for i in (0, 3, 6):
        proj += [kw["params"][f"proj.{i}.weight"].cuda().requires_grad_(), kw["params"][f"proj.{i}.bias"].cuda().requires_grad_()]
    q, kk, v, mk, uu = (kw[n].cuda() for n in ("Q", "K", "V", "mask", "u"))
    k = kw["num_clusters"]
    assert not ops._fwd_only(q, cw)
    ref = ops.sbm_attention(q, kk, v, mk, cw, proj, k, uniforms=uu)
    assert ref[2].shape == ref[3].shape == (2, 2, 45, 70)
    for ctx in (torch.no_grad, torch.inference_mode):
        with ctx():
            assert ops._fwd_only(q, cw, *proj)
            got = ops.sbm_attention(q, kk, v, mk, cw, proj, k, uniforms=uu)
        for a, b in zip(ref, got):
            assert torch.equal(a.detach(), b)


# ---------------------------------------------------------------------------------------------------------
# dense, fp32
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", DENSE_SHAPES)
def test_rect_dense_train_mode_with_attn_gradient_matches_oracle(shape):
    c = rect_dense_case(shape)
    got = run_dense_gpu(c, False)
    B, H, N, M, d = shape
    assert got["X"].shape == got["Q"].shape == (B, H, N, d) and got["K"].shape == got["V"].shape == (B, H, M, d)
    check_dense(c, got, False, f"dense{shape}")


# ---------------------------------------------------------------------------------------------------------
# bf16
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BF16_EVAL_SHAPES)
def test_rect_bf16_eval_matches_emulation(shape, rect_tol):
    c = rect_case(shape)
    check_sbm(c, run_sbm_gpu(c), f"rect eval{shape}")


def test_rect_bf16_train_mode_matches_emulation(rect_tol):
    c = rect_case(BF16_TRAIN_SHAPE, train=True)
    check_sbm(c, run_sbm_gpu(c), f"rect train{BF16_TRAIN_SHAPE}")


def test_rect_bf16_train_mode_map_gradients_match_emulation(rect_tol):
    c = rect_case(BF16_MAP_SHAPE, train=True, maps=True)
    got = run_sbm_gpu(c)
    check_sbm(c, got, f"rect train+maps{BF16_MAP_SHAPE}")
    assert not torch.equal(got["Q"], run_sbm_gpu(c, maps=False)["Q"])  # the map gradients reached dQ


def test_rect_bf16_dead_key_tiles_past_the_dead_tile_record(rect_tol):
    c = rect_case(BF16_DEAD_SHAPE, dead="tail")
    check_sbm(c, run_sbm_gpu(c), f"rect dead{BF16_DEAD_SHAPE}")


def test_rect_bf16_dense_train_mode_matches_emulation(rect_tol):
    c = rect_dense_case(BF16_DENSE_SHAPE, with_dattn=False)
    check_dense(c, run_dense_gpu(c, True), True, f"rect dense{BF16_DENSE_SHAPE}")
