"""GPU parity of the CSE relation attention (csrc/csa_rel.hip) away from the production shape: relation vocabulary
L, AST length N, head size d_k, batch splits of the dlq / dlk reduction, plane layouts and bf16 mode, each against
the fp64 oracle (oracle/cse_ref.py under autograd) on seeded random inputs.

Inputs (make_inputs): relation codes uniform over [0, L) -- every bin, at every N, so also on the merged-prep
N <= 256 path -- with the last AST of the batch carrying a quarter of code 0 and a quarter of code L - 1 (the
clamp ends of collate_relations); Bernoulli(0.3) masks that are asymmetric and hold, per AST and plane, a fully
masked query row (uniform attention over all N keys), a row with a single unmasked key (softmax = 1: dq of that
row is 0 in exact arithmetic; the oracle's value is asserted < 1e-8 and the row is compared at the plain
tolerance) and a fully masked key column.

What the cases reach (the derived values follow make_rel / rel_layout / csa_rel_attn_fwd in csa_rel.hip):

A. L sweep, fused fp32 (d = 64, H = 2, compact, B = 2, N = 70: three key tiles, the last partial). ng = ceil(L/8)
   is the number of K groups of both bins_times (32-row kernels, bf16 mode: KB2 = 4 ng, chunks of RING = 4 groups
   then ng % 4 leftover ones) and bins_times16 (16-row kernels, fp32: Q4 = 2 ng, chunks of RING = 8 then ng % 8
   leftover); NW = ceil(L/32) is k_rel_lgrad's waves per workgroup, which share the 8 DMA pieces of a chunk
   (q = lt; q < 8; q += NW), and k_rel_logits' l-tiles.
       L    KB2  ng  32-row chunks+left  16-row chunks+left  NW  note
       1      4   1        0+1                0+1             1   L = 32k+1; clamped l-tile (imin(l, L-1))
       7      4   1        0+1                0+1             1   Lp = 8 > L
       8      4   1        0+1                0+1             1
       9      8   2        0+2                0+2             1
       24    12   3        0+3                0+3             1   no whole chunk (ng <= 3)
       32    16   4        4+0                0+4             1   multiple of 32, ng multiple of 4
       33    20   5        4+1                0+5             2   L = 32k+1
       44    24   6        4+2                0+6             2
       56    28   7        4+3                0+7             2
       96    48  12       12+0                8+4             3   NW = 3: waves take 3, 3, 2 pieces
       100   52  13       12+1                8+5             4
       128   64  16       16+0               16+0             4   multiple of 32, no leftover group
       136   68  17       16+1               16+1             5
       150   76  19       16+3               16+3             5   (the production L)
       200  100  25       24+1               24+1             7
       255  128  32       32+0               32+0             8
       256  128  32       32+0               32+0             8   code 255 used
   LB = 2 KB2 + 4 for every L: 2 KB2 / 4 = 2 ceil(L/8) is always even, so make_rel's "+ 4 so that LB / 4 is odd"
   is taken at every L, L = 150 included, and the other arm cannot be reached; there is one LB class, not two.
   test_l_sweep_covers_every_class asserts the classes above from the same formulas.
B. N edges, fused fp32 (d = 64, L = 150, B = 1): N = 1 (one query, one key), 31 / 32 / 33 / 64 (no partial tile
   at 32 and 64), 255 / 256 (merged prep: the 32-row items ride in the k_rel_logits launch, 16 KB of LDS at 256),
   257 (first separate k_rel_prep launch), 1024 (last k_rel_prep, 64 KB of dynamic LDS) and 1025 (first
   k_rel_prep_t), 37 and 23 (rel_prep_item's byte staging: a 32-row block whose byte count is no multiple of 4).
   N = 1024 / 1025 run one head with a (B,1,N,N) plane (the compact layout needs two head halves).
C. k_rel_lgrad's 3-deep chunk ring (d = 64, L = 150): splits of exactly 3 chunks (B = 24, N = 100), 3 and 4
   (B = 20, N = 150), 5 and 6 (B = 44, N = 100, one head with a (B,1,N,N) plane); the chunk counts are asserted
   from rel_layout's formula.
D. Unfused path: d = 16 / 32 / 96 (k_rel_fwd<D>, k_rel_bwd_q<D>, k_bgemm, k_rel_scatter) at N = 1 / 32 / 37 / 70,
   L = 5 / 150 / 256, B = 1 / 3 / 17 (RS = 16 splits 17 elements as 1 and 2), compact and reference layouts.
E. Layouts: per-head planes that differ (P_ = H = 4) at d = 64 and d = 32; compact with H = 2 (two planes, one
   head each) and H = 4 (group = 2); q / k / v as views of one packed (B,N,3,H,64) tensor (the packed-gradient
   return). P_ = 1 (rel_sh == 0, one plane for all heads) cannot be reached through rel_ops: _planes makes the
   planes contiguous and accepts 2 or H of them, and csa_torch.cpp passes their strides, so a (B,1,N,N) plane
   arrives with rel_sh = N * N and H = 1 (P_ = H). test_rel_attn_shared_plane_abi reaches that arm of make_rel /
   prep_row through the C ABI with ctypes (H = 2, d = 64 and d = 32).
F. bf16 mode (the only user of the 32-row kernels k_rel_bwd_qf / k_rel_bwd_kf and bins_scatter / bins_times /
   bins_store_t): L = 8 / 33 / 44 / 128 / 150 / 256 at the bf16 rule of tests/test_bf16_gpu.py, and not bit-equal
   to fp32.

Every fp32 case runs twice and must repeat bitwise (the bins add in a fixed order).

Tolerances: out / dq / dk / dv at the suite's RTOL, ATOL = 1e-4, 1e-5; dlq / dlk at the population rule
atol = ATOL max(1, max|ref| / 100) of tests/test_cse_gpu.py. The float32 oracle alone (cse_ref.rel_attn in float32
on the CPU against itself in float64) stays below 0.09 of that bound on every output of every case (the table
above the case lists, per case the largest element-wise err / (RTOL |ref| + atol)); the bar for a case to be
usable is 0.5. The GPU kernels measured at most 0.03 (out), 0.13 (dq), 0.12 (dk), 0.05 (dv), 0.19 (dlq) and
0.12 (dlk) of the bound over all cases; each test prints its six ratios before it asserts.
"""
import collections
import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu
from test_bf16_gpu import close_bf16

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]
RTOL, ATOL = 1e-4, 1e-5
NAMES = ("out", "dq", "dk", "dv", "dlq", "dlk")

Case = collections.namedtuple("Case", "B H N d L seed layout packed", defaults=(False,))


def _heads_of_plane(H, nplanes, pl):
    """Heads that read base plane pl: all layouts but per_head share plane 0 / 1 between the head halves."""
    if nplanes == 1:
        return list(range(H))
    if nplanes == H:
        return [pl]
    return list(range(pl * (H // 2), (pl + 1) * (H // 2)))


def make_inputs(B, H, N, d, L, seed, layout):
    """q, k, v, dO (B,H,N,d), lq, lk (1,H,L,d), the rel / mask planes in `layout` as rel_ops.rel_attn takes them,
    the (B,H,N,N) int64 / bool planes the oracle takes, and the (AST, heads, row) of every single-key row."""
    from oracle import cse_ref
    g = torch.Generator().manual_seed(seed)
    q, k, v, dO = (torch.randn(B, H, N, d, generator=g) for _ in range(4))
    lq, lk = (torch.randn(1, H, L, d, generator=g) for _ in range(2))
    P = H if layout == "per_head" else 1 if layout == "shared" else 2
    rel = torch.randint(0, L, (B, P, N, N), generator=g, dtype=torch.int64)
    u = torch.rand(P, N, N, generator=g)  # the last AST: a quarter of each clamp end
    rel[B - 1][u < 0.25] = 0
    rel[B - 1][u > 0.75] = L - 1
    mask = torch.rand(B, P, N, N, generator=g) < 0.3
    single = []
    if N >= 4:
        for b in range(B):
            for pl in range(P):
                r0, r1 = (int(x) for x in torch.randperm(N, generator=g)[:2])
                c0, c1 = (int(x) for x in torch.randperm(N, generator=g)[:2])
                mask[b, pl, :, c0] = True   # a fully masked key column
                mask[b, pl, r0, :] = True   # a fully masked query row
                mask[b, pl, r1, :] = True   # a row with the single unmasked key c1 != c0
                mask[b, pl, r1, c1] = False
                single.append((b, _heads_of_plane(H, P, pl), r1))
                assert bool((mask[b, pl] != mask[b, pl].T).any()), "mask must be asymmetric"
    if layout == "per_head":
        orel, omask = rel, mask
        grel, gmask = rel.clone(), mask.clone()
    elif layout == "shared":  # one (B,1,N,N) plane for every head (C ABI only: head stride 0)
        orel, omask = rel.expand(B, H, N, N), mask.expand(B, H, N, N)
        grel, gmask = rel.to(torch.uint8), mask.to(torch.uint8)
    else:
        r8, m8 = cse_ref.build_rel_mask(rel[:, 0], rel[:, 1], mask[:, 0], mask[:, 1])
        heads = [0] * (H // 2) + [4] * (H // 2)  # build_rel_mask repeats each plane 4x: keep H / 2 of each
        orel, omask = r8[:, heads].contiguous(), m8[:, heads].contiguous()
        if layout == "compact":
            grel, gmask = rel.to(torch.uint8), mask.to(torch.uint8)
        else:
            assert layout == "reference"
            grel, gmask = orel.clone(), omask.clone()
    assert N < 4 or (int(rel.max()) == L - 1 and int(rel.min()) == 0)
    return (q, k, v, dO, lq, lk), (grel, gmask), (orel, omask), single


def oracle(inp, orel, omask, dtype=torch.float64):
    """[out, dq, dk, dv, dlq, dlk] of cse_ref.rel_attn under autograd at `dtype`, as float64 numpy arrays."""
    from oracle import cse_ref
    q, k, v, dO, lq, lk = inp
    t = [x.to(dtype).requires_grad_(True) for x in (q, k, v, lq, lk)]
    o = cse_ref.rel_attn(*t, orel, omask)
    (o * dO.to(dtype)).sum().backward()
    return [o.detach().double().numpy()] + [x.grad.double().numpy() for x in t]


@functools.lru_cache(maxsize=None)
def reference(c):
    """Inputs and fp64 oracle of one case, computed once and shared (read-only)."""
    inp, gplanes, (orel, omask), single = make_inputs(c.B, c.H, c.N, c.d, c.L, c.seed, c.layout)
    ref = oracle(inp, orel, omask)
    for b, heads, r1 in single:  # softmax = 1 on the single key: dq of the row vanishes in exact arithmetic
        assert np.abs(ref[1][b, heads, r1]).max() < 1e-8
    return inp, gplanes, ref


def atol_of(i, ref):
    return ATOL * max(1.0, float(np.abs(ref).max()) / 100) if i >= 4 else ATOL


def ratios(got, ref):
    """Per output, the largest element-wise err / (RTOL |ref| + atol): <= 1 passes assert_allclose."""
    return [float((np.abs(np.asarray(g, np.float64) - r) / (RTOL * np.abs(r) + atol_of(i, r))).max())
            for i, (g, r) in enumerate(zip(got, ref))]


def run_gpu(c, inp, gplanes, bf16=False):
    from csa_amd import rel_ops
    from csa_amd.ops import packed_qkv
    q, k, v, dO, lq, lk = inp
    rel, mask = (x.cuda() for x in gplanes)
    lqd, lkd = (x.cuda().requires_grad_(True) for x in (lq, lk))
    if c.packed:  # q, k, v: the head-major views of one (B,N,3,H,d) projection output
        pk = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).contiguous().cuda().requires_grad_(True)
        qd, kd, vd = (pk[:, :, i].transpose(1, 2) for i in range(3))
        assert packed_qkv(qd, kd, vd)
    else:
        qd, kd, vd = (x.cuda().requires_grad_(True) for x in (q, k, v))
    o = rel_ops.rel_attn(qd, kd, vd, lqd, lkd, rel, mask, bf16=bf16)
    (o * dO.cuda()).sum().backward()
    torch.cuda.synchronize()
    if c.packed:
        grads = [pk.grad[:, :, i].transpose(1, 2).contiguous().cpu() for i in range(3)]
    else:
        grads = [x.grad.cpu() for x in (qd, kd, vd)]
    return [o.detach().cpu()] + grads + [lqd.grad.cpu(), lkd.grad.cpu()]


def run_abi_shared(c, inp, gplanes):
    """csa_rel_attn_fwd / csa_rel_attn_bwd through ctypes with rel_sh = mask_sh = 0: one plane per AST read by
    every head (make_rel's P_ = 1), contiguous tensors (zero stride triples), in-order schedule."""
    import ctypes
    from csa_amd import _lib
    lib = _lib.lib()
    q, k, v, dO, lq, lk = (x.contiguous().cuda() for x in inp)
    rel, mask = (x.contiguous().cuda() for x in gplanes)
    B, H, N, d = q.shape
    L = lq.shape[-2]
    assert rel.shape == mask.shape == (B, 1, N, N) and rel.dtype == mask.dtype == torch.uint8
    new = lambda *s: torch.empty(*s, device="cuda")
    raw = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")
    out, stats, state = new(B, H, N, d), new(B, H, N, 2), raw(lib.csa_rel_attn_state_bytes(B, H, N, L, d))
    dq, dk, dv, dlq, dlk = new(B, H, N, d), new(B, H, N, d), new(B, H, N, d), new(H, L, d), new(H, L, d)
    ws = raw(lib.csa_rel_attn_bwd_workspace_bytes(B, H, N, L, d))
    a = _lib.RelAttnArgs(B=B, H=H, N=N, L=L, d=d, lq=lq.data_ptr(), lk=lk.data_ptr(),
                         rel=rel.data_ptr(), rel_sb=N * N, rel_sh=0, mask=mask.data_ptr(), mask_sb=N * N, mask_sh=0,
                         rel_head_group=0, dtype=_lib.CSA_DTYPE_F32, out=out.data_ptr(), row_stats=stats.data_ptr(),
                         state=state.data_ptr())
    for n, t in (("q", q), ("k", k), ("v", v)):
        setattr(a, n, t.data_ptr())
        for s, x in zip(("sb", "sh", "sn"), t.stride()):
            setattr(a, f"{n}_{s}", x)
    b = _lib.RelAttnBwdArgs(fwd=ctypes.pointer(a), dout=dO.data_ptr(), dq=dq.data_ptr(), dk=dk.data_ptr(),
                            dv=dv.data_ptr(), dlq=dlq.data_ptr(), dlk=dlk.data_ptr(), workspace=ws.data_ptr(),
                            schedule=_lib.CSA_SCHED_IN_ORDER)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.csa_rel_attn_fwd(ctypes.byref(a), stream), "csa_rel_attn_fwd")
    _lib.check(lib.csa_rel_attn_bwd(ctypes.byref(b), stream), "csa_rel_attn_bwd")
    torch.cuda.synchronize()
    return [out.cpu(), dq.cpu(), dk.cpu(), dv.cpu(), dlq.cpu().unsqueeze(0), dlk.cpu().unsqueeze(0)]


def check_fp32(c, run=run_gpu):
    inp, gplanes, ref = reference(c)
    r1 = run(c, inp, gplanes)
    r2 = run(c, inp, gplanes)
    got = [x.numpy() for x in r1]
    print("ratios", c, " ".join(f"{n}={x:.3f}" for n, x in zip(NAMES, ratios(got, ref))))
    for n, a, b in zip(NAMES, r1, r2):
        assert torch.equal(a, b), f"{n}: two runs differ"
    for i, n in enumerate(NAMES):
        np.testing.assert_allclose(got[i], ref[i], rtol=RTOL, atol=atol_of(i, ref[i]), err_msg=n)


def cid(c):
    return f"B{c.B}-H{c.H}-N{c.N}-d{c.d}-L{c.L}-{c.layout}" + ("-packed" if c.packed else "")


# The float32 oracle alone: cse_ref.rel_attn in float32 on the CPU against itself in float64, per case and output
# the largest element-wise err / (RTOL |ref| + atol) with the atol each output is tested at (the bf16 cases F reuse
# the inputs of A). Every entry must stay below 0.5 for the case to be kept.
#   group case                                       out     dq     dk     dv    dlq    dlk
#   A     B2-H2-N70-d64-L1-compact                 0.027  0.019  0.026  0.023  0.061  0.043
#   A     B2-H2-N70-d64-L7-compact                 0.026  0.015  0.017  0.026  0.030  0.021
#   A     B2-H2-N70-d64-L8-compact                 0.016  0.014  0.019  0.015  0.041  0.022
#   A     B2-H2-N70-d64-L9-compact                 0.015  0.015  0.023  0.031  0.028  0.044
#   A     B2-H2-N70-d64-L24-compact                0.019  0.017  0.022  0.019  0.027  0.022
#   A     B2-H2-N70-d64-L32-compact                0.017  0.016  0.020  0.018  0.021  0.021
#   A     B2-H2-N70-d64-L33-compact                0.023  0.017  0.023  0.018  0.019  0.022
#   A     B2-H2-N70-d64-L44-compact                0.023  0.017  0.021  0.024  0.041  0.022
#   A     B2-H2-N70-d64-L56-compact                0.019  0.015  0.019  0.018  0.019  0.028
#   A     B2-H2-N70-d64-L96-compact                0.017  0.015  0.016  0.018  0.016  0.018
#   A     B2-H2-N70-d64-L100-compact               0.021  0.016  0.019  0.022  0.032  0.021
#   A     B2-H2-N70-d64-L128-compact               0.020  0.017  0.022  0.018  0.024  0.018
#   A     B2-H2-N70-d64-L136-compact               0.021  0.018  0.019  0.016  0.014  0.020
#   A     B2-H2-N70-d64-L150-compact               0.021  0.016  0.018  0.016  0.016  0.021
#   A     B2-H2-N70-d64-L200-compact               0.018  0.016  0.018  0.028  0.018  0.016
#   A     B2-H2-N70-d64-L255-compact               0.015  0.018  0.021  0.028  0.031  0.019
#   A     B2-H2-N70-d64-L256-compact               0.017  0.021  0.019  0.016  0.019  0.018
#   B     B1-H2-N1-d64-L150-compact                0.000  0.000  0.000  0.000  0.000  0.000
#   B     B1-H2-N31-d64-L150-compact               0.045  0.010  0.019  0.014  0.013  0.010
#   B     B1-H2-N32-d64-L150-compact               0.015  0.018  0.014  0.013  0.021  0.018
#   B     B1-H2-N33-d64-L150-compact               0.019  0.014  0.012  0.016  0.022  0.019
#   B     B1-H2-N64-d64-L150-compact               0.019  0.014  0.016  0.018  0.020  0.024
#   B     B1-H2-N255-d64-L150-compact              0.013  0.015  0.016  0.018  0.028  0.024
#   B     B1-H2-N256-d64-L150-compact              0.013  0.013  0.017  0.014  0.024  0.032
#   B     B1-H2-N257-d64-L150-compact              0.014  0.017  0.012  0.016  0.022  0.019
#   B     B1-H2-N37-d64-L150-compact               0.022  0.014  0.014  0.022  0.023  0.017
#   B     B1-H2-N23-d64-L150-compact               0.018  0.025  0.028  0.019  0.017  0.017
#   B     B1-H1-N1024-d64-L150-per_head            0.012  0.010  0.009  0.013  0.031  0.038
#   B     B1-H1-N1025-d64-L150-per_head            0.011  0.011  0.012  0.011  0.038  0.035
#   C     B24-H2-N100-d64-L150-compact             0.032  0.023  0.024  0.024  0.049  0.038
#   C     B20-H2-N150-d64-L150-compact             0.025  0.030  0.019  0.029  0.036  0.032
#   C     B44-H1-N100-d64-L150-per_head            0.034  0.030  0.028  0.029  0.045  0.051
#   D     B1-H2-N37-d16-L150-compact               0.009  0.007  0.011  0.011  0.008  0.011
#   D     B3-H2-N37-d32-L150-reference             0.017  0.012  0.014  0.017  0.013  0.012
#   D     B1-H2-N37-d96-L150-compact               0.031  0.018  0.015  0.027  0.015  0.015
#   D     B1-H2-N70-d32-L5-compact                 0.013  0.011  0.015  0.016  0.015  0.015
#   D     B3-H2-N32-d96-L5-reference               0.024  0.019  0.020  0.033  0.034  0.032
#   D     B1-H2-N32-d32-L256-reference             0.015  0.009  0.016  0.013  0.009  0.010
#   D     B1-H2-N70-d96-L256-compact               0.023  0.016  0.020  0.028  0.020  0.021
#   D     B1-H2-N70-d16-L256-reference             0.008  0.007  0.009  0.011  0.013  0.013
#   D     B3-H2-N32-d16-L5-compact                 0.011  0.016  0.014  0.014  0.020  0.017
#   D     B3-H2-N1-d16-L150-reference              0.000  0.000  0.000  0.000  0.000  0.000
#   D     B1-H2-N1-d32-L150-compact                0.000  0.000  0.000  0.000  0.000  0.000
#   D     B1-H2-N1-d96-L5-compact                  0.000  0.000  0.000  0.000  0.000  0.000
#   D     B17-H2-N37-d16-L150-compact              0.016  0.013  0.017  0.016  0.015  0.017
#   D     B17-H2-N32-d32-L256-reference            0.021  0.024  0.026  0.019  0.013  0.018
#   D     B17-H2-N70-d96-L5-reference              0.031  0.032  0.027  0.027  0.089  0.066
#   E     B2-H4-N70-d64-L150-per_head              0.017  0.022  0.036  0.022  0.023  0.018
#   E     B2-H4-N70-d32-L150-per_head              0.017  0.014  0.016  0.015  0.017  0.015
#   E     B2-H2-N70-d64-L150-compact               0.019  0.020  0.019  0.020  0.024  0.015
#   E     B2-H4-N70-d64-L150-compact               0.031  0.015  0.017  0.024  0.025  0.025
#   E     B2-H4-N70-d64-L150-compact-packed        0.028  0.019  0.021  0.024  0.030  0.025
#   E     B2-H2-N70-d64-L150-shared                0.045  0.019  0.024  0.028  0.013  0.020
#   E     B2-H2-N70-d32-L150-shared                0.018  0.010  0.012  0.018  0.016  0.012
#   max                                            0.045  0.032  0.036  0.033  0.089  0.066
L_SWEEP = (1, 7, 8, 9, 24, 32, 33, 44, 56, 96, 100, 128, 136, 150, 200, 255, 256)
CASES_A = [Case(2, 2, 70, 64, L, 100 + L, "compact") for L in L_SWEEP]
CASES_B = ([Case(1, 2, N, 64, 150, 200 + N, "compact") for N in (1, 31, 32, 33, 64, 255, 256, 257, 37, 23)]
           + [Case(1, 1, N, 64, 150, 200 + N, "per_head") for N in (1024, 1025)])
CASES_C = [(Case(24, 2, 100, 64, 150, 301, "compact"), {3}),
           (Case(20, 2, 150, 64, 150, 302, "compact"), {3, 4}),
           (Case(44, 1, 100, 64, 150, 303, "per_head"), {5, 6})]
CASES_D = [Case(B, 2, N, d, L, 400 + i, layout) for i, (d, N, L, B, layout) in enumerate([
    (16, 37, 150, 1, "compact"), (32, 37, 150, 3, "reference"), (96, 37, 150, 1, "compact"),
    (32, 70, 5, 1, "compact"), (96, 32, 5, 3, "reference"), (32, 32, 256, 1, "reference"),
    (96, 70, 256, 1, "compact"), (16, 70, 256, 1, "reference"), (16, 32, 5, 3, "compact"),
    (16, 1, 150, 3, "reference"), (32, 1, 150, 1, "compact"), (96, 1, 5, 1, "compact"),
    (16, 37, 150, 17, "compact"), (32, 32, 256, 17, "reference"), (96, 70, 5, 17, "reference")])]
CASES_E = [Case(2, 4, 70, 64, 150, 501, "per_head"), Case(2, 4, 70, 32, 150, 502, "per_head"),
           Case(2, 2, 70, 64, 150, 503, "compact"), Case(2, 4, 70, 64, 150, 504, "compact"),
           Case(2, 4, 70, 64, 150, 505, "compact", True)]
CASES_E_ABI = [Case(2, 2, 70, 64, 150, 506, "shared"), Case(2, 2, 70, 32, 150, 507, "shared")]
L_BF16 = (8, 33, 44, 128, 150, 256)
CASES_F = [c for c in CASES_A if c.L in L_BF16]
GROUPS = {"A": CASES_A, "B": CASES_B, "C": [c for c, _ in CASES_C], "D": CASES_D, "E": CASES_E + CASES_E_ABI,
          "F": CASES_F}


def test_l_sweep_covers_every_class():
    """The L lists reach every class of the tables in the module docstring (formulas of make_rel, bins_times,
    bins_times16 and rel_param_grads)."""
    ng = {L: (L + 7) // 8 for L in L_SWEEP}
    for L in L_SWEEP:
        KB2 = 4 * ng[L]
        assert (2 * KB2 // 4) % 2 == 0  # make_rel's LB "+ 4" at every L: the other arm is unreachable
    assert any(n <= 3 for n in ng.values()) and any(n % 4 == 0 for n in ng.values())
    assert {n % 4 for n in ng.values() if n >= 4} == {0, 1, 2, 3}    # 32-row leftovers after a whole chunk
    assert {n % 4 for n in ng.values() if n < 4} == {1, 2, 3}        # 32-row: no whole chunk
    assert {n % 8 for n in ng.values() if n < 8} == set(range(1, 8))  # 16-row: no whole chunk
    assert {0, 1, 4, 5} <= {n % 8 for n in ng.values() if n >= 8}    # 16-row leftovers after a whole chunk
    assert {1, 2, 3, 4, 5, 7, 8} <= {(L + 31) // 32 for L in L_SWEEP}  # k_rel_lgrad waves / logits l-tiles
    assert any(L % 32 == 0 for L in L_SWEEP) and any(L % 32 == 1 and L > 32 for L in L_SWEEP)
    ngb = {L: (L + 7) // 8 for L in L_BF16}  # what actually runs the 32-row kernels
    assert {n % 4 for n in ngb.values() if n >= 4} == {0, 1, 2, 3} and any(n < 4 for n in ngb.values())


@pytest.mark.parametrize("c", CASES_A, ids=cid)
def test_rel_attn_l_sweep(c):
    """A: relation vocabulary L from 1 to 256 on the fused fp32 path (classes: module docstring, table A)."""
    check_fp32(c)


@pytest.mark.parametrize("c", CASES_B, ids=cid)
def test_rel_attn_n_edges(c):
    """B: AST length N at the tile and prep-path boundaries. Prep path by N: <= 256 merged into k_rel_logits
    (rel_prep_lds_bytes(N) <= 16384), 257 .. 1024 k_rel_prep (<= 65536), above k_rel_prep_t."""
    lds = 2 * ((32 * c.N + 15) // 16 * 16)
    path = "merged" if lds <= 16384 else "prep" if lds <= 65536 else "prep_t"
    assert path == {1024: "prep", 1025: "prep_t", 257: "prep"}.get(c.N, "merged")
    if c.N in (37, 23):  # rel_prep_item stages a block byte-wise when its byte count is no multiple of 4
        assert any((min(32, c.N - a0) * c.N) & 3 for a0 in range(0, c.N, 32))
    check_fp32(c)


@pytest.mark.parametrize("c,chunks", CASES_C, ids=lambda x: cid(x) if isinstance(x, Case) else None)
def test_rel_attn_lgrad_ring(c, chunks):
    """C: k_rel_lgrad splits of 3, 3 / 4 and 5 / 6 chunks (the 3-deep register ring takes its third step, re-enters
    the loop and leaves at each position). Chunks per split as rel_layout and k_rel_lgrad derive them."""
    NP = (c.N + 31) // 32 * 32
    nch = c.B * NP // 32
    RS = min(32, nch)
    assert {(s + 1) * nch // RS - s * nch // RS for s in range(RS)} == chunks
    check_fp32(c)


@pytest.mark.parametrize("c", CASES_D, ids=cid)
def test_rel_attn_unfused(c):
    """D: the generic path at d_k = 16 / 32 / 96; B = 17 splits the dlq / dlk batch sum (RS = 16) into parts of
    one and two elements."""
    if c.B == 17:
        assert {(s + 1) * c.B // 16 - s * c.B // 16 for s in range(16)} == {1, 2}
    check_fp32(c)


@pytest.mark.parametrize("c", CASES_E, ids=cid)
def test_rel_attn_layouts(c):
    """E: per-head planes that differ (P_ = H), compact planes with H = 2 and H = 4, packed q / k / v."""
    if c.layout == "per_head":
        rel = reference(c)[1][0]
        assert all(not torch.equal(rel[:, 0], rel[:, h]) for h in range(1, c.H))
    check_fp32(c)


@pytest.mark.parametrize("c", CASES_E_ABI, ids=cid)
def test_rel_attn_shared_plane_abi(c):
    """E: one plane for every head (rel_sh = mask_sh = 0: P_ = 1 in the fused path, head stride 0 in the generic
    one). rel_ops cannot express it (see the module docstring), so the C ABI is called through ctypes."""
    check_fp32(c, run_abi_shared)


@pytest.mark.parametrize("c", CASES_F, ids=cid)
def test_rel_attn_bf16_l_sweep(c):
    """F: bf16 mode (32-row kernels: bins_scatter / bins_times / bins_store_t with LB / KB2) over L, at the bf16
    rule of tests/test_bf16_gpu.py against the fp64 oracle; the result differs from the fp32 one."""
    inp, gplanes, ref = reference(c)
    r16 = run_gpu(c, inp, gplanes, bf16=True)
    r32 = run_gpu(c, inp, gplanes)
    for n, a, b in zip(NAMES, r16, r32):
        assert not torch.equal(a, b), f"{n}: bf16 result is bit-equal to fp32"
    for n, a, r in zip(NAMES, r16, ref):
        print("bf16", cid(c), n, f"fro={close_bf16(a.numpy(), r, n):.4f}")
