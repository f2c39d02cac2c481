"""The CSE relation attention through the C ABI with every caller-owned buffer guarded and poisoned: the checks of
tests/test_sbm_abi_guard_gpu.py for csa_rel_attn_fwd / csa_rel_attn_bwd (csrc/csa_rel.hip).

out, row_stats, the state, dq, dk, dv, dlq, dlk and the workspace are carved from tests/abi_arena.Arena at exactly the
byte counts csa_rel_attn_state_bytes / csa_rel_attn_bwd_workspace_bytes return; the calls go through ctypes on the
current stream, as test_cse_shapes_gpu.run_abi_shared does for one layout. Per case:

  G  after fwd and after bwd no guard byte and no stride-gap element has changed (the prepared planes RM / RT / RB
     and the gt tiles are sized for NP = 32 ceil(N / 32) rows, out / dq / dk / dv / row_stats and the logit tables for N);
  P  two runs, state / workspace / outputs prefilled 0x00 and 0xFF, give bitwise equal out, row_stats, dq, dk, dv, dlq,
     dlk (a gt / RB tile or a gc2p / gp2ct bin its producer skipped would differ);
  W  in the 0xFF run every addressed element of those seven was written and is finite;
  I  q, k, v, lq, lk, the planes and dout are bitwise what was passed in;
  A  out, dq, dk, dv, dlq, dlk are bitwise those of rel_ops.rel_attn under autograd on the same inputs (the shared plane
     expanded to one identical plane per head, which rel_ops can express).

Inputs: test_cse_shapes_gpu.make_inputs (asymmetric masks with a fully masked row, a single-key row and a masked
column per plane; every relation code used). Cases, B <= 2:

  group    d    N                    L                      forms
  fused    64   70 (merged prep),    150                    fp32 and bf16 x shared plane (H = 2, rel_sh = mask_sh = 0)
                257 (k_rel_prep)                            and two planes (H = 8, rel_head_group = 4) x contiguous
                                                            (zero stride triples) and head-major out / dq / dk / dv /
                                                            dout, rows pitched d + 4: views of (B,N,H,d+4) buffers
                                                            whose gap elements are guards
  tile     64   1040, B = 1          150                    k_rel_prep_t (N > 1024): shared plane, fp32 and bf16
  l-sweep  64   70                   L_SWEEP (fp32),        every class of test_l_sweep_covers_every_class (bins K
                                     L_BF16 (bf16)          groups, chunk leftovers, k_rel_lgrad waves), shared plane
  generic  16, 32, 96   37           150                    k_rel_fwd<D>, k_bgemm, k_rel_scatter: shared and two planes

Every N has a ragged last tile. Bodies of out / dq / dk / dv are 16-byte and not 256-byte aligned."""
import collections
import ctypes

import pytest
import torch

from abi_arena import GUARD, POISON_ONES, POISON_ZERO, Arena
from conftest import has_gpu
from csa_amd import _lib
from test_cse_shapes_gpu import L_BF16, L_SWEEP, make_inputs
from test_sbm_abi_guard_gpu import same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]
NAMES = ("out", "dq", "dk", "dv", "dlq", "dlk")

# the source lines of csrc/csa_rel.hip the case list relies on: the fused / generic split, the three prep paths by N,
# the plane forms, and which buffers are sized for padded rows
REL_LINES = ("R.fused = (d == 64);",
             "inline size_t rel_prep_lds_bytes(int64_t N) { return 2 * (size_t)((32 * N + 15) / 16 * 16); }",
             "const bool merged = prep_lds <= 16384;",
             "} else if (prep_lds <= 65536) {",
             "p.P_ = a->rel_head_group > 0 ? 2 : (a->rel_sh == 0 && a->mask_sh == 0 ? 1 : (int)a->H);",
             "R.NP = ((N + 31) / 32) * 32;",
             "R.c2p = take(sizeof(float) * B * H * N * R.Lp);",
             "R.RB = take(R.fused ? sizeof(float) * B * H * R.NP * R.NP : 0);  // tile-major relation bias",
             "R.gc2p = take(R.fused ? sizeof(float) * H * B * R.Lp * R.ldx : sizeof(float) * B * H * N * R.Lp);",
             "R.qstat = take(R.fused ? sizeof(float) * B * H * N * 4 : 0);",
             "R.gt = take(R.fused ? sizeof(float) * B * H * R.NP * R.NP : 0);",
             "if (a->dtype == CSA_DTYPE_BF16 && a->d != 64) return rfail(CSA_UNSUPPORTED_SHAPE, \"bf16 CSE needs d_k = 64\");",
             "if (a->d != 64 && !contig3(a->o_sb, a->o_sh, a->o_sn, a->H, a->N, a->d))")

CSpec = collections.namedtuple("CSpec", "group B H N d L seed form bf16 layout", defaults=(False, "contig"))
FORMS = {"shared": 2, "two_plane": 8}  # heads of the form


def prep_path(N):
    lds = 2 * ((32 * N + 15) // 16 * 16)
    return "merged" if lds <= 16384 else "prep" if lds <= 65536 else "prep_t"


def guard_specs():
    s, seed = [], 600
    for N in (70, 257):
        for form, H in FORMS.items():
            for bf16 in (False, True):
                for layout in ("contig", "head_major"):
                    seed += 1
                    s.append(CSpec("fused", 2 if N == 70 or form == "shared" else 1, H, N, 64, 150, seed, form, bf16, layout))
    s += [CSpec("tile", 1, 2, 1040, 64, 150, 640 + bf16, "shared", bool(bf16)) for bf16 in (0, 1)]
    s += [CSpec("l-sweep", 2, 2, 70, 64, L, 700 + L, "shared") for L in L_SWEEP]
    s += [CSpec("l-sweep", 2, 2, 70, 64, L, 700 + L, "shared", True) for L in L_BF16]
    s += [CSpec("generic", 2 if form == "shared" else 1, H, 37, d, 150, 800 + d + H, form)
          for d in (16, 32, 96) for form, H in FORMS.items()]
    return s


def spec_id(s):
    return f"{s.group}-B{s.B}-H{s.H}-N{s.N}-d{s.d}-L{s.L}-{s.form}-{'bf16' if s.bf16 else 'fp32'}-{s.layout}"


def assert_specs_cover_every_path():
    """What the module docstring's table promises (tests/test_abi_arena_cpu.py runs this without a GPU)."""
    S = guard_specs()
    assert len({spec_id(s) for s in S}) == len(S) and all(s.B <= 2 and s.N % 32 for s in S)
    fused = [s for s in S if s.group == "fused"]
    assert {(prep_path(s.N), s.form, s.bf16, s.layout) for s in fused} == {
        (p, f, b, l) for p in ("merged", "prep") for f in FORMS for b in (False, True) for l in ("contig", "head_major")}
    assert {(prep_path(s.N), s.bf16) for s in S if s.group == "tile"} == {("prep_t", False), ("prep_t", True)}
    assert all(prep_path(s.N) == "merged" for s in S if s.group in ("l-sweep", "generic"))
    assert [s.L for s in S if s.group == "l-sweep" and not s.bf16] == list(L_SWEEP)
    assert [s.L for s in S if s.group == "l-sweep" and s.bf16] == list(L_BF16)
    assert {(s.d, s.form) for s in S if s.group == "generic"} == {(d, f) for d in (16, 32, 96) for f in FORMS}
    assert all(s.d == 64 for s in S if s.bf16 or s.layout != "contig")
    assert all(s.H == FORMS[s.form] for s in S)


def build_inputs(s):
    """Device tensors of a case: q, k, v, dout (B,H,N,d), lq, lk (H,L,d), the uint8 planes; head_major: q / k / v /
    dout stay contiguous, only the library's outputs are strided (dout too: its (B,N,H,d) memory)."""
    layout = "shared" if s.form == "shared" else "compact"
    (q, k, v, dO, lq, lk), (rel, mask), _, _ = make_inputs(s.B, s.H, s.N, s.d, s.L, s.seed, layout)
    assert rel.shape == mask.shape == (s.B, 1 if s.form == "shared" else 2, s.N, s.N) and rel.dtype == torch.uint8
    inp = {n: t.contiguous().cuda() for n, t in (("q", q), ("k", k), ("v", v), ("lq", lq[0]), ("lk", lk[0]),
                                                  ("rel", rel), ("mask", mask))}
    inp["dout"] = (dO.transpose(1, 2).contiguous().cuda().transpose(1, 2) if s.layout == "head_major"
                   else dO.contiguous().cuda())
    return inp


def run_anchor(s, inp):
    from csa_amd import rel_ops
    t = [inp[n].clone().requires_grad_(True) for n in ("q", "k", "v", "lq", "lk")]
    rel, mask = inp["rel"], inp["mask"]
    if s.form == "shared":  # one identical plane per head: P_ = H with the same bytes
        rel, mask = (x.expand(s.B, s.H, s.N, s.N).contiguous() for x in (rel, mask))
    o = rel_ops.rel_attn(*t, rel, mask, bf16=s.bf16, schedule="in_order")
    o.backward(inp["dout"])
    torch.cuda.synchronize()
    return dict(zip(NAMES, [o.detach().cpu().contiguous()] + [x.grad.cpu().contiguous() for x in t]))


def _strides(a, prefix, t):
    for n, x in zip(("sb", "sh", "sn"), t.stride()):
        setattr(a, f"{prefix}_{n}", x)


def run_abi(s, inp, poison):
    L = _lib.lib()
    B, H, N, d, Lr = s.B, s.H, s.N, s.d, s.L
    state_bytes = L.csa_rel_attn_state_bytes(B, H, N, Lr, d)
    ws_bytes = L.csa_rel_attn_bwd_workspace_bytes(B, H, N, Lr, d)
    host = {n: t.cpu().clone() for n, t in inp.items()}
    payload = state_bytes + ws_bytes + 4 * (4 * B * H * N * (d + 4) + 2 * B * H * N + 2 * H * Lr * d)
    ar = Arena("cuda", capacity=payload + 16 * (2 * GUARD + 1024), poison=poison)

    def rows(name):
        if s.layout == "head_major":
            return ar.carve(name, shape=(B, N, H, d + 4), align=16, views=lambda t: t[..., :d].transpose(1, 2))
        return ar.carve(name, shape=(B, H, N, d), align=16)

    out = {"out": rows("out"), "row_stats": ar.carve("row_stats", shape=(B, H, N, 2))}
    state = ar.carve("state", nbytes=state_bytes)
    out.update({n: rows(n) for n in ("dq", "dk", "dv")})
    out.update({n: ar.carve(n, shape=(H, Lr, d)) for n in ("dlq", "dlk")})
    ws = ar.carve("workspace", nbytes=ws_bytes)
    assert ar.address_mod("state") == 0 and ar.address_mod("out") == 16

    P = inp["rel"].shape[1]
    a = _lib.RelAttnArgs(B=B, H=H, N=N, L=Lr, d=d, lq=inp["lq"].data_ptr(), lk=inp["lk"].data_ptr(),
                         rel=inp["rel"].data_ptr(), rel_sb=P * N * N, rel_sh=0 if P == 1 else N * N,
                         mask=inp["mask"].data_ptr(), mask_sb=P * N * N, mask_sh=0 if P == 1 else N * N,
                         rel_head_group=0 if P == 1 else H // 2,
                         dtype=_lib.CSA_DTYPE_BF16 if s.bf16 else _lib.CSA_DTYPE_F32,
                         out=out["out"].data_ptr(), row_stats=out["row_stats"].data_ptr(), state=state.data_ptr())
    for n in ("q", "k", "v"):
        setattr(a, n, inp[n].data_ptr())
        _strides(a, n, inp[n])
    b = _lib.RelAttnBwdArgs(fwd=ctypes.pointer(a), dout=inp["dout"].data_ptr(), dq=out["dq"].data_ptr(),
                            dk=out["dk"].data_ptr(), dv=out["dv"].data_ptr(), dlq=out["dlq"].data_ptr(),
                            dlk=out["dlk"].data_ptr(), workspace=ws.data_ptr(), schedule=_lib.CSA_SCHED_IN_ORDER)
    if s.layout == "head_major":  # contiguous: every stride triple stays zero
        _strides(a, "o", out["out"])
        _strides(b, "do", inp["dout"])
        for n in ("dq", "dk", "dv"):
            _strides(b, n, out[n])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    what = spec_id(s)
    _lib.check(L.csa_rel_attn_fwd(ctypes.byref(a), stream), "csa_rel_attn_fwd")
    ar.assert_guards_intact(f"{what}: after fwd")
    _lib.check(L.csa_rel_attn_bwd(ctypes.byref(b), stream), "csa_rel_attn_bwd")
    ar.assert_guards_intact(f"{what}: after bwd")
    torch.cuda.synchronize()
    if poison == POISON_ONES:
        for n, t in out.items():
            ar.assert_written(t, f"{what}: {n}")
    for n, t in inp.items():
        ok = torch.equal(t.cpu(), host[n]) if t.dtype == torch.uint8 else same_bits(t, host[n])
        assert ok, f"{what}: input {n} was written"
    return {n: t.cpu().contiguous() for n, t in out.items()}


@pytest.mark.parametrize("s", guard_specs(), ids=spec_id)
def test_rel_attn_abi_buffers_guards_poison_written_inputs_anchor(s):
    inp = build_inputs(s)
    zero, ones = run_abi(s, inp, POISON_ZERO), run_abi(s, inp, POISON_ONES)
    assert zero.keys() == ones.keys() and len(ones) == 7
    for n in ones:  # P
        assert same_bits(zero[n], ones[n]), f"{spec_id(s)}: {n} depends on what state / workspace / outputs held before"
    anchor = run_anchor(s, inp)
    for n in NAMES:  # A
        assert same_bits(ones[n], anchor[n]), f"{spec_id(s)}: {n} differs from rel_ops.rel_attn on the same inputs"
