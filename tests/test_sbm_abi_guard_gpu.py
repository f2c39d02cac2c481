"""SBM and dense attention through the C ABI with every caller-owned buffer guarded and poisoned.

include/csa_hip.h: "the caller allocates every output, the saved state and the workspace (sizes from the *_bytes()
queries)". The op shim allocates them with at::empty, so in training they sit beside live activations and start out
holding whatever their previous owner left. Every other SBM / dense test compares output values only; this file
checks the buffer contract itself. csa_sbm_fwd, csa_sbm_maps (graph and attn) and csa_sbm_bwd (dense cases:
csa_dense_attn_fwd / _bwd) run through ctypes on the current stream with X, sparsity, the state, the maps, dQ / dK / dV,
dcluster_w, the three dproj_w and dproj_b and the workspace carved from tests/abi_arena.Arena at exactly the byte
counts csa_sbm_state_bytes / csa_sbm_bwd_workspace_bytes return. Per case:

  G  guards      after fwd, after maps and after bwd no guard byte and no stride-gap element has changed: a store to
                 a padded row (Qh, Kh, T, stats, w_dQh, w_dT, X, dQ / dK / dV are sized for N and M rows, not NQB * 32 /
                 NKB * 32), past a CSA_FLAG_FWD_ONLY state without its Act segment, or into the gap of a strided row
                 lands there.
  P  poison      the whole sequence runs twice, state / workspace / outputs prefilled 0x00 and 0xFF (every fp32 word a
                 NaN, every Abits word all edges), same seed, offset and uniforms: the 13 outputs and the attn map are
                 bitwise equal. A kernel that reads a tile its producer skipped (dead-tile handoff, slabs, w_gx
                 without map gradients, padded w_brow rows, the no-edge plane) differs.
  W  written     in the 0xFF run no addressed output element is still poison, and every one is finite.
  I  inputs      Q, K, V, mask, weights, uniforms, dX, dsparsity, dgraph, dattn are bitwise what was passed in.
  A  anchor      the outputs are bitwise those of torch.ops.csa.sbm_fwd / _maps / _bwd (the oracle-checked path) on
                 the same inputs, seed and offset: the same kernels, and layout does not change bits
                 (test_rect_strided_views_equal_contiguous_run). No second tolerance.

Inputs come from test_sbm_rect_gpu.rect_case / rect_dense_case and test_sbm_wide_gpu.host_uniform_case (seed =
sum(shape)); no random-input code is added here. Cases (B, H, N, M, d, k), ragged last tiles on both sides (M = 2080
is 65 whole key tiles):

  group        classes / shapes                                                    what it adds
  class        A B C D E F (CLASS_SHAPES), eval and train (attn_p 0.2, proj_p 0.1)   every launch class; dgraph / dattn
                                                                                     NULL: w_gx never written or read
  rng          A, E: eval with Philox draws, train with host uniforms               the other HAS_U form of k_attn_fwd
  maps         A, C with dgraph and dattn, eval and train                           k_attn_rowprep, w_gx, both planes
  dead         (6,2,40,150,64,10), (2,1,40,2080,64,10), eval and train              dead key tiles; past the record
  fwd-only     A, B, C, E with the CSA_FLAG_FWD_ONLY state, eval and train          fwd + maps only: G, P, and X /
                                                                                     sparsity / maps bitwise the full run
  dense        (2,2,45,70,64), (1,2,100,1,96), with and without dattn, train        csa_dense_attn_fwd / _bwd
  bf16         A, E, dense (2,2,45,70,64); train; workspace with / without           CSA_DTYPE_BF16, CSA_FLAG_BF16_WS
               CSA_FLAG_BF16_WS
  layout       A: X / dX head-major (B,N,H,d); dQ / dK / dV views of a packed        strided stores, gaps are guards
               (B,N,3,H,d) (N = M = 45); X / dQ / dK / dV with row pitch d + 4
  concurrent   A, E, train: side stream + two events made with torch               CSA_SCHED_CONCURRENT = in-order bits
  twice        A, train with map gradients: backward again on the same forward      retain_graph: workspace and outputs
               state (and a third time, back on the arena's own poison)             refilled with the other poison byte

Buffers default to (B,H,R,d) contiguous with the zero stride triple (the shim always passes head-major X and explicit
strides, so that ABI form runs nowhere else); X / dQ / dK / dV bodies are 16-byte aligned and NOT 256-byte aligned,
state and workspace 256-byte aligned as the allocator hands them out. tests/test_abi_arena_cpu.py proves without a
GPU that the arena reports each kind of stray store and unwritten element, and pins the dispatch lines the case
lists rely on."""
import collections
import ctypes

import pytest
import torch

from abi_arena import GUARD, POISON_ONES, POISON_ZERO, Arena
from conftest import has_gpu
from csa_amd import _lib
from test_bf16_paths_gpu import OFFSET, PARAM_NAMES, SEED
from test_sbm_rect_gpu import rect_case, rect_dense_case
from test_sbm_wide_gpu import host_uniform_case, launch_class

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]

CLASS_SHAPES = {"A": (2, 2, 45, 70, 64, 10), "B": (2, 3, 45, 45, 64, 20), "C": (2, 2, 45, 70, 64, 40),
                "D": (1, 2, 70, 33, 64, 100), "E": (2, 2, 45, 70, 96, 10), "F": (1, 2, 70, 33, 96, 32)}
DEAD_SHAPES = [(6, 2, 40, 150, 64, 10), (2, 1, 40, 2080, 64, 10)]  # the second: 65 key tiles, past TDEAD_TILES
DENSE_SHAPES = [(2, 2, 45, 70, 64), (1, 2, 100, 1, 96)]
PACKED_SHAPE = (2, 2, 45, 45, 64, 10)  # class A with N == M: one packed (B,N,3,H,d) gradient
FWD_ONLY_CLASSES = "ABCE"

# the source lines of csrc/csa_sbm.hip the lists above rely on beside test_sbm_wide_gpu.DISPATCH_LINES: which buffers
# are sized for N / M rows, what CSA_FLAG_FWD_ONLY and CSA_FLAG_BF16_WS drop, and the dead-tile record
LAYOUT_LINES = ("L.NQB = (N + 31) / 32; L.NKB = (M + 31) / 32; L.Mpad = L.NKB * 32;",
                "L.Qh = take(sizeof(float) * B * H * N * L.kp);",
                "L.Kh = take(sizeof(float) * B * H * M * L.kp);",
                "L.T = take(sizeof(float) * B * H * M * L.kp);",
                "L.stats = take(sizeof(float) * B * H * N * 4);",
                "L.Act = take(sizeof(float) * ((dense || (flags & CSA_FLAG_FWD_ONLY)) ? 0 : B * H * (L.NQB + L.NKB) * (3 * D + KP32) * 32));",
                "L.total = o;",
                "L.w_dQh = take(sizeof(float) * B * H * N * L.kp);",
                "L.w_dT = take(sizeof(float) * B * H * M * L.kp);",
                "L.w_gx = take(sizeof(float) * B * H * N);  // used only when an attn-map gradient is passed",
                "L.w_dsg = take(sizeof(float) * ((flags & CSA_FLAG_BF16_WS) ? 0 : L.w_dsg_plane * (dense ? 1 : 2)));",
                "L.w_brow = take(sizeof(float) * B * H * L.NQB * 32 * 4);",
                "constexpr int TDEAD_TILES = 64;",
                "p.Act = (a->flags & CSA_FLAG_FWD_ONLY) ? nullptr : (float*)((char*)st + L.Act);")

Spec = collections.namedtuple(
    "Spec", "group kind shape train maps dead rng bf16 bf16_ws fwd_only layout schedule twice",
    defaults=("sbm", None, False, False, False, "default", False, True, False, "contig", "in_order", False))


def _spec(group, shape, **kw):
    return Spec(group=group, shape=shape, **kw)


def guard_specs():
    s = []
    for cls, shape in CLASS_SHAPES.items():
        s += [_spec("class", shape, train=tr) for tr in (False, True)]
    for cls in "AE":  # eval mode draws from Philox, train mode from the caller's uniforms
        s += [_spec("rng", CLASS_SHAPES[cls], train=False, rng="philox"), _spec("rng", CLASS_SHAPES[cls], train=True, rng="host")]
    for cls in "AC":
        s += [_spec("maps", CLASS_SHAPES[cls], train=tr, maps=True) for tr in (False, True)]
    s += [_spec("dead", shape, train=tr, dead=True) for shape in DEAD_SHAPES for tr in (False, True)]
    s += [_spec("fwd-only", CLASS_SHAPES[cls], train=tr, fwd_only=True) for cls in FWD_ONLY_CLASSES for tr in (False, True)]
    s += [_spec("dense", shape, kind="dense", train=True, maps=da) for shape in DENSE_SHAPES for da in (False, True)]
    for ws in (True, False):
        s += [_spec("bf16", CLASS_SHAPES[cls], train=True, bf16=True, bf16_ws=ws) for cls in "AE"]
        s += [_spec("bf16", DENSE_SHAPES[0], kind="dense", train=True, maps=True, bf16=True, bf16_ws=ws)]
    s += [_spec("layout", CLASS_SHAPES["A"], train=True, layout="head_major"),
          _spec("layout", PACKED_SHAPE, train=True, layout="packed"),
          _spec("layout", CLASS_SHAPES["A"], train=True, layout="pitch")]
    s += [_spec("concurrent", CLASS_SHAPES[cls], train=True, schedule="concurrent") for cls in "AE"]
    s += [_spec("twice", CLASS_SHAPES["A"], train=True, maps=True, twice=True)]
    return s


def spec_id(s):
    bits = [s.group, "x".join(str(v) for v in s.shape), "train" if s.train else "eval"]
    bits += [n for n, on in (("maps", s.maps and s.group != "maps"), ("bf16ws" if s.bf16_ws else "fullws", s.bf16)) if on]
    bits += [v for v in (s.rng, s.layout, s.schedule) if v not in ("default", "contig", "in_order")]
    return "-".join(bits)


def assert_specs_cover_every_class_and_path():
    """What the module docstring's table promises, from the lists themselves (tests/test_abi_arena_cpu.py runs this
    without a GPU, beside the source-line pins)."""
    S = guard_specs()
    assert len({spec_id(s) for s in S}) == len(S)
    cls = lambda s: launch_class(s.shape[4], s.shape[5])
    assert [cls(Spec("x", "sbm", sh)) for sh in CLASS_SHAPES.values()] == list("ABCDEF") == list(CLASS_SHAPES)
    for sh in list(CLASS_SHAPES.values()) + DEAD_SHAPES[:1]:  # ragged last tiles on both sides
        assert sh[2] % 32 and sh[3] % 32, sh
    assert DEAD_SHAPES[1][2] % 32 and DEAD_SHAPES[1][3] == 65 * 32  # 65 whole key tiles under a ragged query tile
    sbm = [s for s in S if s.kind == "sbm"]
    for c in "ABCDEF":
        assert {s.train for s in sbm if s.group == "class" and cls(s) == c} == {False, True}, c
    assert {(cls(s), s.train, s.rng) for s in sbm if s.group == "rng"} == {(c, False, "philox") for c in "AE"} | {(c, True, "host") for c in "AE"}
    assert {(cls(s), s.train) for s in sbm if s.group == "maps"} == {(c, t) for c in "AC" for t in (False, True)}
    dead = [s for s in sbm if s.dead]
    assert {s.shape for s in dead} == set(DEAD_SHAPES) and all({t.train for t in dead if t.shape == s.shape} == {False, True} for s in dead)
    assert DEAD_SHAPES[0][0] >= 6 and (DEAD_SHAPES[0][3] + 31) // 32 <= 64 < (DEAD_SHAPES[1][3] + 31) // 32
    assert {(cls(s), s.train) for s in sbm if s.fwd_only} == {(c, t) for c in FWD_ONLY_CLASSES for t in (False, True)}
    dense = [s for s in S if s.kind == "dense" and not s.bf16]
    assert {(s.shape, s.maps) for s in dense} == {(sh, m) for sh in DENSE_SHAPES for m in (False, True)} and all(s.train for s in dense)
    assert {s.shape[4] for s in dense} == {64, 96}
    b16 = [s for s in S if s.bf16]
    assert {(s.kind, s.shape[4], s.bf16_ws) for s in b16} == {(k, d, w) for k, d in (("sbm", 64), ("sbm", 96), ("dense", 64)) for w in (False, True)}
    assert all(s.train and (s.kind == "dense" or cls(s) in "AE") for s in b16)
    assert [s.layout for s in S if s.group == "layout"] == ["head_major", "packed", "pitch"]
    assert all(cls(s) == "A" for s in S if s.group == "layout") and PACKED_SHAPE[2] == PACKED_SHAPE[3]
    assert {cls(s) for s in S if s.schedule == "concurrent"} == {"A", "E"} and sum(s.twice for s in S) == 1


def build_case(s):
    if s.kind == "dense":
        return rect_dense_case(s.shape, with_dattn=s.maps)
    if s.rng == "host":
        return host_uniform_case(s.shape)
    return rect_case(s.shape, train=s.train, maps=s.maps, dead=s.dead)


# ---------------------------------------------------------------------------------------------------------
# device inputs (shared by the ABI run and the anchor)
# ---------------------------------------------------------------------------------------------------------
def device_inputs(s, c):
    """name -> CUDA tensor of everything the calls read; dX is the (B,H,N,d) view the layout asks for."""
    kw = c["kw"]
    f = lambda t: t.float().contiguous().cuda()
    inp = {n: f(kw[n]) for n in ("Q", "K", "V", "mask")}
    if s.kind == "sbm":
        inp["cw"] = f(kw["params"]["layer.weight"])
        for i, l in enumerate((0, 3, 6)):
            inp[f"pw{i}"], inp[f"pb{i}"] = f(kw["params"][f"proj.{l}.weight"]), f(kw["params"][f"proj.{l}.bias"])
        host_u = (not s.train and s.rng != "philox") or s.rng == "host"
        if host_u:
            inp["u"] = f(kw["u"])
        inp["dsparsity"] = f(kw["dsparsity"])
        if s.maps:
            inp["dgraph"] = f(kw["dgraph"])
    if s.maps:
        inp["dattn"] = f(kw["dattn"])
    if s.layout == "head_major":
        inp["dX"] = kw["dX"].float().transpose(1, 2).contiguous().cuda().transpose(1, 2)  # (B,N,H,d) memory
    else:
        inp["dX"] = f(kw["dX"])
    return inp


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------
# the anchor: the op shim on the same inputs
# ---------------------------------------------------------------------------------------------------------
def run_shim(s, c, inp):
    dense = s.kind == "dense"
    k = 0 if dense else c["kw"]["num_clusters"]
    cw = inp.get("cw")
    pw, pb = ([inp[f"p{x}{i}"] for i in range(3)] for x in "wb") if not dense else ([], [])
    q, kk, v, mk = (inp[n] for n in ("Q", "K", "V", "mask"))
    proj_p = 0.0 if dense else c["proj_p"]
    X, sp, state = torch.ops.csa.sbm_fwd(q, kk, v, mk, cw, pw, pb, inp.get("u"), k, SEED, OFFSET, c["attn_p"], proj_p,
                                         dense, s.bf16, s.fwd_only)
    graph, attn = torch.ops.csa.sbm_maps(q, kk, v, mk, state, k, dense)
    got = {"X": X, "graph": graph, "attn": attn}
    if not dense:
        got["sparsity"] = sp
    if not s.fwd_only:
        g = torch.ops.csa.sbm_bwd(q, kk, v, mk, cw, pw, pb, k, c["attn_p"], proj_p, SEED, OFFSET, dense, state, X,
                                  inp["dX"], inp.get("dsparsity"), inp.get("dgraph"), s.bf16, False, inp.get("dattn"),
                                  _lib.CSA_SCHED_IN_ORDER)
        got.update(dict(zip(["Q", "K", "V"] + ([] if dense else PARAM_NAMES), g)))
    torch.cuda.synchronize()
    return {n: t.cpu().contiguous() for n, t in got.items()}


# ---------------------------------------------------------------------------------------------------------
# the ABI run
# ---------------------------------------------------------------------------------------------------------
def _strides(a, prefix, t):
    for n, x in zip(("sb", "sh", "sn"), t.stride()):
        setattr(a, f"{prefix}_{n}", x)


def run_abi(s, c, inp, poison):
    """fwd, maps and (unless fwd_only) bwd with every writable buffer carved from an arena poisoned `poison`; asserts
    G after each call, W in the 0xFF run and I at the end; returns the outputs on the CPU. s.twice: a second backward
    on the same state with the workspace and the outputs refilled with the other poison byte must give the same bits."""
    L = _lib.lib()
    dense = s.kind == "dense"
    B, H, N, d = c["kw"]["Q"].shape
    M = c["kw"]["K"].shape[2]
    k = 0 if dense else c["kw"]["num_clusters"]
    size_flags = (_lib.CSA_FLAG_DENSE if dense else 0) | (_lib.CSA_FLAG_FWD_ONLY if s.fwd_only else 0)
    state_bytes = L.csa_sbm_state_bytes(B, H, N, M, d, k, size_flags)
    ws_bytes = L.csa_sbm_bwd_workspace_bytes(B, H, N, M, d, k, (_lib.CSA_FLAG_DENSE if dense else 0)
                                             | (_lib.CSA_FLAG_BF16_WS if s.bf16 and s.bf16_ws else 0))
    if s.fwd_only:
        assert state_bytes < L.csa_sbm_state_bytes(B, H, N, M, d, k, 0)
    if s.bf16:
        full = L.csa_sbm_bwd_workspace_bytes(B, H, N, M, d, k, _lib.CSA_FLAG_DENSE if dense else 0)
        assert (ws_bytes < full) if s.bf16_ws else (ws_bytes == full)
    host = {n: t.cpu().clone() for n, t in inp.items()}
    pitch = d + 4
    payload = state_bytes + ws_bytes + 4 * (2 * B * H * N * M + 3 * B * H * (N + 2 * M) * pitch + 4 * d * d + H * (k + 1) * d)
    ar = Arena("cuda", capacity=payload + 32 * (2 * GUARD + 1024), poison=poison)

    def rows(name, R):  # a (B,H,R,d) output in the case's layout: (view, pass explicit strides?)
        if s.layout == "pitch":
            return ar.carve(name, shape=(B, H, R, pitch), align=16, views=lambda t: t[..., :d]), True
        if s.layout == "head_major" and name == "X":
            return ar.carve(name, shape=(B, R, H, d), align=16, views=lambda t: t.transpose(1, 2)), True
        return ar.carve(name, shape=(B, H, R, d), align=16), s.layout == "head_major"

    out = {}
    out["X"], x_strided = rows("X", N)
    if not dense:
        out["sparsity"] = ar.carve("sparsity", shape=(H,))
    state = ar.carve("state", nbytes=state_bytes)
    out["graph"], out["attn"] = ar.carve("graph", shape=(B, H, N, M)), ar.carve("attn", shape=(B, H, N, M))
    bwd_names = []
    if not s.fwd_only:
        if s.layout == "packed":
            assert N == M
            out["Q"], out["K"], out["V"] = ar.carve("dQKV", shape=(B, N, 3, H, d), align=16,
                                                    views=lambda t: tuple(t[:, :, i].transpose(1, 2) for i in range(3)))
            g_strided = True
            bwd_names.append("dQKV")
        else:
            (out["Q"], g_strided), (out["K"], _), (out["V"], _) = rows("dQ", N), rows("dK", M), rows("dV", M)
            bwd_names += ["dQ", "dK", "dV"]
        if not dense:
            out["layer.weight"] = ar.carve("dcluster_w", shape=(H * k, d))
            for i, l in enumerate((0, 3, 6)):
                out[f"proj.{l}.weight"] = ar.carve(f"dproj_w{i}", shape=(d, d))
                out[f"proj.{l}.bias"] = ar.carve(f"dproj_b{i}", shape=(d,))
            bwd_names += ["dcluster_w"] + [f"dproj_{x}{i}" for x in "wb" for i in range(3)]
        ws = ar.carve("workspace", nbytes=ws_bytes)
        bwd_names.append("workspace")
    assert ar.address_mod("state") == 0 and ar.address_mod("X") == 16 and ar.address_mod("X", 16) == 0

    a = _lib.SbmFwdArgs(B=B, H=H, N=N, M=M, d=d, k=k, key_mask=inp["mask"].data_ptr(), mask_sb=inp["mask"].stride(0),
                        seed=SEED, offset=OFFSET, attn_dropout=c["attn_p"], proj_dropout=0.0 if dense else c["proj_p"],
                        flags=_lib.CSA_FLAG_FWD_ONLY if s.fwd_only else 0,  # the dense entry points force CSA_FLAG_DENSE
                        dtype=_lib.CSA_DTYPE_BF16 if s.bf16 else _lib.CSA_DTYPE_F32,
                        X=out["X"].data_ptr(), state=state.data_ptr())
    for n, t in (("q", inp["Q"]), ("k", inp["K"]), ("v", inp["V"])):
        setattr(a, n.upper(), t.data_ptr())
        _strides(a, n, t)
    if x_strided:
        _strides(a, "x", out["X"])
    if not dense:
        a.cluster_w, a.sparsity = inp["cw"].data_ptr(), out["sparsity"].data_ptr()
        a.proj_w = (_lib.vp * 3)(*(inp[f"pw{i}"].data_ptr() for i in range(3)))
        a.proj_b = (_lib.vp * 3)(*(inp[f"pb{i}"].data_ptr() for i in range(3)))
        if "u" in inp:
            a.uniforms = inp["u"].data_ptr()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    what = spec_id(s)
    _lib.check((L.csa_dense_attn_fwd if dense else L.csa_sbm_fwd)(ctypes.byref(a), stream), "fwd")
    ar.assert_guards_intact(f"{what}: after fwd")
    am = _lib.SbmFwdArgs.from_buffer_copy(a)
    if dense:  # there is no dense maps entry point: the flag is the caller's
        am.flags |= _lib.CSA_FLAG_DENSE
    _lib.check(L.csa_sbm_maps(ctypes.byref(am), ctypes.c_void_p(out["graph"].data_ptr()),
                              ctypes.c_void_p(out["attn"].data_ptr()), stream), "csa_sbm_maps")
    ar.assert_guards_intact(f"{what}: after maps")

    if not s.fwd_only:
        b = _lib.SbmBwdArgs(fwd=ctypes.pointer(a), dX=inp["dX"].data_ptr(), dQ=out["Q"].data_ptr(), dK=out["K"].data_ptr(),
                            dV=out["V"].data_ptr(), workspace=ws.data_ptr(), schedule=_lib.SCHEDULES[s.schedule])
        _strides(b, "dx", inp["dX"])
        if g_strided:
            for n in "QKV":
                _strides(b, "d" + n.lower(), out[n])
        if "dattn" in inp:
            b.dattn = inp["dattn"].data_ptr()
        if not dense:
            b.dsparsity = inp["dsparsity"].data_ptr()
            if "dgraph" in inp:
                b.dgraph = inp["dgraph"].data_ptr()
            b.dcluster_w = out["layer.weight"].data_ptr()
            b.dproj_w = (_lib.vp * 3)(*(out[f"proj.{l}.weight"].data_ptr() for l in (0, 3, 6)))
            b.dproj_b = (_lib.vp * 3)(*(out[f"proj.{l}.bias"].data_ptr() for l in (0, 3, 6)))
        lane = None
        if s.schedule == "concurrent":  # the caller's side lane: a stream and two timing-free events, made by torch
            lane = (torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event())
            lane[1].record()
            lane[2].record()  # a torch event exists once it has been recorded
            b.side_stream, b.side_fork, b.side_join = lane[0].cuda_stream, lane[1].cuda_event, lane[2].cuda_event
            assert b.side_stream and b.side_fork and b.side_join
        bwd = L.csa_dense_attn_bwd if dense else L.csa_sbm_bwd
        _lib.check(bwd(ctypes.byref(b), stream), "bwd")
        ar.assert_guards_intact(f"{what}: after bwd")
        if s.twice:
            first = {n: out[n].cpu().clone() for n in ["Q", "K", "V"] + PARAM_NAMES}
            for n in bwd_names:
                ar.fill(n, POISON_ZERO if poison == POISON_ONES else POISON_ONES)
            _lib.check(bwd(ctypes.byref(b), stream), "second bwd")
            ar.assert_guards_intact(f"{what}: after the second bwd")
            for n, t in first.items():
                assert same_bits(out[n], t), f"{what}: {n} of the second backward on one forward state differs"
            for n in bwd_names:
                ar.fill(n, poison)
            _lib.check(bwd(ctypes.byref(b), stream), "third bwd")
            ar.assert_guards_intact(f"{what}: after the third bwd")
    torch.cuda.synchronize()
    if poison == POISON_ONES:
        for n, t in out.items():
            ar.assert_written(t, f"{what}: {n}")
    for n, t in inp.items():
        assert same_bits(t, host[n]), f"{what}: input {n} was written"
    return {n: t.cpu().contiguous() for n, t in out.items()}


def check_spec(s):
    c = build_case(s)
    inp = device_inputs(s, c)
    zero, ones = run_abi(s, c, inp, POISON_ZERO), run_abi(s, c, inp, POISON_ONES)
    want = 4 if s.fwd_only else 14 if s.kind == "sbm" else 6
    assert zero.keys() == ones.keys() and len(ones) == want
    for n in ones:  # P
        assert same_bits(zero[n], ones[n]), f"{spec_id(s)}: {n} depends on what state / workspace / outputs held before"
    anchor = run_shim(s._replace(fwd_only=False), c, inp)  # A (fwd-only: X, sparsity and the maps of the full-state run)
    for n in ones:
        assert same_bits(ones[n], anchor[n]), f"{spec_id(s)}: {n} differs from torch.ops.csa.* on the same inputs"
    return ones


@pytest.mark.parametrize("s", guard_specs(), ids=spec_id)
def test_sbm_abi_buffers_guards_poison_written_inputs_anchor(s):
    got = check_spec(s)
    if s.train and s.kind == "sbm":
        assert 0 < float(got["graph"].mean()) < 1
    if s.dead:
        assert float(got["graph"][:, :, :, 64:].sum()) > 0  # sampled edges at padded keys: the dead tiles ran


def test_sbm_abi_forward_only_state_is_the_full_state_minus_act():
    """The CSA_FLAG_FWD_ONLY run above is anchored to the full-state run; here the ABI's own full-state forward gives
    the same X, sparsity and maps bit for bit in class B (k_proj_fwd_l off the W16 path)."""
    s = _spec("fwd-only", CLASS_SHAPES["B"], train=True, fwd_only=True)
    c = build_case(s)
    inp = device_inputs(s, c)
    full = run_abi(s._replace(fwd_only=False), c, inp, POISON_ONES)
    only = run_abi(s, c, inp, POISON_ONES)
    for n in only:
        assert same_bits(only[n], full[n]), n
