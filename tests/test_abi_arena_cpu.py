"""The would-fail proof of tests/abi_arena.py, on CPU tensors with plain torch writes, and the source-line pins of the
case lists of tests/test_sbm_abi_guard_gpu.py and tests/test_cse_abi_guard_gpu.py. No GPU needed.

A guard test is only worth something if a stray store, a gap store and a skipped element are each reported; here a
"kernel" is a torch assignment through an oversized alias of the arena, so every detection is exercised one element
at a time: one element before a body, one past it, one in a stride gap (pitched rows, head-major pitched rows, the
planes of a packed buffer), one addressed element left unwritten, one written NaN, and the clean write that passes."""
import os

import pytest
import torch

import test_cse_abi_guard_gpu as cse_guard
import test_sbm_abi_guard_gpu as sbm_guard
from abi_arena import GUARD, GUARD_FILL, POISON_ONES, POISON_ZERO, Arena, GuardError
from conftest import PKG
from test_sbm_wide_gpu import DISPATCH_LINES

B, H, R, d = 2, 3, 5, 8


def _alias(ar, body, before, n):
    """float32 alias of the arena that starts `before` elements in front of `body` and holds n elements: what a kernel
    with a wrong bound addresses."""
    off = body.data_ptr() - ar.base - 4 * before
    return ar.buf[off:off + 4 * n].view(torch.float32)


def _keep(box, t):
    """Remembers the container of a strided carve (the first call: the second one marks the mask alias)."""
    box.setdefault("c", t)
    return t


def test_clean_writes_pass_and_bodies_are_where_they_should_be():
    for poison in (POISON_ZERO, POISON_ONES):
        ar = Arena("cpu", capacity=1 << 20, poison=poison)
        x = ar.carve("x", shape=(B, H, R, d), align=16)
        st = ar.carve("state", nbytes=1000)
        y = ar.carve("y", shape=(B, H, R, d + 4), align=16, views=lambda t: t[..., :d])
        p = ar.carve("packed", shape=(B, R, 3, H, d), views=lambda t: tuple(t[:, :, i].transpose(1, 2) for i in range(3)))
        assert ar.address_mod("x") == 16 and ar.address_mod("y") == 16 and ar.address_mod("state") == 0
        assert st.dtype == torch.uint8 and st.numel() == 1000 and bool((st == poison).all())
        assert x.shape == y.shape == p[0].shape == (B, H, R, d) and y.stride() == (H * R * (d + 4), R * (d + 4), d + 4, 1)
        assert bool((x.view(torch.int32) == (-1 if poison == POISON_ONES else 0)).all())
        ar.assert_guards_intact("fresh")
        if poison == POISON_ONES:
            for t in (x, y) + p:
                with pytest.raises(GuardError, match="never written"):
                    ar.assert_written(t, "t")
        for i, t in enumerate((x, y) + p):
            t.copy_(torch.randn(B, H, R, d) + i)
        st.fill_(7)
        ar.assert_guards_intact("after clean writes")
        for t in (x, y, st) + p:
            ar.assert_written(t, "t")
        assert not torch.equal(p[0], p[1])  # the three planes of the packed buffer are separate elements


@pytest.mark.parametrize("side", ["before", "past"])
@pytest.mark.parametrize("kind", ["typed", "bytes"])
def test_one_element_outside_a_body_is_reported(kind, side):
    ar = Arena("cpu", capacity=1 << 20)
    ar.carve("left", shape=(7,))
    body = ar.carve("mid", shape=(B, H, R, d), align=16) if kind == "typed" else ar.carve("mid", nbytes=4 * 250)
    ar.carve("right", shape=(7,))
    n = body.numel() if kind == "typed" else 250
    w = _alias(ar, body, 1, n + 2)
    w[1:n + 1] = 1.0  # the clean write
    ar.assert_guards_intact("clean")
    w[0 if side == "before" else n + 1] = 1.0
    off = -4 if side == "before" else 4 * n
    with pytest.raises(GuardError, match=rf"stray store near buffer 'mid' \({4 * n} bytes\): byte offset {off} \("
                                         + ("before its start" if side == "before" else "past its end")):
        ar.assert_guards_intact("after the stray store")


def test_a_store_a_whole_guard_away_is_still_inside_the_guard():
    ar = Arena("cpu", capacity=1 << 20)
    body = ar.carve("only", shape=(64,))
    w = _alias(ar, body, GUARD // 4, 64 + 2 * (GUARD // 4))
    w[0] = 0.0
    with pytest.raises(GuardError, match=rf"'only' \(256 bytes\): byte offset -{GUARD} "):
        ar.assert_guards_intact("far")
    w[0] = torch.frombuffer(bytearray([GUARD_FILL] * 4), dtype=torch.float32)[0]
    ar.assert_guards_intact("restored")
    w[-1] = 0.0
    with pytest.raises(GuardError, match=rf"byte offset {256 + GUARD - 4} \(past its end\)"):
        ar.assert_guards_intact("far")


@pytest.mark.parametrize("layout", ["pitch", "head_major_pitch", "packed"])
def test_one_element_in_a_stride_gap_is_reported(layout):
    ar = Arena("cpu", capacity=1 << 20)
    if layout == "pitch":
        box = {}
        v = ar.carve("y", shape=(B, H, R, d + 4), views=lambda t: _keep(box, t)[..., :d])
        v.fill_(1.0)
        ar.assert_guards_intact("clean")
        box["c"][1, 2, 3, d] = 1.0  # the first gap element of a row
        want = 4 * (((1 * H + 2) * R + 3) * (d + 4) + d)
    elif layout == "head_major_pitch":
        box = {}
        v = ar.carve("y", shape=(B, R, H, d + 4), views=lambda t: _keep(box, t)[..., :d].transpose(1, 2))
        assert v.shape == (B, H, R, d)
        v.fill_(1.0)
        ar.assert_guards_intact("clean")
        box["c"][0, 4, 1, d + 3] = 1.0  # the last gap element of a row
        want = 4 * ((4 * H + 1) * (d + 4) + d + 3)
    else:  # dQ and dV are handed to the library, the middle plane is not: it is gap
        box = {}
        v = ar.carve("y", shape=(B, R, 3, H, d),
                     views=lambda t: tuple(_keep(box, t)[:, :, i].transpose(1, 2) for i in (0, 2)))
        for t in v:
            t.fill_(1.0)
        ar.assert_guards_intact("clean")
        box["c"][1, 0, 1, 0, 0] = 1.0
        want = 4 * ((1 * R * 3 + 1) * H * d)
    with pytest.raises(GuardError, match=rf"near buffer 'y' .*: byte offset {want} \(in a stride gap\)"):
        ar.assert_guards_intact("after the gap store")


def test_one_unwritten_or_non_finite_element_is_reported():
    ar = Arena("cpu", capacity=1 << 20, poison=POISON_ONES)
    y = ar.carve("y", shape=(B, H, R, d + 4), views=lambda t: t[..., :d])
    ids = ar.carve("ids", shape=(9,), dtype=torch.int64)
    y.fill_(0.5)
    ids.fill_(3)
    ar.assert_written(y, "y")
    ar.assert_written(ids, "ids")
    y[1, 0, 4, d - 1] = torch.full((1,), -1, dtype=torch.int32).view(torch.float32)[0]  # the poison pattern again
    with pytest.raises(GuardError, match=r"'y': element \(1, 0, 4, 7\) was never written .*1 of 240 unwritten"):
        ar.assert_written(y, "y")
    y[1, 0, 4, d - 1] = float("inf")
    with pytest.raises(GuardError, match=r"'y': element \(1, 0, 4, 7\) is inf, not finite"):
        ar.assert_written(y, "y")
    ids[8] = -1
    with pytest.raises(GuardError, match=r"'ids': element \(8,\) was never written"):
        ar.assert_written(ids, "ids")
    ar.assert_guards_intact("none of this touched a guard")


def test_fill_repoisons_the_body_and_leaves_gaps_and_guards():
    ar = Arena("cpu", capacity=1 << 20, poison=POISON_ZERO)
    y = ar.carve("y", shape=(B, H, R, d + 4), views=lambda t: t[..., :d])
    assert bool((y == 0).all())
    y.fill_(2.0)
    ar.fill("y", POISON_ONES)
    assert bool(torch.isnan(y).all())
    ar.assert_guards_intact("after fill")
    with pytest.raises(GuardError, match="capacity"):
        ar.carve("big", nbytes=2 << 20)


def test_guard_case_lists_cover_their_tables_and_the_dispatch_lines_still_stand():
    """The SBM list hits classes A-F (test_sbm_wide_gpu.launch_class) and every group of its table, the CSE list every
    prep path, form and class; the csrc lines those lists restate are still there, so a moved threshold or a resized
    buffer fails here instead of silently shrinking what the GPU tests cover."""
    for name, lines in (("csa_sbm.hip", DISPATCH_LINES + sbm_guard.LAYOUT_LINES), ("csa_rel.hip", cse_guard.REL_LINES)):
        with open(os.path.join(PKG, "csrc", name)) as f:
            src = f.read()
        for line in lines:
            assert line in src, f"{name} no longer has `{line}`: restate the case lists of the ABI guard tests"
    sbm_guard.assert_specs_cover_every_class_and_path()
    cse_guard.assert_specs_cover_every_path()
    assert [cse_guard.prep_path(N) for N in (70, 256, 257, 1024, 1025, 1040)] == ["merged", "merged", "prep", "prep",
                                                                                 "prep_t", "prep_t"]
