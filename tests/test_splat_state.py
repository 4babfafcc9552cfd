"""Splat state: hide, select and tint resident splats without re-upload (include/gsplat/gs_abi.h "splat state").

The reference every GPU answer is held to is tests/state_restate.py: a numpy restatement of the region membership, of the four
operations and of the frame a state plane must produce.  The CPU tests prove that the restatement's projection IS the oracle's
(the uv words of GaussianData), that the constructed frame IS the oracle's frame of the scene without the hidden records, and
that the regions are non-trivial.  The GPU tests compare bit for bit: the plane, `matched` and the counts after every call of a
scripted sequence; every tap and the image of frames rendered with hidden and selected splats on every frame path; and that a
context with the flag and an all-zero plane renders what a context without it renders.  No tolerance appears except
gpu_checks.check_image for the fused blend, used as it stands.
"""
import ctypes
import functools
import re

import numpy as np
import pytest

import state_restate as sr
from support import F, FRAME_CASES, NODE, c_layout, hidden_plane, host_sources, in_region, mk, run_node, state_ref, state_scene, timeless

_mk = functools.partial(mk, exact=True, state=True)

# matched splats per region, checked on the CPU when the feature was specified
EXPECTED = {"cfgA": {"centre_half_rect": 2394, "strip": 441, "sphere_r1": 489, "sphere_r075": 214, "box": 615, "mask": 1280},
            "ragged": {"centre_half_rect": 477, "strip": 118, "sphere_r1": 144, "sphere_r075": 67, "box": 189, "mask": 158}}
FRAME_IDS = ["%s-t%d" % c for c in FRAME_CASES]
HIDDEN_SETS = ("every_third", "centre_half_rect", "all")


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_state_abi(tmp_path):
    """The symbols are exported without a GPU; constants and the gs_region layout agree between the header (compiled), ctypes and
    the JS tables; a null context is refused with a message; the ABI version stays 3."""
    from gsplat import _abi
    L = _abi.load()
    for name in ("gs_state_region", "gs_state_ids", "gs_state_count", "gs_state_write"):
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    assert L.gs_abi_version() == 3
    fields = [n for n, _ in _abi.GsRegion._fields_]
    consts = ["GS_FLAG_SPLAT_STATE", "GS_BUF_SPLAT_STATE", "GS_OPT_SELECT_TINT", "GS_SPLAT_HIDDEN", "GS_SPLAT_SELECTED", "GS_STATE_SET",
              "GS_STATE_CLEAR", "GS_STATE_TOGGLE", "GS_STATE_ASSIGN", "GS_REGION_ALL", "GS_REGION_SPHERE", "GS_REGION_BOX",
              "GS_REGION_SCREEN_RECT", "GS_REGION_SCREEN_MASK", "GS_ABI_VERSION"]
    prog = 'printf("%zu", sizeof(gs_region));'
    prog += "".join('printf(" %%zu", offsetof(gs_region, %s));' % n for n in fields)
    prog += "".join('printf(" %%u", (unsigned)%s);' % c for c in consts)
    out = c_layout(tmp_path, "state_layout", prog)
    assert out[0] == ctypes.sizeof(_abi.GsRegion) == 72
    assert out[1:1 + len(fields)] == [getattr(_abi.GsRegion, n).offset for n in fields]
    got = out[1 + len(fields):]
    assert got == [0x10, 15, 11, 1, 2, 1, 2, 3, 4, 0, 1, 2, 3, 4, 3]
    assert got[:-1] == [getattr(_abi, c) for c in consts[:-1]]
    assert [sr.HIDDEN, sr.SELECTED, sr.SET, sr.CLEAR, sr.TOGGLE, sr.ASSIGN, sr.ALL, sr.SPHERE, sr.BOX, sr.RECT, sr.MASK] == got[3:14]
    assert _abi.GS_SELECT_TINT_DEFAULT == sr.TINT_DEFAULT == 0x80FFFF00
    rjs, idx, dts, napi, hdr = host_sources()
    assert re.search(r"#define GS_ABI_VERSION 3\b", hdr) and "default 0x80FFFF00" in hdr and "no counterpart" in hdr
    assert "STATE = { HIDDEN: 0x1, SELECTED: 0x2, SET: 1, CLEAR: 2, TOGGLE: 3, ASSIGN: 4 }" in rjs
    assert "REGION = { ALL: 0, SPHERE: 1, BOX: 2, SCREEN_RECT: 3, SCREEN_MASK: 4 }" in rjs
    assert re.search(r"\bSTATE, REGION\b", idx) and re.search(r"SPLAT_STATE: 15\b", idx) and re.search(r"SPLAT_STATE: 0x10\b", idx)
    assert re.search(r"SELECT_TINT: 11\b", idx)
    assert "HIDDEN: 0x1; SELECTED: 0x2; SET: 1; CLEAR: 2; TOGGLE: 3; ASSIGN: 4" in dts
    assert "ALL: 0; SPHERE: 1; BOX: 2; SCREEN_RECT: 3; SCREEN_MASK: 4" in dts
    for m in ("stateRegion(", "stateIds(", "stateCount(", "readState(", "writeState("):
        assert m in dts and m in rjs
    for name in ("stateRegion", "stateIds", "stateCount", "readState", "writeState"):
        assert '{"%s", js_' % name in napi
    for name in ("FLAG_SPLAT_STATE", "BUF_SPLAT_STATE", "OPT_SELECT_TINT"):
        assert '"%s", GS_%s' % (name, name) in napi
    # no context: refused, with a message, before anything else is looked at
    rg = _abi.GsRegion()
    rg.struct_size = ctypes.sizeof(rg)
    n = ctypes.c_uint64()
    ids = (ctypes.c_uint32 * 1)(0)
    for call, who in ((lambda: L.gs_state_region(None, ctypes.byref(rg), 1, 1, ctypes.byref(n)), b"gs_state_region"),
                      (lambda: L.gs_state_ids(None, ids, 1, 1, 1), b"gs_state_ids"),
                      (lambda: L.gs_state_count(None, 0, 0, ctypes.byref(n)), b"gs_state_count"),
                      (lambda: L.gs_state_write(None, ids, 1), b"gs_state_write")):
        assert call() == _abi.GS_ERR_INVALID_ARGUMENT
        assert who in L.gs_last_error() and b"null" in L.gs_last_error()


@pytest.mark.parametrize("name,ts,count", [("cfgA", 16, 5813), ("ragged", 8, 1347)])
def test_restated_projection_is_the_oracles(oracle, name, ts, count):
    """uv of the restatement is bit-equal to words 0 and 1 of the oracle's GaussianData for every splat with a count."""
    s, u, W, H = state_scene(name)
    gdata, counts = oracle.preprocess(s, u, W, H, ts)
    uvx, uvy, px, py, _ = sr.project(s, u, W, H)
    vis = counts > 0
    assert int(vis.sum()) == count
    np.testing.assert_array_equal(uvx.view(np.uint32)[vis], gdata[vis, 0])
    np.testing.assert_array_equal(uvy.view(np.uint32)[vis], gdata[vis, 1])
    np.testing.assert_array_equal(px.view(np.uint32), (uvx * F(W)).view(np.uint32))
    np.testing.assert_array_equal(py.view(np.uint32), (uvy * F(H)).view(np.uint32))


@pytest.mark.parametrize("name,ts", [("cfgA", 16), ("ragged", 8)])
def test_frame_construction_is_right(oracle, name, ts):
    """Hidden = i % 3 == 1: the constructed frame's f32 image is bit-equal to the oracle's frame of the scene with those records
    REMOVED (another route to the same pixels: the ids differ, the image cannot), and differs from the full frame."""
    s, u, W, H = state_scene(name)
    state = hidden_plane(name, "every_third")
    fr = state_ref(oracle, name, ts, "every_third", state)
    removed = oracle.render(s[state == 0], u, W, H, ts)
    np.testing.assert_array_equal(fr["rgbf"].view(np.uint32), removed["rgbf"].view(np.uint32))
    np.testing.assert_array_equal(fr["rgba8"], removed["rgba8"])
    full = oracle.render(s, u, W, H, ts)
    changed = int((fr["rgbf"].view(np.uint32) != full["rgbf"].view(np.uint32)).any(axis=2).sum())
    print("\n%s: %d pixels change against the full frame" % (name, changed))
    assert changed > W * H // 10
    # a selected splat changes the frame too, and a = 0 does not
    sel = np.where(in_region(name, "centre_half_rect"), sr.SELECTED, 0).astype(np.uint8)
    tinted = sr.state_frame(oracle, s, u, W, H, ts, sel)
    assert (tinted["rgbf"].view(np.uint32) != full["rgbf"].view(np.uint32)).any()
    untinted = sr.state_frame(oracle, s, u, W, H, ts, sel, tint=0x00FF00FF)
    np.testing.assert_array_equal(untinted["rgbf"].view(np.uint32), full["rgbf"].view(np.uint32))
    np.testing.assert_array_equal(untinted["gdata"], full["gdata"])


@pytest.mark.parametrize("name", ["cfgA", "ragged"])
def test_regions_are_non_trivial(name):
    """Every region matches the number of splats it was specified with: more than 1 % and less than 50 % of N, so a kernel that
    matches nothing or everything cannot pass."""
    s, u, W, H = state_scene(name)
    n = s.shape[0]
    got = {r: int(in_region(name, r).sum()) for r in sr.issue_regions(W, H, u)}
    print("\n%s: %s" % (name, got))
    assert got == EXPECTED[name]
    for r, m in got.items():
        assert 0.01 * n < m < 0.5 * n, (r, m)


def test_restated_operations():
    """The four operations, the where filter and sequential ids of the restatement itself, on a plane small enough to read."""
    s0 = np.array([0, 1, 2, 3, 0x80, 0xFF], np.uint8)
    inside = np.array([1, 1, 1, 0, 1, 1], bool)
    out, m = sr.apply_region(s0, inside, sr.SET, 0x04)
    assert m == 5 and out.tolist() == [4, 5, 6, 3, 0x84, 0xFF]
    out, m = sr.apply_region(s0, inside, sr.CLEAR, 0x81, where=(1, 1))
    assert m == 2 and out.tolist() == [0, 0, 2, 3, 0x80, 0x7E]
    out, m = sr.apply_region(s0, inside, sr.TOGGLE, 0x03, where=(2, 0))
    assert m == 3 and out.tolist() == [3, 2, 2, 3, 0x83, 0xFF]
    out, m = sr.apply_region(s0, inside, sr.ASSIGN, 0x10)
    assert m == 5 and out.tolist() == [0x10, 0x10, 0x10, 3, 0x10, 0x10]
    assert sr.apply_ids(s0, [1, 1, 2, 1], sr.TOGGLE, 0x02).tolist() == [0, 3, 0, 3, 0x80, 0xFF]
    assert sr.count(s0, 0x1, 0x1) == 3 and sr.count(s0, 0, 0) == 6 and sr.count(s0, 0xFF, 0x80) == 1


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
def _kernel_scene(n):
    """(splats, uniforms, W, H) with n splats: the two issue scenes, and for 1 and 5 a few of config A's splats, members and
    non-members of the regions alternating."""
    if n == 10000:
        return state_scene("cfgA")
    if n == 3001:
        return state_scene("ragged")
    s, u, W, H = state_scene("cfgA")
    inr = in_region("cfgA", "centre_half_rect") & in_region("cfgA", "box")
    pick = np.stack([np.flatnonzero(inr)[:n], np.flatnonzero(~inr)[:n]], axis=1).ravel()[:n]
    return np.ascontiguousarray(s[pick]), u, W, H


def _script(n, W, H, u):
    """About 20 calls: every kind, every op, where filters on the HIDDEN bit, the SELECTED bit and a host bit, id lists with
    duplicates, TOGGLE twice, neighbours of one word under different ops, and the write of a snapshot."""
    HID, SEL = sr.HIDDEN, sr.SELECTED
    ids = lambda a: (np.asarray(a, np.int64) % n).astype(np.uint32)  # noqa: E731
    quad = 4 * (np.arange(40) * 37 % max(n // 4, 1))
    return [
        ("region", "centre_half_rect", sr.SET, SEL, (0, 0)),
        ("region", "sphere_r1", sr.SET, HID, (0, 0)),
        ("region", "box", sr.TOGGLE, 0x10, (0, 0)),
        ("region", "mask", sr.ASSIGN, 0x22, (HID, 0)),                 # only what is not hidden
        ("region", "strip", sr.SET, 0x04, (SEL, SEL)),                 # only what is selected
        ("region", None, sr.CLEAR, HID, (0x10, 0x10)),                 # ALL, filtered on a host bit
        ("ids", ids([7, 7, 7, 12, 0, n - 1, n - 1]), sr.SET, SEL),     # duplicates
        ("ids", ids(list(range(0, 64, 3)) * 2), sr.TOGGLE, 0x40),      # every id twice: a no-op
        ("ids", ids([5, 9, 5, 5]), sr.TOGGLE, 0x40),                   # three times: once
        ("ids", ids(quad), sr.SET, 0x80),                              # the four bytes of one word, one op each
        ("ids", ids(quad + 1), sr.CLEAR, 0xFF),
        ("ids", ids(quad + 2), sr.TOGGLE, 0x03),
        ("ids", ids(quad + 3), sr.ASSIGN, 0x55),
        ("snapshot",),
        ("region", None, sr.ASSIGN, 0x00, (0, 0)),
        ("region", "sphere_r075", sr.TOGGLE, 0xFF, (0, 0)),
        ("restore",),
        ("region", "sphere_r075", sr.CLEAR, SEL, (0x80, 0)),
        ("region", None, sr.TOGGLE, 0xFF, (HID | SEL, HID | SEL)),
        ("region", "box", sr.ASSIGN, HID | SEL, (0x0C, 0x04)),
        ("ids", np.zeros(0, np.uint32), sr.SET, 0xFF),                 # an empty list: nothing
        ("region", "centre_half_rect", sr.ASSIGN, 0x00, (0, 0)),
    ]


COUNT_PAIRS = ((0, 0), (sr.HIDDEN, sr.HIDDEN), (sr.HIDDEN | sr.SELECTED, sr.SELECTED), (0xFF, 0x22), (0x10, 0), (0xFF, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 3001, 10000])
def test_state_kernels(n):
    """After every call of the script: the plane, `matched` and the counts equal the restatement.  N = 1, 5: the tail of the
    four-per-thread kernel and a partial last word; 3001: one odd tail behind 750 full words; 10000: several workgroups."""
    s, u, W, H = _kernel_scene(n)
    assert s.shape[0] == n
    R = sr.issue_regions(W, H, u)
    r = _mk(s, W, H, 8)
    want = np.zeros(n, np.uint8)
    np.testing.assert_array_equal(r.read_state(), want)  # an upload zeroes the plane; readable before any frame
    snap = None
    seen_change = 0
    for step, call in enumerate(_script(n, W, H, u)):
        if call[0] == "region":
            _, region, op, bits, where = call
            kind, kw = R[region] if region else (sr.ALL, {})
            new, m = sr.apply_region(want, sr.member(kind, s, W, H, **kw), op, bits, where)
            got = r.state_region(kind, op, bits, where, **kw)
            print("step %d %s: matched %d (restatement %d)" % (step, region or "all", got, m))
            assert got == m, (step, call[1:])
        elif call[0] == "ids":
            _, ids, op, bits = call
            new = sr.apply_ids(want, ids, op, bits)
            r.state_ids(ids, op, bits)
        elif call[0] == "snapshot":
            snap = r.read_state()
            new = want
        else:
            r.write_state(snap)
            new = snap.copy()
        seen_change += int(not np.array_equal(new, want))
        want = new
        np.testing.assert_array_equal(r.read_state(), want, err_msg="plane after step %d %r" % (step, call[:2]))
        for mask, value in COUNT_PAIRS:
            assert r.state_count(mask, value) == sr.count(want, mask, value), (step, mask, value)
    assert seen_change >= (10 if n >= 3001 else 3)  # the script moves the plane
    # the one-liners are the calls they stand for
    a = r.select_rect(*R["centre_half_rect"][1]["rect"], u)
    b = r.select_sphere((0.0, 0.0, 0.0), 1.0, op=sr.TOGGLE)
    c = r.select_box((-1.0, -0.5, -1.0), (0.5, 1.0, 1.5), op=sr.CLEAR)
    d = r.select_mask(sr.issue_mask(W, H), u)
    for got, region in ((a, "centre_half_rect"), (b, "sphere_r1"), (c, "box"), (d, "mask")):
        assert got == int(sr.member(R[region][0], s, W, H, **R[region][1]).sum())
    want, _ = sr.apply_region(want, sr.member(*[R["centre_half_rect"][0], s, W, H], **R["centre_half_rect"][1]), sr.SET, sr.SELECTED)
    want, _ = sr.apply_region(want, sr.member(R["sphere_r1"][0], s, W, H, **R["sphere_r1"][1]), sr.TOGGLE, sr.SELECTED)
    want, _ = sr.apply_region(want, sr.member(R["box"][0], s, W, H, **R["box"][1]), sr.CLEAR, sr.SELECTED)
    want, _ = sr.apply_region(want, sr.member(R["mask"][0], s, W, H, **R["mask"][1]), sr.SET, sr.SELECTED)
    np.testing.assert_array_equal(r.read_state(), want)
    nsel = sr.count(want, sr.SELECTED, sr.SELECTED)
    assert r.hide_selected() == nsel
    want, _ = sr.apply_region(want, np.ones(n, bool), sr.SET, sr.HIDDEN, (sr.SELECTED, sr.SELECTED))
    np.testing.assert_array_equal(r.read_state(), want)
    assert r.clear_selection() == n and r.unhide_all() == n
    np.testing.assert_array_equal(r.read_state(), want & np.uint8(0xFC))
    r.destroy()


@pytest.mark.gpu
def test_state_errors():
    """Every refused call leaves the plane as it was; a context without the flag refuses every call, the tap and the option."""
    from gsplat import _abi
    s, u, W, H = state_scene("ragged")
    n = s.shape[0]
    L = _abi.load()
    r = _mk(s, W, H, 8)
    r.state_region(sr.SPHERE, sr.SET, 0x21, a=(0, 0, 0), b=(1.0, 0, 0))
    before = r.read_state()
    assert before.any()

    def code(fn):
        with pytest.raises(_abi.GsError) as e:
            fn()
        return e.value.code, str(e.value)

    def region(**over):
        rg = _abi.GsRegion()
        rg.struct_size, rg.kind = ctypes.sizeof(rg), sr.ALL
        for k, v in over.items():
            setattr(rg, k, v)
        return rg

    uu = np.ascontiguousarray(u, F)
    mask = sr.issue_mask(W, H)
    m = ctypes.c_uint64(77)
    c, msg = code(lambda: r.state_ids(np.array([3, 5, n, 7], np.uint32), sr.ASSIGN, 0xFF))
    assert c == _abi.GS_ERR_INVALID_ARGUMENT and "ids[2]" in msg and str(n) in msg
    c, msg = code(lambda: r.state_ids(np.array([0xFFFFFFFF], np.uint32), sr.SET, 1))
    assert c == _abi.GS_ERR_INVALID_ARGUMENT and "ids[0]" in msg
    assert code(lambda: r.write_state(np.ones(n - 1, np.uint8)))[0] == _abi.GS_ERR_INVALID_ARGUMENT
    assert code(lambda: r.write_state(np.ones(n + 1, np.uint8)))[0] == _abi.GS_ERR_INVALID_ARGUMENT
    assert code(lambda: r.state_region(5, sr.SET, 0xFF))[0] == _abi.GS_ERR_INVALID_ARGUMENT          # kind
    assert code(lambda: r.state_region(sr.ALL, 0, 0xFF))[0] == _abi.GS_ERR_INVALID_ARGUMENT          # op
    assert code(lambda: r.state_region(sr.ALL, 5, 0xFF))[0] == _abi.GS_ERR_INVALID_ARGUMENT
    assert code(lambda: r.state_ids(np.array([1], np.uint32), 9, 0xFF))[0] == _abi.GS_ERR_INVALID_ARGUMENT
    assert code(lambda: r.state_region(sr.ALL, sr.SET, 0x100))[0] == _abi.GS_ERR_INVALID_ARGUMENT    # bits beyond the byte
    assert L.gs_state_region(r._ctx, ctypes.byref(region(struct_size=64)), sr.SET, 0xFF, ctypes.byref(m)) == -1
    assert b"struct_size" in L.gs_last_error()
    assert L.gs_state_region(r._ctx, None, sr.SET, 0xFF, ctypes.byref(m)) == -1
    assert L.gs_state_region(r._ctx, ctypes.byref(region(kind=sr.RECT, x1=W, y1=H)), sr.SET, 0xFF, ctypes.byref(m)) == -1  # no camera
    assert b"uniforms160" in L.gs_last_error()
    assert L.gs_state_region(r._ctx, ctypes.byref(region(kind=sr.MASK, mask=mask.ctypes.data)), sr.SET, 0xFF, ctypes.byref(m)) == -1
    assert L.gs_state_region(r._ctx, ctypes.byref(region(kind=sr.MASK, uniforms160=uu.ctypes.data)), sr.SET, 0xFF, ctypes.byref(m)) == -1
    assert b"mask" in L.gs_last_error()
    assert L.gs_state_count(r._ctx, 0, 0, None) == -1
    assert L.gs_state_ids(r._ctx, None, 3, sr.SET, 1) == -1
    assert L.gs_state_write(r._ctx, None, n) == -1
    assert m.value == 77
    with pytest.raises(ValueError):
        r.state_region(sr.MASK, sr.SET, 1, uniforms=u, mask=np.zeros((H, W + 1), np.uint8))
    np.testing.assert_array_equal(r.read_state(), before)
    # matched may be left out
    assert L.gs_state_region(r._ctx, ctypes.byref(region()), sr.TOGGLE, 0x80, None) == 0
    np.testing.assert_array_equal(r.read_state(), before ^ np.uint8(0x80))
    r.destroy()
    # a context without the flag
    p = _mk(s, W, H, 8, state=False)
    p.render_uniforms(u)
    p.wait()
    img = p.read_rgba8()
    for fn in (lambda: p.state_region(sr.ALL, sr.SET, 1), lambda: p.state_ids(np.array([1], np.uint32), sr.SET, 1),
               lambda: p.state_count(0, 0), lambda: p.write_state(np.zeros(n, np.uint8)), lambda: p.read_state(),
               lambda: p.device_ptr(_abi.GS_BUF_SPLAT_STATE), lambda: p.read_buffer(_abi.GS_BUF_SPLAT_STATE, np.uint8),
               lambda: p.set_option(_abi.GS_OPT_SELECT_TINT, 0xFF00FF00), lambda: p.hide_selected()):
        c, msg = code(fn)
        assert c == _abi.GS_ERR_INVALID_ARGUMENT and "GS_FLAG_SPLAT_STATE" in msg
    p.render_uniforms(u)
    p.wait()
    np.testing.assert_array_equal(p.read_rgba8(), img)
    # sharing: a flagged context cannot borrow from an unflagged owner
    with pytest.raises(_abi.GsError) as e:
        _mk(s, W, H, 8, share_with=p)
    assert e.value.code == _abi.GS_ERR_INVALID_ARGUMENT
    p.destroy()


PRODUCT_PATHS = [(1, 2), (1, 0), (1, 1), (0, 0), (0, 1), (0, 2)]  # (GS_OPT_TILE_CULL, GS_OPT_EMIT_ORDER)


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", HIDDEN_SETS)
@pytest.mark.parametrize("case", FRAME_CASES, ids=FRAME_IDS)
def test_hidden_frames(oracle, case, hidden):
    """EXACT: gs_render_debug equals the constructed reference in every tap; gs_render on every binning and emission order passes
    check_product_lists and the bit-equal image check.  Fused: check_image as it stands."""
    from gpu_checks import check_image, check_stages
    from gsplat import _abi
    name, ts = case
    s, u, W, H = state_scene(name)
    state = hidden_plane(name, hidden)
    ref = state_ref(oracle, name, ts, hidden, state)
    if hidden == "all":
        assert ref["num_intersections"] == 0 and not ref["rgba8"][..., :3].any()
    r = _mk(s, W, H, ts, exact=True)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    r.write_state(state)
    r.render_uniforms(u, debug=True)
    r.wait()
    check_stages(r, ref, True, debug=True)
    for cull, order in PRODUCT_PATHS:
        r.set_option(_abi.GS_OPT_TILE_CULL, cull)
        r.set_option(_abi.GS_OPT_EMIT_ORDER, order)
        r.render_uniforms(u)
        r.wait()
        assert r.stats()["tight_binning"] == cull
        check_stages(r, ref, True, debug=False, oracle=oracle, W=W, H=H, ts=ts)
        vals = r.read_buffer(_abi.GS_BUF_VALUES)
        assert not (state[vals] & sr.HIDDEN).any()  # no instance of a hidden splat
    r.destroy()
    f = _mk(s, W, H, ts, exact=False)
    f.write_state(state)
    f.render_uniforms(u)
    f.wait()
    check_image(f, ref, False)
    f.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [(0, 3), (3, 16), (5, 16)], ids=lambda c: "cols%d-%d" % c)
def test_hidden_frames_on_slabs(oracle, cols):
    """Tile-column slabs at tile size 16 (with the whole canvas these reach every NB instantiation of the projection: 8, 1 / 2, 4)
    against the oracle with cols=."""
    from gpu_checks import check_stages
    from gsplat import _abi
    name, ts = "cfgA", 16
    s, u, W, H = state_scene(name)
    state = hidden_plane(name, "every_third")
    ref = state_ref(oracle, name, ts, "every_third", state, cols=cols)
    r = _mk(s, W, H, ts, exact=True, cols=cols)
    r.write_state(state)
    r.render_uniforms(u, debug=True)
    r.wait()
    check_stages(r, ref, True, debug=True)
    for cull in (1, 0):
        r.set_option(_abi.GS_OPT_TILE_CULL, cull)
        r.render_uniforms(u)
        r.wait()
        check_stages(r, ref, True, debug=False, oracle=oracle, W=W, H=H, ts=ts)
    # a screen region on a slab context is a region of the CANVAS
    got = r.state_region(sr.RECT, sr.SET, sr.SELECTED, rect=(W // 4, H // 4, 3 * W // 4, 3 * H // 4), uniforms=u)
    assert got == EXPECTED[name]["centre_half_rect"]
    r.destroy()


def _tint_plane(name):
    """selected = the centre-half rect, hidden = every third: some splats are both."""
    state = hidden_plane(name, "every_third") | np.where(in_region(name, "centre_half_rect"), sr.SELECTED, 0).astype(np.uint8)
    assert ((state & 3) == 3).any() and ((state & 3) == 2).any()
    return state


@pytest.mark.gpu
def test_tint(oracle):
    """EXACT image, f32 tap and GaussianData are bit-equal to the constructed reference for the default tint and another colour;
    a = 0 is the untinted frame; a splat that is selected and hidden is absent."""
    from gpu_checks import check_stages
    from gsplat import _abi
    name, ts = "cfgA", 16
    s, u, W, H = state_scene(name)
    state = _tint_plane(name)
    r = _mk(s, W, H, ts, exact=True)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    r.write_state(state)
    frames = {}
    for tint in (None, 0xC03380E6, 0x00FF00FF):
        if tint is not None:
            r.set_option(_abi.GS_OPT_SELECT_TINT, tint)
        t = sr.TINT_DEFAULT if tint is None else tint
        ref = state_ref(oracle, name, ts, "tint", state, tint=t)
        r.render_uniforms(u, debug=True)
        r.wait()
        check_stages(r, ref, True, debug=True)
        r.render_uniforms(u)
        r.wait()
        check_stages(r, ref, True, debug=False, oracle=oracle, W=W, H=H, ts=ts)
        vals = r.read_buffer(_abi.GS_BUF_VALUES)
        assert not (state[vals] & sr.HIDDEN).any() and (state[vals] & sr.SELECTED).any()
        frames[t] = ref["rgbf"]
    untinted = state_ref(oracle, name, ts, "every_third", hidden_plane(name, "every_third"))
    np.testing.assert_array_equal(frames[0x00FF00FF].view(np.uint32), untinted["rgbf"].view(np.uint32))
    assert (frames[sr.TINT_DEFAULT] != untinted["rgbf"]).any() and (frames[0xC03380E6] != frames[sr.TINT_DEFAULT]).any()
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("ts", [8, 16, 32])
def test_nothing_changes_by_default(ts):
    """A context with the flag and an all-zero plane renders what a context without it renders: image, f32 tap, lists, ranges,
    counts and statistics, on the product path and on gs_render_debug."""
    from gsplat import _abi, synth
    s, _, W, H = state_scene("cfgA")
    a = _mk(s, W, H, ts, exact=False, state=True)
    b = _mk(s, W, H, ts, exact=False, state=False)
    for k, debug in ((2, False), (6, False), (3, True)):
        u = synth.orbit_camera(k, W, H).uniforms(W, H)
        for r in (a, b):
            r.render_uniforms(u, debug=debug)
            r.wait()
        np.testing.assert_array_equal(a.read_rgba8(), b.read_rgba8())
        for which in (_abi.GS_BUF_RGB_F32, _abi.GS_BUF_VALUES, _abi.GS_BUF_RANGES, _abi.GS_BUF_TILE_COUNTS, _abi.GS_BUF_KEYS):
            np.testing.assert_array_equal(a.read_buffer(which), b.read_buffer(which), err_msg=str(which))
        if debug:
            np.testing.assert_array_equal(a.read_buffer(_abi.GS_BUF_GAUSSIAN_DATA), b.read_buffer(_abi.GS_BUF_GAUSSIAN_DATA))
        assert timeless(a.stats()) == timeless(b.stats())
    assert not a.read_state().any()
    a.destroy()
    b.destroy()


@pytest.mark.gpu
def test_frame_paths(oracle):
    """Frames in flight, the frame graph, a borrower and a fresh upload."""
    import gsplat
    from gpu_checks import check_image
    from gsplat import _abi
    name, ts = "cfgA", 16
    s, u, W, H = state_scene(name)
    planes = [("every_third", hidden_plane(name, "every_third")), ("centre_half_rect", hidden_plane(name, "centre_half_rect")),
              ("tint", _tint_plane(name))]
    # three frames in flight, the state edited between the batches (the call drains the ring itself)
    r = _mk(s, W, H, ts, exact=True)
    for key, plane in planes:
        r.write_state(plane)
        for _ in range(3):
            r.render_uniforms(u)
        check_image(r, state_ref(oracle, name, ts, key, plane), True)
    assert r.stats()["frames_in_flight"] == 3 and r.stats()["frames"] == 9
    r.destroy()
    # the frame graph: capture, edit the state and replay, change the tint and replay
    g = _mk(s, W, H, ts, exact=True)
    g.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    g.set_option(_abi.GS_OPT_FRAME_GRAPH, 1)
    frames = 0
    for key, plane, tint in (("zero", np.zeros(s.shape[0], np.uint8), None), ("every_third", planes[0][1], None), ("tint", planes[2][1], None),
                             ("tint", planes[2][1], 0xC03380E6)):
        g.write_state(plane)
        if tint is not None:
            g.set_option(_abi.GS_OPT_SELECT_TINT, tint)
        for _ in range(2):
            g.render_uniforms(u)
            g.wait()
            frames += 1
            check_image(g, state_ref(oracle, name, ts, key, plane, tint=sr.TINT_DEFAULT if tint is None else tint), True)
            assert g.stats()["graph_frames"] == frames
    # a state call is not a frame: taps and statistics still describe what was rendered
    before = (g.read_rgba8(), g.read_buffer(_abi.GS_BUF_VALUES), timeless(g.stats()))
    g.state_region(sr.ALL, sr.ASSIGN, sr.HIDDEN)
    after = (g.read_rgba8(), g.read_buffer(_abi.GS_BUF_VALUES), timeless(g.stats()))
    np.testing.assert_array_equal(before[0], after[0])
    np.testing.assert_array_equal(before[1], after[1])
    assert before[2] == after[2]
    g.render_uniforms(u)
    g.wait()
    assert not g.read_rgba8()[..., :3].any() and g.stats()["graph_frames"] == frames + 1  # the replay saw the new plane
    # a fresh upload zeroes the plane
    arr = np.ascontiguousarray(s, dtype=np.float32)
    _abi.check(_abi.load().gs_upload_splats(g._ctx, arr.ctypes.data, arr.shape[0]))
    assert not g.read_state().any()
    g.destroy()
    # a borrower renders the owner's state; PipelinedRenderer forwards to the owner after draining every slot
    p = gsplat.PipelinedRenderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(s), ts, frames_in_flight=2,
                                 flags=_abi.GS_FLAG_EXACT_BLEND | _abi.GS_FLAG_F32_TAP | _abi.GS_FLAG_SPLAT_STATE)
    for key, plane in planes[:2]:
        p.render_uniforms(u)  # in flight when the state call comes
        p.write_state(plane)
        np.testing.assert_array_equal(p.read_state(), plane)
        slots = [p.render_uniforms(u) for _ in range(2)]
        for slot in slots:
            p.wait(slot)
            check_image(p.renderers[slot], state_ref(oracle, name, ts, key, plane), True)
    assert p.select_sphere((0.0, 0.0, 0.0), 1.0) == EXPECTED[name]["sphere_r1"]
    assert p.state_count(sr.SELECTED, sr.SELECTED) == p.renderers[1].state_count(sr.SELECTED, sr.SELECTED) == EXPECTED[name]["sphere_r1"]
    p.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fused"])
def test_pick_after_hiding(oracle, exact):
    """Hide what the centre-half rect selects, render, pick on the lattice of test_pick.py: every field equals pick_restate on
    the constructed reference, and no hidden id appears in any field or contributor slot."""
    from pick_restate import restate_ref
    name, ts = "cfgA", 16
    s, u, W, H = state_scene(name)
    xy = np.array([(x, y) for y in range(3, H, 17) for x in range(5, W, 13)], np.uint32)
    r = _mk(s, W, H, ts, exact=exact)
    assert r.select_rect(W // 4, H // 4, 3 * W // 4, 3 * H // 4, u) == EXPECTED[name]["centre_half_rect"]
    assert r.hide_selected() == EXPECTED[name]["centre_half_rect"]
    state = r.read_state()
    np.testing.assert_array_equal(state, np.where(in_region(name, "centre_half_rect"), 3, 0).astype(np.uint8))
    ref = state_ref(oracle, name, ts, "hidden_selected", state)
    wres, wcon, _ = restate_ref(ref, W, H, ts, xy, 8)
    r.render_uniforms(u)
    r.wait()
    res, con = r.pick(xy, 8)
    words = lambda a: np.ascontiguousarray(a).view(np.uint32).reshape(a.shape + (a.dtype.itemsize // 4,))  # noqa: E731
    keep = [k for k in range(12) if k != 1]  # (list_length: tight lists are a subset of the reference's)
    np.testing.assert_array_equal(words(res)[:, keep], words(wres)[:, keep])
    assert (res["list_length"] <= wres["list_length"]).all()
    np.testing.assert_array_equal(words(con), words(wcon))
    hidden = np.flatnonzero(state & sr.HIDDEN)
    for f in ("first_id", "max_id", "median_id"):
        assert not np.isin(res[f], hidden).any()
    assert not np.isin(con["id"], hidden).any() and (res["hit_count"] > 0).any()
    r.destroy()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_node_host_state_matches_python(tmp_path):
    """tests/js/state_check.js runs a short sequence through the Node host and writes the plane and a frame: both equal what the
    Python host makes of the same sequence, byte for byte."""
    from gsplat import _abi
    s, u, W, H = state_scene("ragged")
    n, ts = s.shape[0], 8
    mask = sr.issue_mask(W, H)
    ids = np.array([5, 5, 9, 2999, 3000, 17, 5], np.uint32)
    rec, ub, mb, ib, out = (str(tmp_path / f) for f in ("rec.bin", "u.bin", "mask.bin", "ids.bin", "state.bin"))
    s.tofile(rec)
    np.ascontiguousarray(u, F).tofile(ub)
    mask.tofile(mb)
    ids.tofile(ib)
    info = run_node("state_check.js", (rec, n, W, H, ts, ub, mb, ib, out))
    r = _mk(s, W, H, ts, exact=False)
    m = [r.state_region(sr.RECT, sr.SET, sr.SELECTED, rect=(W // 4, H // 4, 3 * W // 4, 3 * H // 4), uniforms=u),
         r.state_region(sr.MASK, sr.SET, 0x10, where=(sr.SELECTED, 0), mask=mask, uniforms=u),
         r.state_region(sr.SPHERE, sr.SET, sr.HIDDEN, a=(0.5, 0.2, -0.3), b=(0.75, 0, 0)),
         r.state_region(sr.BOX, sr.TOGGLE, 0x20, a=(-1.0, -0.5, -1.0), b=(0.5, 1.0, 1.5))]
    r.state_ids(ids, sr.TOGGLE, 0x40)
    r.set_option(_abi.GS_OPT_SELECT_TINT, 0xC03380E6)
    plane = r.read_state()
    r.render_uniforms(u)
    r.wait()
    img = r.read_rgba8()
    counts = [r.state_count(sr.HIDDEN, sr.HIDDEN), r.state_count(0xFF, 0)]
    r.write_state(np.zeros(n, np.uint8))
    r.render_uniforms(u)
    r.wait()
    img0 = r.read_rgba8()
    r.destroy()
    assert m == [EXPECTED["ragged"]["centre_half_rect"], info["matched"][1], EXPECTED["ragged"]["sphere_r075"], EXPECTED["ragged"]["box"]]
    assert info["matched"] == m and info["counts"] == counts
    raw = np.fromfile(out, dtype=np.uint8)
    assert raw.size == n + 2 * W * H * 4
    np.testing.assert_array_equal(raw[:n], plane)
    np.testing.assert_array_equal(raw[n:n + W * H * 4].reshape(H, W, 4), img)
    np.testing.assert_array_equal(raw[n + W * H * 4:].reshape(H, W, 4), img0)  # after writeState(zeros): the plain frame
    assert (img != img0).any() and plane.any()
    assert info["errors"] == {"badId": "-1", "unflagged": "-1", "notTyped": "TypeError"}


def _outcome(fn):
    """What a call gives: its value, or the code and message of the GsError it raises."""
    from gsplat import _abi
    try:
        return ("value", fn())
    except _abi.GsError as e:
        return ("error", e.code, str(e))


def _assert_same(a, b, what):
    assert type(a) is type(b), what
    if isinstance(a, tuple):
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            _assert_same(x, y, "%s[%d]" % (what, k))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype, what
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=what)  # floats compared as bits
    else:
        assert a == b, what


@pytest.mark.gpu
def test_pipelined_forwards_reach_the_owner(tmp_path):
    """Every call PipelinedRenderer forwards to the owner of the splats, made while each of its two slots holds a frame nobody
    waited for: the slots are drained, and the return value and the plane afterwards are those of a lone Renderer given the same
    frames and calls.  The four per-slot calls answer what the slot's own renderer answers."""
    import gsplat
    from gsplat import _abi
    from gpu_checks import orbit_uniforms
    s, W, H, ts = np.ascontiguousarray(state_scene("cfgA")[0][:64]), 64, 64, 8
    u = orbit_uniforms(W, H)
    flags = _abi.GS_FLAG_EXACT_BLEND | _abi.GS_FLAG_F32_TAP | _abi.GS_FLAG_SPLAT_STATE
    p = gsplat.PipelinedRenderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(s), ts, frames_in_flight=2, flags=flags)
    lone = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(s), ts, flags=flags)
    SEL, HID = sr.SELECTED, sr.HIDDEN
    mask = sr.issue_mask(W, H)
    snap = {}
    turn = _abi.compose_xform(rot=(0.9, 0.1, -0.2, 0.3), translate=(0.01, 0.0, -0.02), scale=1.25, pivot=(0.1, 0.2, 0.3))
    ply = lambda r: str(tmp_path / ("lone.ply" if r is lone else "ring.ply"))  # noqa: E731
    calls = [
        ("select_sphere", lambda r: r.select_sphere((0.0, 0.0, 0.0), 2.0)),
        ("state_count", lambda r: r.state_count(SEL, SEL)),
        ("state_ids", lambda r: r.state_ids(np.array([1, 2, 2, 63], np.uint32), sr.SET, 0x10)),
        ("read_state", lambda r: snap.setdefault(id(r), r.read_state())),
        ("state_region", lambda r: r.state_region(sr.ALL, sr.TOGGLE, 0x20, (0x10, 0x10))),
        ("write_state", lambda r: r.write_state(snap[id(r)])),
        ("select_box", lambda r: r.select_box((-2.0, -1.0, -2.0), (1.0, 2.0, 3.0), op=sr.TOGGLE)),
        ("select_rect", lambda r: r.select_rect(8, 8, 56, 40, u, op=sr.SET)),
        ("select_mask", lambda r: r.select_mask(mask, u, op=sr.TOGGLE)),
        ("list_state", lambda r: r.list_state(SEL, SEL)),
        ("export_splats", lambda r: r.export_splats(SEL, SEL, with_ids=True)),
        ("translate_selected", lambda r: r.translate_selected((0.05, -0.02, 0.01))),
        ("rotate_selected", lambda r: r.rotate_selected((0.8, 0.0, 0.6, 0.0), pivot=(0.0, 0.1, 0.0))),
        ("scale_selected", lambda r: r.scale_selected(0.9)),
        ("transform", lambda r: r.transform(turn, 0x10, 0x10)),
        ("export_splats", lambda r: r.export_splats()),
        ("reset_coverage", lambda r: r.reset_coverage()),
        ("accumulate_coverage", lambda r: r.accumulate_coverage((4, 4, 60, 50), mask)),
        ("read_coverage", lambda r: r.read_coverage()),
        ("state_coverage", lambda r: r.state_coverage(sr.SET, 0x40, min_hits=2)),
        ("select_visible", lambda r: r.select_visible((0, 0, 32, 64))),
        ("hide_unseen", lambda r: r.hide_unseen()),
        ("hide_selected", lambda r: r.hide_selected()),
        ("save_ply", lambda r: (r.save_ply(ply(r), HID, 0, sh_degree=1), np.fromfile(ply(r), np.uint8))),
        ("unhide_all", lambda r: r.unhide_all()),
        ("clear_selection", lambda r: r.clear_selection()),
    ]
    owner_calls = {"state_region", "state_ids", "state_count", "read_state", "write_state", "select_rect", "select_mask", "select_sphere",
                   "select_box", "clear_selection", "hide_selected", "unhide_all", "accumulate_coverage", "reset_coverage", "read_coverage",
                   "state_coverage", "select_visible", "hide_unseen", "list_state", "export_splats", "save_ply", "transform",
                   "translate_selected", "rotate_selected", "scale_selected"}
    assert {name for name, _ in calls} == owner_calls
    moved = 0
    for name, call in calls:
        for _ in range(2):  # a frame on each slot, in flight when the call comes
            p.render_uniforms(u)
            lone.render_uniforms(u)
        assert p._busy == [True, True]
        before = lone.read_state()
        got, want = call(p), call(lone)
        assert p._busy == [False, False], name  # every slot was drained before the owner was asked
        _assert_same(got, want, name)
        np.testing.assert_array_equal(p.read_state(), lone.read_state(), err_msg="plane after " + name)
        moved += int(not np.array_equal(before, lone.read_state()))
    assert moved >= 8  # the calls move the plane
    # the per-slot calls: the slot is waited for, then its own renderer answers
    xy = np.array([(x, y) for y in range(3, H, 11) for x in range(5, W, 7)], np.uint32)
    for name, via_ring, direct, ok in (("read_rgba8", lambda k: p.read_rgba8(k), lambda r: r.read_rgba8(), True),
                                       ("pick", lambda k: p.pick(k, xy, 4), lambda r: r.pick(xy, 4), True),
                                       ("read_alpha", lambda k: p.read_alpha(k), lambda r: r.read_alpha(), False),  # (no GS_FLAG_AUX_OUTPUTS)
                                       ("read_depth", lambda k: p.read_depth(k, normalized=True), lambda r: r.read_depth(normalized=True), False)):
        slots = [p.render_uniforms(u) for _ in range(2)]
        for slot in slots:
            assert p._busy[slot]
            got = _outcome(lambda: via_ring(slot))
            assert not p._busy[slot], name
            _assert_same(got, _outcome(lambda: direct(p.renderers[slot])), name)
            assert got[0] == ("value" if ok else "error"), (name, got)
    assert p.read_rgba8(slots[0])[..., :3].any()
    p.destroy()
    lone.destroy()
