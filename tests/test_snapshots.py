"""Snapshots and write-back: records scattered into the resident planes by index, and device-resident snapshots of a selection that
restore or swap in place (include/gsplat/gs_abi.h "snapshots and write-back").

The reference every answer is held to is tests/snapshot_restate.py: the floats of the named parts are copied as words, everything
else keeps its bits.  Every float comparison is on the uint32 view and nothing has a tolerance: the only thing computed is an
fmaxf.  A written or restored context is held to the definition the header gives it: indistinguishable from a fresh one given
gs_upload_splats(the edited records) + gs_state_write -- every tap and the image, bit for bit.
"""
import ctypes
import functools
import inspect

import numpy as np
import pytest

from conftest import scene
import export_restate as er
import snapshot_restate as sn
from support import F, SLAB_COLS, TAPS, c_layout, code_of, frame_taps, host_sources, mk, raw_export, special_records, timeless

_mk = functools.partial(mk, exact=True, state=True)
HID, SEL = er.HIDDEN, er.SELECTED
POSITION, GEOMETRY, SH, STATE, RECORD = sn.POSITION, sn.GEOMETRY, sn.SH, sn.STATE, sn.RECORD
SYMBOLS = ("gs_write_splats", "gs_write_splats_device", "gs_snapshot_take", "gs_snapshot_restore", "gs_snapshot_swap",
           "gs_snapshot_get_info", "gs_snapshot_free")
SIZES = [1, 5, 63, 64, 65, 1023, 1025, 3001]
PART_CASES = [POSITION, GEOMETRY, SH, STATE, RECORD | STATE]
W = H = 64
TS = 8


def plane_of(n):
    """State bytes of many values: every third splat selected, every seventh hidden, host bits above."""
    i = np.arange(n)
    return ((((i * 37) & 0x3F) << 2) | np.where(i % 3 == 1, SEL, 0) | np.where(i % 7 == 3, HID, 0)).astype(np.uint8)


def new_records(m, salt):
    """m records to write: special records (NaN payloads, -0, +-inf, a denormal) in another order, every padding float junk."""
    base = special_records(3001)
    out = np.array(base[(np.arange(m) * 7 + 7 * salt) % 3001], dtype=F, copy=True)
    w = out.view(np.uint32)
    w[:, er.PADDING] = 0xC0FFEE00 + salt
    if m:
        w[0, 4], w[m - 1, 17], w[m // 2, 1], w[m // 2, 12] = 0x7FA12345, 0x80000000, 0xFF800000, 0xFFC0BEEF
    return out


def new_states(m, salt):
    return ((np.arange(m) * 29 + 11 * salt + 5) & 0xFF).astype(np.uint8)


def id_sets(n):
    """(name, ids or None, m): the margins of the scatter."""
    sets = [("all", None, n), ("head", None, n // 2), ("first", np.array([0]), 1), ("last", np.array([n - 1]), 1),
            ("third", np.arange(0, n, 3), None)]
    if n >= 8:
        q = (n // 4) // 2
        sets.append(("word", np.arange(4 * q, 4 * q + 4), 4))
    if n > 1024:
        sets.append(("block", np.arange(1020, min(n, 1030)), None))
    return [(name, None if ids is None else ids.astype(np.uint32), m if m is not None else ids.size) for name, ids, m in sets]


def held(r, want_rec, want_state):
    """The context holds exactly these records and state bytes (guarded export, uint32 view)."""
    got, ids = raw_export(r, 0, 0, True)
    np.testing.assert_array_equal(er.bits(got), er.bits(want_rec))
    np.testing.assert_array_equal(ids, np.arange(want_rec.shape[0], dtype=np.uint32))
    if want_state is not None:
        np.testing.assert_array_equal(r.read_state(), want_state)


def frames(r, u):
    """The next two frames of r, product binning and the reference's."""
    return [frame_taps(r, u, debug) for debug in (False, True)]


def same_frames(a, b):
    for fa, fb in zip(a, b):
        for t in TAPS + ("rgba8", "rgbf"):
            np.testing.assert_array_equal(fa[t], fb[t], err_msg=t)


def differ(a, b):
    return any((fa[t] != fb[t]).any() for fa, fb in zip(a, b) for t in ("rgba8", "GAUSSIAN_DATA"))


def uniforms(w=W, h=H):
    from gpu_checks import orbit_uniforms
    return orbit_uniforms(w, h)


def base_scene():
    """3001 plain records (finite: their frames are compared) and their state plane."""
    return np.ascontiguousarray(scene(10000)[:3001]), plane_of(3001)


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_snapshot_abi(tmp_path):
    """The seven symbols are exported without a GPU and listed; the ABI version stays 3; gs_snapshot_info is 32 bytes with the
    header's offsets; null and unknown arguments are refused with a message that names the call; the header section sits between the
    colour grades and the coverage and says what the issue pins."""
    from gsplat import _abi
    L = _abi.load()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    assert L.gs_abi_version() == 3
    fields = [n for n, _ in _abi.GsSnapshotInfo._fields_]
    out = c_layout(tmp_path, "snapinfo", 'printf("%zu", sizeof(gs_snapshot_info));' +
                   "".join('printf(" %%zu", offsetof(gs_snapshot_info, %s));' % n for n in fields) +
                   'printf(" %u %u %u %u %u", GS_PART_POSITION, GS_PART_GEOMETRY, GS_PART_SH, GS_PART_STATE, GS_PART_RECORD);')
    assert out[0] == 32 == ctypes.sizeof(_abi.GsSnapshotInfo)
    assert out[1:6] == [getattr(_abi.GsSnapshotInfo, n).offset for n in fields] == [0, 8, 16, 24, 28]
    assert out[6:] == [_abi.GS_PART_POSITION, _abi.GS_PART_GEOMETRY, _abi.GS_PART_SH, _abi.GS_PART_STATE, _abi.GS_PART_RECORD] == [1, 2, 4, 8, 7]
    rec = np.zeros((1, 80), F)
    st = np.zeros(1, np.uint8)
    n, h = ctypes.c_uint64(77), ctypes.c_void_p(78)
    info = _abi.GsSnapshotInfo()
    for fn, who in ((L.gs_write_splats, b"gs_write_splats"), (L.gs_write_splats_device, b"gs_write_splats_device")):
        for args, word in (((None, None, 1, rec.ctypes.data, None, RECORD), b"null ctx"), ((None, None, 1, None, None, RECORD), b"null records"),
                           ((None, None, 1, rec.ctypes.data, None, RECORD | STATE), b"null states"),
                           ((None, None, 1, rec.ctypes.data, st.ctypes.data, 0x10), b"part")):
            assert fn(*args, ctypes.byref(n)) == _abi.GS_ERR_INVALID_ARGUMENT
            assert who + b":" in L.gs_last_error() and word in L.gs_last_error(), L.gs_last_error()
    for args, word in (((None, 0, 0, RECORD, ctypes.byref(h)), b"null ctx"), ((None, 0, 0, RECORD, None), b"null out"),
                       ((None, 0, 0, 0x10, ctypes.byref(h)), b"part")):
        assert L.gs_snapshot_take(*args) == _abi.GS_ERR_INVALID_ARGUMENT
        assert b"gs_snapshot_take:" in L.gs_last_error() and word in L.gs_last_error(), L.gs_last_error()
    for fn, who in ((L.gs_snapshot_restore, b"gs_snapshot_restore"), (L.gs_snapshot_swap, b"gs_snapshot_swap")):
        assert fn(None, None, 0, ctypes.byref(n)) == _abi.GS_ERR_INVALID_ARGUMENT
        assert who + b":" in L.gs_last_error() and b"null" in L.gs_last_error()
    assert L.gs_snapshot_get_info(None, ctypes.byref(info)) == _abi.GS_ERR_INVALID_ARGUMENT
    assert b"gs_snapshot_get_info: null snapshot" in L.gs_last_error()
    assert L.gs_snapshot_free(None) == 0
    assert n.value == 77 and h.value == 78
    hdr = host_sources().hdr
    for name in SYMBOLS:
        assert "int32_t %s(" % name in hdr
    assert "#define GS_ABI_VERSION 3\n" in hdr
    assert hdr.index("---- colour grades") < hdr.index("---- snapshots and write-back") < hdr.index("---- coverage")
    sec = hdr[hdr.index("---- snapshots and write-back"):hdr.index("---- coverage")]
    for words in ("strictly ascending", "serial", "12 B", "32 B", "192 B", "1 B", "NOT a frame", "typedef struct gs_snapshot_info {"):
        assert words in sec, words
    # the sentences the transform and grade tests pin are still there, each with a pointer to this section
    assert "The inverse transform is NOT a bit-exact undo (every step rounds): a host that wants one exports the selection first." in hdr
    assert "The inverse grade is NOT a bit-exact undo." in hdr
    for title in ("---- splat transforms", "---- colour grades"):
        at = hdr.index(title)
        assert "snapshots and write-back" in hdr[at:hdr.index("#define", at)]


def test_snapshot_module_surface():
    """gsplat.snapshots is a module of free functions and one class with the stated signatures; the host classes are untouched
    (test_abi pins them)."""
    import gsplat
    from gsplat import _abi, snapshots
    assert gsplat.snapshots is snapshots
    want = {"write": "(r, ids, records, states=None, parts=7)", "take": "(r, mask=2, value=2, parts=7)",
            "take_selected_for": "(r, xform_or_grade)"}
    live = {n: str(inspect.signature(f)) for n, f in vars(snapshots).items()
            if inspect.isfunction(f) and f.__module__ == snapshots.__name__ and not n.startswith("_")}
    assert live == want
    methods = {"restore": "(self, parts=0)", "swap": "(self, parts=0)", "info": "(self)", "free": "(self)"}
    S = snapshots.Snapshot
    assert {n: str(inspect.signature(f)) for n, f in vars(S).items() if inspect.isfunction(f) and not n.startswith("_")} == methods
    for f in [getattr(snapshots, n) for n in want] + [getattr(S, n) for n in methods]:
        assert f.__doc__
    assert all(hasattr(S, n) for n in ("__enter__", "__exit__", "__del__"))
    assert (snapshots.POSITION, snapshots.GEOMETRY, snapshots.SH, snapshots.STATE, snapshots.RECORD) == (1, 2, 4, 8, 7)
    # a freed snapshot raises ValueError (free itself may be repeated); no GPU: the handle is never looked at
    s = S(None, None)
    s.free()
    for call in (s.restore, s.swap, s.info):
        with pytest.raises(ValueError):
            call()
    for cls in (gsplat.Renderer, gsplat.PipelinedRenderer):
        assert not any(hasattr(cls, v) for v in ("write_splats", "snapshot", "take_snapshot", "restore", "swap"))
    assert _abi.GS_PART_RECORD == _abi.GS_PART_POSITION | _abi.GS_PART_GEOMETRY | _abi.GS_PART_SH


def test_restatement_agrees_with_the_export():
    """snapshot_restate on records with NaN payloads, -0 and infinities: writing a record's own exported floats back is the identity;
    writing part P changes exactly the floats of P in the export; padding junk never appears."""
    assert sn.PART_FLOATS[POSITION] == [0, 1, 2] and sn.PART_FLOATS[GEOMETRY] == [4, 5, 6, 8, 9, 10, 11, 12]
    assert sn.PART_FLOATS[SH] == [16 + 4 * k + c for k in range(16) for c in range(3)]
    assert sn.floats_of(RECORD) == sorted(er.CARRIED) and sn.floats_of(STATE) == [] and sn.floats_of(0) == []
    for n in (5, 65, 3001):
        old = special_records(n)
        plane = plane_of(n)
        exported = er.records(old, plane, 0, 0)
        assert not np.isfinite(old).all() or n == 5
        ids = np.arange(0, n, 3)
        rec, st = sn.written(old, plane, ids, exported[ids], plane[ids], RECORD | STATE)
        np.testing.assert_array_equal(er.bits(rec), er.bits(exported))
        np.testing.assert_array_equal(st, plane)
        new, ns = new_records(ids.size, n), new_states(ids.size, n)
        assert er.bits(new)[:, er.PADDING].all()
        for parts in PART_CASES + [0]:
            rec, st = sn.written(old, plane, ids, new, ns, parts)
            assert not er.bits(rec)[:, er.PADDING].any()
            changed = er.bits(rec) != er.bits(exported)
            fl = sn.floats_of(parts)
            other = [f for f in range(80) if f not in fl]
            assert not changed[:, other].any()
            rest = np.setdiff1d(np.arange(n), ids)
            assert not changed[rest].any()
            np.testing.assert_array_equal(er.bits(rec)[np.ix_(ids, fl)], er.bits(new)[:, fl])
            want_st = plane.copy()
            if parts & STATE:
                want_st[ids] = ns
            np.testing.assert_array_equal(st, want_st)
        if n > 5:
            assert (er.bits(sn.written(old, plane, ids, new, ns, SH)[0]) != er.bits(exported)).any()
        # dense (ids None) writes the first m splats
        rec, _ = sn.written(old, plane, None, new, ns, POSITION)
        np.testing.assert_array_equal(er.bits(rec)[:ids.size, :3], er.bits(new)[:, :3])
        np.testing.assert_array_equal(er.bits(rec)[ids.size:], er.bits(exported)[ids.size:])


# ---- GPU: the scatter at its margins ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_write_at_its_margins(n):
    """Every id set x host and device variant x each single part and RECORD | STATE, one after the other on one context: after every
    write the guarded export of everything and the state plane equal the restatement -- unnamed parts and unnamed splats keep every
    bit, NaN payloads included, and padding junk never arrives."""
    import torch
    from gsplat import snapshots
    old = special_records(n)
    rec, plane = er.zero_padding(old), plane_of(n)
    r = _mk(old, W, H, TS)
    r.write_state(plane)
    held(r, rec, plane)
    salt = 0
    for name, ids, m in id_sets(n):
        for device in (False, True):
            for parts in PART_CASES:
                salt += 1
                new, ns = new_records(m, salt), new_states(m, salt)
                if device:
                    got = snapshots.write(r, None if ids is None else torch.from_numpy(ids.view(np.int32).copy()).cuda(),
                                          torch.from_numpy(new).cuda().reshape(-1, 80), torch.from_numpy(ns).cuda(), parts)
                else:
                    got = snapshots.write(r, ids, new, ns, parts)
                assert got == m, (name, device, parts)
                rec, plane = sn.written(rec, plane, ids, new, ns, parts)
                held(r, rec, plane)
    assert r.stats()["num_gaussians"] == n
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_snapshot_kernels_at_their_margins(n):
    """take / restore / swap over the same id sets (as selections) and parts, dense and by id list, on special records: a restore
    after a write of junk brings back every bit; a swap leaves the junk in the snapshot and a second swap puts it back."""
    from gsplat import _abi, snapshots
    old = special_records(n)
    rec0 = er.zero_padding(old)
    r = _mk(old, W, H, TS)
    salt = 100
    for name, ids, m in id_sets(n):
        if name == "head":
            continue  # (a selection is a set of splats: the dense prefix is "all" on a smaller scene)
        plane = plane_of(n) & ~np.uint8(SEL)
        if ids is not None:
            plane[ids] |= SEL
        r.write_state(plane)
        filt = (0, 0) if ids is None else (SEL, SEL)
        at = np.arange(n, dtype=np.uint32) if ids is None else ids
        snapshots.write(r, None, old, None, RECORD)
        held(r, rec0, plane)
        for parts in PART_CASES:
            salt += 1
            with snapshots.take(r, *filt, parts) as s:
                info = s.info()
                m4 = (m + 3) & ~3
                bytes_want = (0 if ids is None else 4 * m4) + (12 * m4 if parts & POSITION else 0) + (32 * m if parts & GEOMETRY else 0) + \
                    (192 * m if parts & SH else 0) + (m4 if parts & STATE else 0)
                assert info == {"count": m, "n_at_take": n, "device_bytes": bytes_want, "parts": parts, "dense": ids is None}
                new, ns = new_records(m, salt), new_states(m, salt)
                snapshots.write(r, None if ids is None else at, new, ns, RECORD | STATE)
                junk_rec, junk_plane = sn.written(rec0, plane, at, new, ns, RECORD | STATE)
                held(r, junk_rec, junk_plane)
                # restore: the parts taken come back, the others keep the junk
                assert s.restore() == m
                want_rec, want_plane = sn.written(junk_rec, junk_plane, at, rec0[at], plane[at], parts)
                held(r, want_rec, want_plane)
                # swap: scene <- snapshot (already equal for these parts), snapshot <- scene; then junk again, swap, swap
                snapshots.write(r, None if ids is None else at, new, ns, RECORD | STATE)
                assert s.swap() == m
                held(r, want_rec, want_plane)
                assert s.swap() == m
                held(r, junk_rec, junk_plane)
                assert s.swap(parts) == m
                held(r, want_rec, want_plane)
            snapshots.write(r, None, old, plane, RECORD | STATE)
            held(r, rec0, plane)
    r.destroy()


# ---- the derived plane ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_derived_plane_follows_geometry():
    """The largest log-scale is the one derived plane and only a tile-column slab reads it: after a GEOMETRY write and after a
    GEOMETRY restore the frames of a slab context equal, tap for tap and image for image, those of a fresh slab context uploaded
    with the edited records.  (72 x 64: the narrowest canvas on which SLAB_COLS[8] is a slab with its right edge included.)"""
    from gsplat import snapshots
    w, h = 72, 64
    u = uniforms(w, h)
    s, plane = base_scene()
    n = s.shape[0]
    ids = np.arange(1, n, 2, dtype=np.uint32)
    edited = s.copy()
    edited[ids, 4:7] += np.array([1.5, -0.7, 2.0], F)  # the largest log-scale moves, and which of the three it is
    edited[ids, 12] += F(0.5)
    r = _mk(s, w, h, TS, cols=SLAB_COLS[8])
    fresh_old = _mk(s, w, h, TS, cols=SLAB_COLS[8])
    fresh_new = _mk(edited, w, h, TS, cols=SLAB_COLS[8])
    a, b = frames(fresh_old, u), frames(fresh_new, u)
    assert differ(a, b) and a[0]["rgba8"][..., :3].any()
    same_frames(frames(r, u), a)
    undo = snapshots.take(r, 0, 0, GEOMETRY)
    assert snapshots.write(r, ids, edited[ids], None, GEOMETRY) == ids.size
    held(r, er.zero_padding(edited), None)
    same_frames(frames(r, u), b)
    assert undo.swap() == n
    held(r, er.zero_padding(s), None)
    same_frames(frames(r, u), a)
    assert undo.restore(GEOMETRY) == n  # the snapshot now holds the edit
    same_frames(frames(r, u), b)
    undo.free()
    for x in (r, fresh_old, fresh_new):
        x.destroy()


# ---- undo and redo ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_undo_and_redo():
    """On an EXACT, stateful context: frame A, take(selection, RECORD | STATE), rotate, scale, grade, fade and a state change, frame
    B; swap gives A back -- export, plane and every tap of the frame, bit for bit --, swap again gives B, restore twice gives A
    twice.  A POSITION-only translate is undone by a snapshot of 16 bytes per splat."""
    from gsplat import _abi, colours, snapshots
    u = uniforms()
    s, plane = base_scene()
    r = _mk(s, W, H, TS)
    r.write_state(plane)
    sel = np.flatnonzero(plane & SEL).astype(np.uint32)
    m = sel.size
    fa = frames(r, u)
    rec_a = er.zero_padding(s)
    undo = snapshots.take(r, SEL, SEL, RECORD | STATE)
    assert undo.info()["count"] == m and not undo.info()["dense"]
    assert r.rotate_selected((0.9, 0.1, -0.3, 0.2), pivot=(0.5, 0.0, -1.0)) == m
    assert r.scale_selected(1.3) == m
    assert colours.brighten(r, 1.4) == m and colours.saturate(r, 0.3) == m and colours.fade(r, 0.5) == m
    r.state_ids(sel[::2], _abi.GS_STATE_SET, HID | 0x80)
    r.state_ids(sel[1::4], _abi.GS_STATE_CLEAR, SEL)
    rec_b, plane_b = r.export_splats(), r.read_state()
    fb = frames(r, u)
    assert differ(fa, fb) and (plane_b != plane).any()
    rest = np.setdiff1d(np.arange(s.shape[0]), sel)
    np.testing.assert_array_equal(er.bits(rec_b)[rest], er.bits(rec_a)[rest])
    assert undo.swap() == m
    held(r, rec_a, plane)
    same_frames(frames(r, u), fa)
    assert undo.swap() == m
    held(r, rec_b, plane_b)
    same_frames(frames(r, u), fb)
    for _ in range(2):
        assert undo.restore() == m
        held(r, rec_a, plane)
    same_frames(frames(r, u), fa)
    undo.free()
    # the editor's verb: the parts a transform names
    x = _abi.compose_xform(translate=(0.25, -0.5, 0.125))
    assert x.flags == _abi.GS_XFORM_POSITION
    with snapshots.take_selected_for(r, x) as t:
        info = t.info()
        assert info["parts"] == POSITION and info["count"] == m
        print("POSITION snapshot: %d B for %d splats" % (info["device_bytes"], m))
        assert info["device_bytes"] <= 16 * m + 4 * m and info["device_bytes"] <= 16 * (m + 3)
        assert r.transform(x) == m
        assert (er.bits(r.export_splats()) != er.bits(rec_a)).any()
        assert t.swap() == m
        held(r, rec_a, plane)
        same_frames(frames(r, u), fa)
    assert snapshots.take_selected_for(r, _abi.compose_xform(rot=(0.9, 0.1, 0.0, 0.3), scale=2.0)).info()["parts"] == POSITION | GEOMETRY | SH
    assert snapshots.take_selected_for(r, colours.compose(gain=(1.2, 1.0, 1.0))).info()["parts"] == SH
    assert snapshots.take_selected_for(r, colours.compose(opacity_gain=0.5)).info()["parts"] == GEOMETRY
    r.destroy()


@pytest.mark.gpu
def test_part_subsets():
    """Restoring only POSITION from a RECORD snapshot leaves the SH and the geometry at their edited values; a part that was not
    taken is refused and nothing changes."""
    from gsplat import _abi, colours, snapshots
    s, plane = base_scene()
    r = _mk(s, W, H, TS)
    r.write_state(plane)
    sel = np.flatnonzero(plane & SEL)
    rec_a = er.zero_padding(s)
    full = snapshots.take(r, SEL, SEL, RECORD)
    only_sh = snapshots.take(r, SEL, SEL, SH)
    r.transform(_abi.compose_xform(rot=(0.8, 0.2, 0.1, -0.4), translate=(1, 2, 3), scale=0.7))
    colours.tint(r, (1.1, 0.9, 0.8))
    rec_b = r.export_splats()
    for part in (POSITION, GEOMETRY, SH):
        assert (er.bits(rec_b)[np.ix_(sel, sn.floats_of(part))] != er.bits(rec_a)[np.ix_(sel, sn.floats_of(part))]).any()
    assert full.restore(POSITION) == sel.size
    want, _ = sn.written(rec_b, plane, sel, rec_a[sel], None, POSITION)
    held(r, want, plane)
    for s_, parts in ((only_sh, POSITION), (only_sh, RECORD), (full, STATE), (full, RECORD | STATE)):
        for call in (s_.restore, s_.swap):
            c, msg = code_of(lambda: call(parts))
            assert c == _abi.GS_ERR_INVALID_ARGUMENT and "not taken" in msg and "gs_snapshot_" in msg
    held(r, want, plane)
    assert only_sh.restore() == sel.size
    want, _ = sn.written(want, plane, sel, rec_a[sel], None, SH)
    held(r, want, plane)
    full.free()
    only_sh.free()
    r.destroy()


# ---- validity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_snapshot_validity():
    """A snapshot names splats by index: refused (serial) on another context, after an upload and after a compaction, the scene
    unchanged; still good after an insertion, whose new splats keep every bit; free() works after the context is gone."""
    import gsplat
    from gsplat import _abi, insert, snapshots
    L = _abi.load()
    n = 1025
    old = special_records(n)
    rec, plane = er.zero_padding(old), plane_of(n)
    sel = np.flatnonzero(plane & SEL)
    r = _mk(old, W, H, TS)
    r.write_state(plane)
    other = _mk(old, W, H, TS)
    other.write_state(plane)
    snap = snapshots.take(r, SEL, SEL, RECORD | STATE)
    dense = snapshots.take(r, 0, 0, POSITION)

    def refused(ctx_owner, s):
        for fn in (L.gs_snapshot_restore, L.gs_snapshot_swap):
            moved = ctypes.c_uint64(77)
            assert fn(ctx_owner._ctx, s._h, 0, ctypes.byref(moved)) == _abi.GS_ERR_INVALID_ARGUMENT
            msg = L.gs_last_error()
            assert b"serial" in msg and b"replaced or renumbered" in msg and b"gs_snapshot_" in msg, msg
            assert moved.value == 77

    refused(other, snap)
    held(other, rec, plane)
    # an insertion keeps the snapshot valid; the new splats are left alone
    tail = new_records(65, 3)
    assert insert.append(r, tail, 0xA4) == (n, 65)
    new, ns = new_records(sel.size, 9), new_states(sel.size, 9)
    snapshots.write(r, sel, new, ns, RECORD | STATE)
    assert snap.restore() == sel.size and dense.restore() == n
    held(r, np.concatenate([rec, er.zero_padding(tail)]), np.concatenate([plane, np.full(65, 0xA4, np.uint8)]))
    assert snap.info()["n_at_take"] == n and r.stats()["num_gaussians"] == n + 65
    # a compaction renumbers
    kept = r.compact(HID, 0)
    want_rec, want_plane = r.export_splats(), r.read_state()
    assert 0 < want_rec.shape[0] < n + 65 and kept.size == want_rec.shape[0]
    refused(r, snap)
    refused(r, dense)
    held(r, want_rec, want_plane)
    # ... and so does an upload, of the very same records
    fresh = snapshots.take(r, 0, 0, RECORD)
    _abi.check(L.gs_upload_splats(r._ctx, want_rec.ctypes.data, want_rec.shape[0]))
    refused(r, fresh)
    held(r, want_rec, np.zeros(want_rec.shape[0], np.uint8))
    empty = snapshots.take(r, 0xFF, 0xFF, RECORD | STATE)  # matches nothing: a valid object, restore and swap are no-ops
    assert empty.info() == {"count": 0, "n_at_take": want_rec.shape[0], "device_bytes": 0, "parts": RECORD | STATE, "dense": False}
    assert empty.restore() == 0 and empty.swap() == 0
    r.destroy()
    other.destroy()
    for s in (snap, dense, fresh, empty):
        assert s.info()["parts"]  # needs no context
        s.free()
        s.free()
        with pytest.raises(ValueError):
            s.info()


# ---- not a frame, not an upload -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_not_a_frame_and_not_an_upload():
    """Around a write and a restore: stats() (but the clocks), pick and the image read as before; frames in flight stay; the
    coverage, neighbour-count and cluster planes read back unchanged; with a captured frame graph the next frame is a replay that
    shows the written scene."""
    from gsplat import _abi, clusters, neighbours, snapshots
    u = uniforms()
    s, plane = base_scene()
    n = s.shape[0]
    ids = np.arange(0, n, 2, dtype=np.uint32)
    edited = s.copy()
    edited[ids, 0:3] += np.array([0.5, -0.25, 0.125], F)
    edited[ids, 16:19] = F(1.0) - edited[ids, 16:19]
    xy = np.array([(px, py) for py in range(3, H, 9) for px in range(5, W, 7)], np.uint32)
    fresh = _mk(edited, W, H, TS)
    fresh.write_state(plane)
    want = frames(fresh, u)
    fresh.destroy()
    r = _mk(s, W, H, TS)
    r.write_state(plane)
    old = frame_taps(r, u, False)
    assert (old["rgba8"] != want[0]["rgba8"]).any()
    r.accumulate_coverage()
    neighbours.count(r, 0.5, limit=8)
    clusters.label(r, 0.5)
    cover, neigh, clus = r.read_coverage(), neighbours.read(r), clusters.read(r)
    assert cover["hits"].any() and neigh.any() and (clus[1] > 1).any()
    st, picked = timeless(r.stats()), r.pick(xy)
    assert (picked["hit_count"] > 0).any()
    undo = snapshots.take(r, 0, 0, RECORD)
    for step in ("write", "restore", "write"):
        if step == "restore":
            assert undo.restore() == n
        else:
            assert snapshots.write(r, ids, edited[ids]) == ids.size
        np.testing.assert_array_equal(r.read_rgba8(), old["rgba8"])
        assert timeless(r.stats()) == st
        again = r.pick(xy)
        for f in picked.dtype.names:
            np.testing.assert_array_equal(again[f], picked[f], err_msg=f)
        after = r.read_coverage()
        for f in cover.dtype.names:
            np.testing.assert_array_equal(after[f], cover[f], err_msg=f)
        np.testing.assert_array_equal(neighbours.read(r), neigh)
        for a_, b_ in zip(clusters.read(r), clus):
            np.testing.assert_array_equal(a_, b_)
    same_frames(frames(r, u), want)
    undo.free()
    r.destroy()
    # frames in flight: three enqueued and not waited for, the call drains them and the ring stays
    r = _mk(s, W, H, TS)
    r.write_state(plane)
    for _ in range(3):
        r.render_uniforms(u)
    assert snapshots.write(r, ids, edited[ids]) == ids.size
    assert r.stats()["frames_in_flight"] == 3
    for _ in range(3):
        r.render_uniforms(u)
    r.wait()
    np.testing.assert_array_equal(r.read_rgba8(), want[0]["rgba8"])
    assert r.stats()["frames_in_flight"] == 3
    r.destroy()
    # a captured graph goes on replaying across a write and a restore
    g = _mk(s, W, H, TS)
    g.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    g.set_option(_abi.GS_OPT_FRAME_GRAPH, 1)
    g.write_state(plane)
    for _ in range(2):
        np.testing.assert_array_equal(frame_taps(g, u, False)["rgba8"], old["rgba8"])
    assert g.stats()["graph_frames"] == 2
    undo = snapshots.take(g, 0, 0, RECORD)
    assert snapshots.write(g, ids, edited[ids]) == ids.size
    np.testing.assert_array_equal(g.read_rgba8(), old["rgba8"])
    np.testing.assert_array_equal(frame_taps(g, u, False)["rgba8"], want[0]["rgba8"])
    assert g.stats()["graph_frames"] == 3
    assert undo.restore() == n
    np.testing.assert_array_equal(frame_taps(g, u, False)["rgba8"], old["rgba8"])
    assert g.stats()["graph_frames"] == 4
    undo.free()
    g.destroy()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_are_atomic():
    """Every refusal returns its code with a message that names the call, and the export and the plane are bit-identical
    afterwards; parts == 0 and m == 0 are GS_OK no-ops."""
    import torch
    from gsplat import _abi, snapshots
    L = _abi.load()
    n = 1025
    old = special_records(n)
    rec, plane = er.zero_padding(old), plane_of(n)
    r = _mk(old, W, H, TS)
    r.write_state(plane)
    new, ns = new_records(n + 1, 1), new_states(n + 1, 1)
    bad_lists = {"descending": ([3, 9, 8, 20], b"ids[2] = 8", b"ids[1] = 9"), "duplicate": ([0, 5, 5, 7], b"ids[2] = 5", b"ids[1] = 5"),
                 "no splat": ([1, 2, n], b"ids[2] = %d" % n, b"N = %d" % n), "first no splat": ([n + 7], b"ids[0] = %d" % (n + 7), b"N = %d" % n),
                 "late": (list(range(0, 600)) + [599], b"ids[600] = 599", b"ids[599] = 599")}
    for name, (lst, w1, w2) in bad_lists.items():
        ids = np.array(lst, np.uint32)
        for device in (False, True):
            if device:
                t_ids, t_rec = torch.from_numpy(ids.view(np.int32).copy()).cuda(), torch.from_numpy(new[:ids.size]).cuda()
                t_st = torch.from_numpy(ns[:ids.size]).cuda()
                c, msg = code_of(lambda: snapshots.write(r, t_ids, t_rec, t_st, RECORD | STATE))
            else:
                c, msg = code_of(lambda: snapshots.write(r, ids, new[:ids.size], ns[:ids.size], RECORD | STATE))
            who = "gs_write_splats_device" if device else "gs_write_splats"
            assert c == _abi.GS_ERR_INVALID_ARGUMENT and who + ":" in msg, (name, msg)
            assert w1.decode() in msg and w2.decode() in msg, (name, msg)
            held(r, rec, plane)
    # m > N with ids == NULL, host and device
    c, msg = code_of(lambda: snapshots.write(r, None, new, ns, RECORD | STATE))
    assert c == _abi.GS_ERR_INVALID_ARGUMENT and "gs_write_splats:" in msg and str(n + 1) in msg
    c, msg = code_of(lambda: snapshots.write(r, None, torch.from_numpy(new).cuda(), None, RECORD))
    assert c == _abi.GS_ERR_INVALID_ARGUMENT and "gs_write_splats_device:" in msg
    # filters and parts that fit nothing
    written = ctypes.c_uint64(77)
    h = ctypes.c_void_p(78)
    for mask, value in ((0x100, 0), (0, 0x100)):
        assert L.gs_snapshot_take(r._ctx, mask, value, RECORD, ctypes.byref(h)) == _abi.GS_ERR_INVALID_ARGUMENT
        assert b"gs_snapshot_take:" in L.gs_last_error() and b"state byte" in L.gs_last_error()
    assert L.gs_snapshot_take(r._ctx, 0, 0, 0x17, ctypes.byref(h)) == _abi.GS_ERR_INVALID_ARGUMENT
    assert L.gs_write_splats(r._ctx, None, 1, new.ctypes.data, None, 0x20, ctypes.byref(written)) == _abi.GS_ERR_INVALID_ARGUMENT
    assert L.gs_write_splats(r._ctx, None, 1, new.ctypes.data, None, RECORD | STATE, ctypes.byref(written)) == _abi.GS_ERR_INVALID_ARGUMENT
    assert b"null states" in L.gs_last_error()
    assert h.value == 78 and written.value == 77
    held(r, rec, plane)
    # no-ops: parts == 0 and m == 0 (null pointers are then accepted)
    assert snapshots.write(r, np.arange(4), new[:4], ns[:4], 0) == 0
    assert snapshots.write(r, None, new[:0], None, RECORD) == 0
    assert L.gs_write_splats(r._ctx, None, 0, None, None, RECORD | STATE, None) == 0
    assert L.gs_write_splats_device(r._ctx, None, 0, None, None, RECORD | STATE, ctypes.byref(written)) == 0 and written.value == 0
    held(r, rec, plane)
    # a borrower: all five calls refuse, the owner's scene stays
    snap = snapshots.take(r, SEL, SEL, RECORD | STATE)
    b = _mk(old, W, H, TS, share_with=r)
    calls = {"gs_write_splats": lambda: snapshots.write(b, None, new[:4], None, POSITION),
             "gs_write_splats_device": lambda: snapshots.write(b, None, torch.from_numpy(new[:4]).cuda(), None, POSITION),
             "gs_snapshot_take": lambda: snapshots.take(b, 0, 0, POSITION),
             "gs_snapshot_restore": lambda: _abi.check(L.gs_snapshot_restore(b._ctx, snap._h, 0, None)),
             "gs_snapshot_swap": lambda: _abi.check(L.gs_snapshot_swap(b._ctx, snap._h, 0, None))}
    for who, call in calls.items():
        c, msg = code_of(call)
        assert c == _abi.GS_ERR_INVALID_ARGUMENT and who + ":" in msg and "owner" in msg, msg
    held(r, rec, plane)
    b.destroy()
    snap.free()
    r.destroy()
    # without GS_FLAG_SPLAT_STATE: (0, 0) and the record parts work, any other filter and GS_PART_STATE are refused as the state calls refuse
    p = _mk(old, W, H, TS, state=False)
    for call, who in ((lambda: snapshots.take(p, SEL, SEL, RECORD), "gs_snapshot_take"), (lambda: snapshots.take(p, 0, 0, STATE), "gs_snapshot_take"),
                      (lambda: snapshots.write(p, None, new[:4], ns[:4], RECORD | STATE), "gs_write_splats")):
        c, msg = code_of(call)
        assert c == _abi.GS_ERR_INVALID_ARGUMENT and who + ":" in msg and "GS_FLAG_SPLAT_STATE" in msg, msg
    held(p, rec, None)
    with snapshots.take(p, 0, 0, RECORD) as s:
        assert snapshots.write(p, np.array([0, n - 1]), new[:2], None, RECORD) == 2
        assert s.info()["dense"] and s.swap() == n
        held(p, rec, None)
    p.destroy()
    # before any upload: GS_ERR_NO_SCENE
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size = ctypes.sizeof(_abi.GsConfig), W, H, TS
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    assert L.gs_write_splats(ctx, None, 1, new.ctypes.data, None, RECORD, None) == _abi.GS_ERR_NO_SCENE
    assert b"gs_write_splats:" in L.gs_last_error()
    assert L.gs_snapshot_take(ctx, 0, 0, RECORD, ctypes.byref(h)) == _abi.GS_ERR_NO_SCENE and h.value == 78
    _abi.check(L.gs_destroy(ctx))


# ---- PipelinedRenderer -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pipelined_renderer_undo():
    """A take, an edit and a restore through the owner while frames are in flight: every member's next frame equals the pre-edit
    frame; the members read the owner's planes, so nothing is shared again and numGaussians is unchanged."""
    import gsplat
    from gsplat import _abi, colours, snapshots
    u = uniforms()
    s, plane = base_scene()
    n = s.shape[0]
    p = gsplat.PipelinedRenderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(s), TS, frames_in_flight=3,
                                 flags=_abi.GS_FLAG_EXACT_BLEND | _abi.GS_FLAG_F32_TAP | _abi.GS_FLAG_SPLAT_STATE)
    p.write_state(plane)
    slot = p.render_uniforms(u)
    before = p.read_rgba8(slot).copy()
    assert before[..., :3].any()
    p.render_uniforms(u)  # in flight when the calls come
    undo = snapshots.take(p, SEL, SEL, RECORD)
    m = undo.info()["count"]
    assert m == int((plane & SEL != 0).sum())
    assert p.rotate_selected((0.7, 0.1, 0.6, 0.2)) == m and colours.brighten(p, 1.5) == m
    edited = []
    for slot in [p.render_uniforms(u) for _ in range(3)]:
        edited.append(p.read_rgba8(slot).copy())
    assert all((e == edited[0]).all() for e in edited) and (edited[0] != before).any()
    p.render_uniforms(u)
    assert undo.restore() == m
    slots = [p.render_uniforms(u) for _ in range(3)]
    assert sorted(slots) == [0, 1, 2]
    for slot in slots:
        np.testing.assert_array_equal(p.read_rgba8(slot), before)
        assert p.renderers[slot].numGaussians == n == p.renderers[slot].stats()["num_gaussians"]
    np.testing.assert_array_equal(er.bits(p.export_splats()), er.bits(er.zero_padding(s)))
    undo.free()
    p.destroy()
