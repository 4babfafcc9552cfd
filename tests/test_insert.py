"""Splat insertion: append records, a .ply or a copy of a selection to the resident splats (include/gsplat/gs_abi.h "splat
insertion").

The reference every answer is held to is tests/insert_restate.py: the records are old ++ new with the 21 padding floats zeroed, the
state plane is old ++ m x new_state, a duplicate's new records are the ascending matches of its filter.  Every float comparison is
on the uint32 view; the only tolerance is gpu_checks.check_image for fused frames, used as it stands.  An insertion is held to the
definition the header gives it: the context must be indistinguishable from a fresh one given gs_upload_splats(old ++ new) +
gs_state_write(old bytes ++ m x new_state) -- every tap and the image, bit for bit.
"""
import ctypes
import functools
import inspect

import numpy as np
import pytest

from conftest import scene
import cluster_restate as cr
import export_restate as er
import grade_restate as gr
import insert_restate as ir
import neigh_restate as nr
import state_restate as sr
import xform_restate as xr
from support import (F, FRAME_CASES, SLAB_COLS, TAPS, cached, code_of, frame_taps, guarded, host_sources, is_fill, mk, raw_export,
                     special_records, state_scene)

_mk = functools.partial(mk, exact=True, state=True)
HID, SEL = er.HIDDEN, er.SELECTED
SYMBOLS = ("gs_append_splats", "gs_append_splats_device", "gs_append_ply", "gs_duplicate_splats")
NEW = 0xA6  # selected, not hidden, host bits 2, 5 and 7
# (N, m): N mod 4 and m mod 4 in {0, 1, 2, 3}; sums that stay under, land on and cross a multiple of 64 (the plane stride); the
# 1024-splat select block crossed by N, by m and by both
MARGINS = [(0, 1), (1, 1), (3, 5), (5, 3), (62, 1), (63, 2), (64, 64), (65, 1023), (1023, 1), (1025, 4), (3001, 1025)]
DUP = (0x3, 0x1)  # the duplicate's filter: every third splat of old_plane


_NO_DUP = np.array([v for v in range(256) if v & 3 != 1], np.uint8)


def old_plane(n):
    """State bytes of every value mod 256 (once n allows), dealt so that exactly every third splat passes DUP: splat 3 j + 1 gets
    the j-th of the 64 bytes with low bits 01 (in steps of 5 of them), the others run through the 192 other bytes (in steps of 37)."""
    i = np.arange(n)
    hit = i % 3 == 1
    dup = ((i // 3 * 20) & 0xFC) | 1
    rank = np.cumsum(~hit) - 1
    return np.where(hit, dup, _NO_DUP[(rank * 37) % 192]).astype(np.uint8)


def margin_records(n, m):
    """(old, new): the first n and the last m of n + m special records."""
    base = special_records(n + m)
    return np.ascontiguousarray(base[:n]), np.ascontiguousarray(base[n:])


def held(r, want_rec, want_state):
    """The context holds exactly these records and state bytes (guarded export, uint32 view)."""
    got, ids = raw_export(r, 0, 0, True)
    np.testing.assert_array_equal(er.bits(got), er.bits(want_rec))
    np.testing.assert_array_equal(ids, np.arange(want_rec.shape[0], dtype=np.uint32))
    if want_state is not None:
        np.testing.assert_array_equal(r.read_state(), want_state)
    assert r.numGaussians == want_rec.shape[0] == r.stats()["num_gaussians"]


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_insert_abi():
    """The four symbols are exported without a GPU and listed; the ABI version stays 3; a null context and a null path are refused
    with a message that names the call; a new_state that is no byte is refused; the header section sits behind the splat edits."""
    from gsplat import _abi
    L = _abi.load()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    assert L.gs_abi_version() == 3
    first, m = ctypes.c_uint64(77), ctypes.c_uint64(78)
    rec = np.zeros((1, 80), F)
    for call, who in ((lambda s: L.gs_append_splats(None, rec.ctypes.data, 1, s, ctypes.byref(first)), b"gs_append_splats"),
                      (lambda s: L.gs_append_splats_device(None, None, 0, s, ctypes.byref(first)), b"gs_append_splats_device"),
                      (lambda s: L.gs_append_ply(None, b"x.ply", s, ctypes.byref(first), ctypes.byref(m)), b"gs_append_ply"),
                      (lambda s: L.gs_duplicate_splats(None, 0, 0, s, ctypes.byref(first), ctypes.byref(m), None), b"gs_duplicate_splats")):
        assert call(0) == _abi.GS_ERR_INVALID_ARGUMENT
        assert who + b":" in L.gs_last_error() and b"null" in L.gs_last_error()
        assert call(0x100) == _abi.GS_ERR_INVALID_ARGUMENT
        assert who + b":" in L.gs_last_error() and b"new_state" in L.gs_last_error()
    assert L.gs_append_ply(None, None, 0, ctypes.byref(first), ctypes.byref(m)) == _abi.GS_ERR_INVALID_ARGUMENT
    assert b"gs_append_ply: null path" in L.gs_last_error()
    assert L.gs_append_splats(None, None, 1, 0, ctypes.byref(first)) == _abi.GS_ERR_INVALID_ARGUMENT
    assert b"gs_append_splats: null records" in L.gs_last_error()
    assert first.value == 77 and m.value == 78
    hdr = host_sources().hdr
    for name in SYMBOLS:
        assert "int32_t %s(gs_ctx* ctx" % name in hdr
    assert "#define GS_ABI_VERSION 3\n" in hdr
    assert hdr.index("---- splat edits") < hdr.index("---- splat insertion") < hdr.index("---- splat transforms")
    sec = hdr[hdr.index("---- splat insertion"):hdr.index("---- splat transforms")]
    for words in ("245 B x (2 N + m)", "ASCENDING source index", "out of scope", "GS_ERR_NO_FRAME", "BESIDE", "no-op"):
        assert words in sec, words


def test_insert_module_surface():
    """gsplat.insert is a module of free functions with the stated signatures; the host classes are untouched (test_abi pins them)."""
    import gsplat
    from gsplat import insert
    assert gsplat.insert is insert
    want = {"append": "(r, records, state=0)", "append_ply": "(r, path, state=0)", "duplicate": "(r, mask, value, state=0)",
            "merge_ply": "(r, path)", "duplicate_selected": "(r, xform=None)"}
    live = {n: str(inspect.signature(f)) for n, f in vars(insert).items()
            if inspect.isfunction(f) and f.__module__ == insert.__name__ and not n.startswith("_")}
    assert live == want
    for n in want:
        assert getattr(insert, n).__doc__


def test_restatement_agrees_with_the_export():
    """insert_restate on records with NaN payloads, -0 and infinities: an append is the export of the concatenation, a duplicate's
    tail is the export of its filter, both bit for bit."""
    for n, m in ((5, 3), (65, 1023), (3001, 1025)):
        old, new = margin_records(n, m)
        plane = old_plane(n)
        rec, state, first, count = ir.appended(old, plane, new, NEW)
        both = np.concatenate([old, new])
        assert (first, count) == (n, m) and rec.shape == (n + m, 80) and state.shape == (n + m,)
        np.testing.assert_array_equal(er.bits(rec), er.bits(er.records(both, np.zeros(n + m, np.uint8), 0, 0)))
        assert not er.bits(rec)[:, er.PADDING].any() and er.bits(both)[:, er.PADDING].any()
        np.testing.assert_array_equal(er.bits(rec)[:, er.CARRIED], er.bits(both)[:, er.CARRIED])
        np.testing.assert_array_equal(state[:n], plane)
        assert (state[n:] == NEW).all()
        drec, dstate, dfirst, dcount, ids = ir.duplicated(old, plane, *DUP, NEW)
        np.testing.assert_array_equal(ids, er.ids_of(plane, *DUP))
        assert (dfirst, dcount) == (n, ids.size) and (np.diff(ids.astype(np.int64)) > 0).all()
        assert abs(ids.size - n / 3.0) <= 1
        np.testing.assert_array_equal(er.bits(drec[n:]), er.bits(er.records(old, plane, *DUP)))
        np.testing.assert_array_equal(er.bits(drec[:n]), er.bits(er.zero_padding(old)))
        np.testing.assert_array_equal(dstate, np.concatenate([plane, np.full(ids.size, NEW, np.uint8)]))
    assert not np.isfinite(special_records(3001 + 1025)).all()
    assert sorted(set(old_plane(1025).tolist())) == list(range(256))


# ---- GPU: the kernels at their margins ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,m", MARGINS, ids=["%d+%d" % p for p in MARGINS])
def test_insert_kernels_at_their_margins(n, m):
    """append, append from a device tensor and duplicate on special records over old state bytes of every value: the export of
    everything, the state plane and the returned first / count / ids equal the restatement; the guards behind the outputs are
    intact."""
    import torch
    from gsplat import _abi, insert
    L = _abi.load()
    old, new = margin_records(n, m)
    plane = old_plane(n)
    want_rec, want_state, _, _ = ir.appended(old, plane, new, NEW)
    for device in (False, True):
        r = _mk(old, 64, 64, 8)
        r.write_state(plane)
        src = torch.from_numpy(new).cuda() if device else new
        assert insert.append(r, src, NEW) == (n, m)
        held(r, want_rec, want_state)
        r.destroy()
    # the duplicate, through the C call with a guarded id buffer
    drec, dstate, _, dcount, dids = ir.duplicated(old, plane, *DUP, NEW)
    r = _mk(old, 64, 64, 8)
    r.write_state(plane)
    ids = guarded(n + 1, np.uint32)
    first, cnt = ctypes.c_uint64(99), ctypes.c_uint64(99)
    _abi.check(L.gs_duplicate_splats(r._ctx, DUP[0], DUP[1], NEW, ctypes.byref(first), ctypes.byref(cnt), ids.ctypes.data))
    assert (first.value, cnt.value) == (n, dcount)
    np.testing.assert_array_equal(ids[:dcount], dids)
    assert is_fill(ids[dcount:])
    r.numGaussians = n + dcount
    held(r, drec, dstate)
    # ... and once more on what is resident now, through the module, with every splat ((0, 0)) and another byte
    if 0 < n <= 1025:
        n2 = n + dcount
        assert insert.duplicate(r, 0, 0, 0x41)[:2] == (n2, n2)
        held(r, np.concatenate([drec, drec]), np.concatenate([dstate, np.full(n2, 0x41, np.uint8)]))
    r.destroy()


# ---- insertion is a concatenated upload --------------------------------------------------------------------------------------------
def _split(name):
    """(head, tail, plane of the head, k): the scene split at an odd index; hidden and selected splats and host bits in the plane."""
    def make():
        s = state_scene(name)[0]
        n = s.shape[0]
        k = (n // 2) | 1
        i = np.arange(k)
        host = (np.random.default_rng(41).integers(0, 64, k, dtype=np.uint8) << 2).astype(np.uint8)
        plane = host | np.where(i % 7 == 3, HID, 0).astype(np.uint8) | np.where(i % 3 == 1, SEL, 0).astype(np.uint8)
        return np.ascontiguousarray(s[:k]), np.ascontiguousarray(s[k:]), plane, k
    return cached(("insert_split", name), make)


def _same_frames(oracle, r, fresh, u, exact, ref_key, ref_make, lit=True):
    """The next frames of r (both binnings) equal those of the fresh context: every tap; the image bit for bit in EXACT mode, else
    against the oracle's frame of the concatenated scene."""
    from gpu_checks import check_image
    for debug in (False, True):
        a, b = frame_taps(r, u, debug), frame_taps(fresh, u, debug)
        for t in TAPS:
            np.testing.assert_array_equal(a[t], b[t], err_msg="%s debug=%s" % (t, debug))
        if exact:
            np.testing.assert_array_equal(a["rgba8"], b["rgba8"])
            np.testing.assert_array_equal(a["rgbf"], b["rgbf"])
        else:
            check_image(r, cached(ref_key, ref_make), False)
    assert a["rgba8"][..., :3].any() or not lit


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fused"])
@pytest.mark.parametrize("case", FRAME_CASES, ids=lambda c: "%s-t%d" % c)
def test_insertion_is_a_concatenated_upload(oracle, case, exact):
    from gsplat import insert
    name, ts = case
    s, u, W, H = state_scene(name)
    head, tail, plane, k = _split(name)
    n = s.shape[0]
    assert k % 2 == 1 and 0 < k < n
    full = np.concatenate([plane, np.full(n - k, NEW, np.uint8)])

    def ref_of(rec, st):
        return lambda: sr.state_frame(oracle, rec, u, W, H, ts, st, want_illcond=True)

    # append: upload the head, render one frame, append the tail
    for cols in (None, SLAB_COLS[ts]) if exact else (None,):
        r = _mk(head, W, H, ts, exact=exact, cols=cols)
        r.write_state(plane)
        frame_taps(r, u, False)
        assert insert.append(r, tail, NEW) == (k, n - k)
        held(r, er.zero_padding(s), full)
        fresh = _mk(s, W, H, ts, exact=exact, cols=cols)
        fresh.write_state(full)
        _same_frames(oracle, r, fresh, u, exact, ("insert_ref", name, ts, "append"), ref_of(s, full), lit=cols is None)
        fresh.destroy()
        r.destroy()
    # duplicate the selected visible splats of the head
    filt = (SEL | HID, SEL)
    drec, dstate, _, dcount, dids = ir.duplicated(head, plane, *filt, NEW)
    assert 0 < dcount < k
    r = _mk(head, W, H, ts, exact=exact)
    r.write_state(plane)
    frame_taps(r, u, False)
    first, count, ids = insert.duplicate(r, *filt, NEW)
    assert (first, count) == (k, dcount)
    np.testing.assert_array_equal(ids, dids)
    both = np.concatenate([head, head[dids]])
    fresh = _mk(both, W, H, ts, exact=exact)
    fresh.write_state(dstate)
    held(r, drec, dstate)
    _same_frames(oracle, r, fresh, u, exact, ("insert_ref", name, ts, "dup"), ref_of(both, dstate))
    fresh.destroy()
    r.destroy()
    # ... and every splat of a context without the state plane (new_state is 0 there)
    r = _mk(head, W, H, ts, exact=exact, state=False)
    frame_taps(r, u, False)
    first, count, ids = insert.duplicate(r, 0, 0)
    assert (first, count) == (k, k)
    np.testing.assert_array_equal(ids, np.arange(k, dtype=np.uint32))
    twice = np.concatenate([head, head])
    fresh = _mk(twice, W, H, ts, exact=exact, state=False)
    held(r, er.zero_padding(twice), None)
    _same_frames(oracle, r, fresh, u, exact, ("insert_ref", name, ts, "dup_unflagged"), ref_of(twice, np.zeros(2 * k, np.uint8)))
    fresh.destroy()
    r.destroy()


# ---- frame paths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_insertion_on_frame_paths(oracle):
    """Frames in flight, a captured frame graph and PipelinedRenderer."""
    import gsplat
    from gpu_checks import check_image
    from gsplat import _abi, insert
    name, ts = "cfgA", 16
    s, u, W, H = state_scene(name)
    head, tail, plane, k = _split(name)
    n = s.shape[0]
    full = np.concatenate([plane, np.full(n - k, NEW, np.uint8)])
    ref = cached(("insert_ref_exact", name, ts), lambda: sr.state_frame(oracle, s, u, W, H, ts, full))
    # three frames enqueued and not waited for: the call drains them
    r = _mk(head, W, H, ts)
    r.write_state(plane)
    for _ in range(3):
        r.render_uniforms(u)
    assert insert.append(r, tail, NEW) == (k, n - k)
    for _ in range(3):
        r.render_uniforms(u)
    check_image(r, ref, True)
    st = r.stats()
    assert st["num_gaussians"] == n and st["frames_in_flight"] == 3
    r.destroy()
    # a captured graph: it is recaptured, the frame after the insertion is right and graph_frames goes on counting
    g = _mk(head, W, H, ts)
    g.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    g.set_option(_abi.GS_OPT_FRAME_GRAPH, 1)
    g.write_state(plane)
    for _ in range(2):
        g.render_uniforms(u)
        g.wait()
    assert g.stats()["graph_frames"] == 2
    assert insert.append(g, tail, NEW) == (k, n - k)
    for _ in range(2):
        g.render_uniforms(u)
        g.wait()
        check_image(g, ref, True)
    assert g.stats()["graph_frames"] == 4 and g.stats()["num_gaussians"] == n
    g.destroy()
    # PipelinedRenderer: the owner grows, the module makes the other members share again; every slot renders the merged scene
    p = gsplat.PipelinedRenderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(head), ts, frames_in_flight=3,
                                 flags=_abi.GS_FLAG_EXACT_BLEND | _abi.GS_FLAG_F32_TAP | _abi.GS_FLAG_SPLAT_STATE)
    p.render_uniforms(u)  # in flight when the calls come
    p.write_state(plane)
    p.render_uniforms(u)
    assert insert.append(p, tail, NEW) == (k, n - k)
    np.testing.assert_array_equal(p.list_state(0, 0), np.arange(n, dtype=np.uint32))
    np.testing.assert_array_equal(p.read_state(), full)
    slots = [p.render_uniforms(u) for _ in range(3)]
    assert sorted(slots) == [0, 1, 2]
    for slot in slots:
        p.wait(slot)
        check_image(p.renderers[slot], ref, True)
        assert p.renderers[slot].stats()["num_gaussians"] == n == p.renderers[slot].numGaussians
    p.destroy()


@pytest.mark.gpu
def test_pick_after_insertion(oracle):
    """gs_pick needs a new frame after an insertion; it then names the new indices too."""
    from gsplat import _abi, insert
    from pick_restate import restate_ref
    name, ts = "cfgA", 16
    s, u, W, H = state_scene(name)
    head, tail, _, k = _split(name)
    xy = np.array([(x, y) for y in range(3, H, 17) for x in range(5, W, 13)], np.uint32)
    r = _mk(head, W, H, ts, state=False)
    r.render_uniforms(u)
    r.wait()
    r.pick(xy)
    assert insert.append(r, tail) == (k, s.shape[0] - k)
    assert code_of(lambda: r.pick(xy))[0] == _abi.GS_ERR_NO_FRAME
    assert code_of(lambda: r.read_rgba8())[0] == _abi.GS_ERR_NO_FRAME
    assert code_of(lambda: r.read_buffer(_abi.GS_BUF_VALUES))[0] == _abi.GS_ERR_NO_FRAME
    r.render_uniforms(u)
    r.wait()
    ref = cached(("insert_pick_ref", name, ts), lambda: oracle.render(s, u, W, H, ts))
    want = restate_ref(ref, W, H, ts, xy)[0]
    got = r.pick(xy)
    for f in ("first_id", "max_id", "median_id", "hit_count"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    hit = got["hit_count"] > 0
    assert (got["first_id"][hit] >= k).any() and (got["first_id"][hit] < k).any()
    r.destroy()


# ---- .ply ------------------------------------------------------------------------------------------------------------------------
def _shuffled_uchar_ply(path, rec):
    """Degree 1, a property order of its own, a property the packer does not use and the opacity as a uchar: vertices of 93 bytes.
    Returns the records gs_ply_load must make of it."""
    rec = np.array(rec, F, copy=True)
    n = rec.shape[0]
    rec.view(np.uint32)[:, er.PADDING] = 0
    rec[:, 16 + 4 * 4:16 + 4 * 16] = 0.0
    op_u8 = ((np.arange(n) * 29 + 5) % 256).astype(np.uint8)
    rec[:, 12] = (op_u8.astype(np.float64) / 255.0).astype(F)
    names = ["rot_0", "rot_1", "rot_2", "rot_3", "x", "y", "z", "nx", "scale_0", "scale_1", "scale_2", "f_dc_0", "f_dc_1", "f_dc_2"] + \
            ["f_rest_%d" % i for i in range(9)]
    cols = {"rot_0": rec[:, 8], "rot_1": rec[:, 9], "rot_2": rec[:, 10], "rot_3": rec[:, 11], "x": rec[:, 0], "y": rec[:, 1], "z": rec[:, 2],
            "nx": np.zeros(n, F), "scale_0": rec[:, 4], "scale_1": rec[:, 5], "scale_2": rec[:, 6]}
    for c in range(3):
        cols["f_dc_%d" % c] = rec[:, 16 + c]
        for i in range(3):
            cols["f_rest_%d" % (c * 3 + i)] = rec[:, 16 + 4 * (i + 1) + c]
    dt = np.dtype([(nm, "<f4") for nm in names] + [("opacity", "u1")], align=False)
    arr = np.zeros(n, dtype=dt)
    for nm in names:
        arr[nm] = cols[nm]
    arr["opacity"] = op_u8
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n + "".join("property float %s\n" % nm for nm in names) +
                 "property uchar opacity\nend_header\n").encode())
        f.write(arr.tobytes())
    return rec


@pytest.mark.gpu
def test_append_ply(tmp_path):
    """append_ply equals gs_ply_load + append: files of degree 3 and 0 written by save_ply, 65 537 vertices onto N = 5 (a second
    chunk of one vertex, at an offset that is no multiple of anything), a uchar property in a shuffled property order."""
    from gsplat import _abi, insert
    old, new = margin_records(5, 70)
    plane = old_plane(5)
    for degree in (3, 0):
        path = str(tmp_path / ("d%d.ply" % degree))
        _abi.save_ply(path, new, degree)
        loaded, deg = _abi.load_ply(path)
        assert deg == degree and (degree == 3 or not er.bits(loaded)[:, 20:].any())
        np.testing.assert_array_equal(er.bits(loaded), er.bits(er.truncate_degree(er.zero_padding(new), degree)))
        want_rec, want_state, _, _ = ir.appended(old, plane, loaded, NEW)
        r, r2 = _mk(old, 64, 64, 8), _mk(old, 64, 64, 8)
        for x in (r, r2):
            x.write_state(plane)
        assert insert.append_ply(r, path, NEW) == (5, 70)
        assert insert.append(r2, loaded, NEW) == (5, 70)
        held(r, want_rec, want_state)
        held(r2, want_rec, want_state)
        r.destroy()
        r2.destroy()
    # one vertex more than a chunk
    n = 65537
    big = np.tile(special_records(10000), (7, 1))[:n].copy()
    big[:, 1] += np.arange(n, dtype=F)  # every record distinct
    pb = str(tmp_path / "big.ply")
    _abi.save_ply(pb, big, 3)
    r = _mk(old, 64, 64, 8)
    r.write_state(plane)
    assert insert.append_ply(r, pb, NEW) == (5, n)
    want_rec, want_state, _, _ = ir.appended(old, plane, big, NEW)
    held(r, want_rec, want_state)
    r.destroy()
    # uchar, shuffled, degree 1, unaligned floats; onto a context without the state plane
    ps = str(tmp_path / "odd.ply")
    want_new = _shuffled_uchar_ply(ps, special_records(300))
    loaded, deg = _abi.load_ply(ps)
    assert deg == 1
    np.testing.assert_array_equal(er.bits(loaded), er.bits(want_new))
    r = _mk(old, 64, 64, 8, state=False)
    assert insert.append_ply(r, ps) == (5, 300)
    held(r, ir.appended(old, plane, loaded, 0)[0], None)
    r.destroy()


@pytest.mark.gpu
def test_append_ply_three_trips(tmp_path):
    """A .ply of 131 329 = 2 x 65 536 + 257 vertices behind 300 resident splats: three trips of the stream, so its first staging
    buffers are used again after the wait for the trip two before, and a last trip of 257.  The context equals one built by
    insert.append of the records (the same ones tests/test_packed.py appends packed): records, ids, first, state bytes, splat count."""
    from gsplat import _abi, insert, synth
    n = 2 * 65536 + 257
    big = cached(("packed_plain", n), lambda: synth.bicycle_like(n))
    old, plane = np.ascontiguousarray(scene(10000)[:300]), old_plane(300)
    path = str(tmp_path / "three.ply")
    _abi.save_ply(path, big, 3)
    r, fresh = _mk(old, 64, 64, 8), _mk(old, 64, 64, 8)
    for x in (r, fresh):
        x.write_state(plane)
    assert insert.append_ply(r, path, NEW) == (300, n) == insert.append(fresh, big, NEW)
    want_rec, want_state, _, _ = ir.appended(old, plane, big, NEW)
    held(r, want_rec, want_state)
    held(fresh, want_rec, want_state)
    fresh.destroy()
    r.destroy()


# ---- rules -----------------------------------------------------------------------------------------------------------------------
def _header_only_ply(path, n, names):
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n + "".join("property float %s\n" % nm for nm in names) +
                 "end_header\n").encode())
        f.write(np.zeros((n, len(names)), "<f4").tobytes())


@pytest.mark.gpu
def test_no_ops_and_refusals(tmp_path):
    """m == 0 in all three forms changes nothing and keeps the last frame readable; after every refused call the export and the
    state plane are byte-equal to before and the last frame is still readable."""
    import torch
    from gpu_checks import orbit_uniforms
    from gsplat import _abi, insert
    L = _abi.load()
    rec = scene(10000)[:2001]
    n, W, H, ts = rec.shape[0], 128, 128, 16
    u = orbit_uniforms(W, H)
    plane = old_plane(n) & np.uint8(0x7E)  # nothing hidden; no byte has bit 7, so a filter on it matches nothing
    r = _mk(rec, W, H, ts)
    r.write_state(plane)
    r.render_uniforms(u)
    r.wait()
    img = r.read_rgba8()
    vals = r.read_buffer(_abi.GS_BUF_VALUES)
    cap = r.stats()["capacity"], r.stats()["row_capacity"]
    assert img[..., :3].any()

    def unchanged():
        np.testing.assert_array_equal(r.read_rgba8(), img)  # the last frame is readable
        np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_VALUES), vals)
        r.pick(np.array([[5, 5]], np.uint32))
        held(r, er.zero_padding(rec), plane)
        st = r.stats()
        assert (st["capacity"], st["row_capacity"]) == cap

    all_names = er.ply_columns(rec[:1], 3)[0]
    empty = str(tmp_path / "empty.ply")
    _abi.save_ply(empty, np.zeros((0, 80), F), 3)
    assert insert.append(r, np.zeros((0, 80), F), NEW) == (n, 0)
    unchanged()
    assert insert.append(r, torch.zeros((0, 80), dtype=torch.float32, device="cuda"), NEW) == (n, 0)
    unchanged()
    assert insert.append_ply(r, empty, NEW) == (n, 0)
    unchanged()
    first, count, ids = insert.duplicate(r, 0x80, 0x80, NEW)
    assert (first, count, ids.size) == (n, 0, 0) and not (plane & 0x80).any()
    unchanged()
    # refusals
    missing = str(tmp_path / "no_such.ply")
    truncated = str(tmp_path / "truncated.ply")
    _abi.save_ply(truncated, rec[:100], 3)
    raw = open(truncated, "rb").read()
    open(truncated, "wb").write(raw[:-1])
    no_pos = str(tmp_path / "no_positions.ply")
    _header_only_ply(no_pos, 4, [nm for nm in all_names if nm not in ("x", "y", "z")])
    one = np.ascontiguousarray(rec[:1])
    first = ctypes.c_uint64(77)
    refused = [(lambda: insert.append(r, one, 0x100), "new_state"),
               (lambda: insert.duplicate(r, 0x100, 0, 0), "filter"),
               (lambda: insert.duplicate(r, 0, 0x1FF, 0), "filter"),
               (lambda: _abi.check(L.gs_append_splats(r._ctx, one.ctypes.data, 2 ** 31, 0, ctypes.byref(first))), "2^31"),
               (lambda: _abi.check(L.gs_append_splats(r._ctx, one.ctypes.data, 2 ** 31 - n, 0, ctypes.byref(first))), "2^31"),
               (lambda: insert.append_ply(r, missing, NEW), "cannot open"),
               (lambda: insert.append_ply(r, truncated, NEW), "truncated"),
               (lambda: insert.append_ply(r, no_pos, NEW), "missing property x")]
    for fn, words in refused:
        c, msg = code_of(fn)
        assert c == _abi.GS_ERR_INVALID_ARGUMENT and words in msg, msg
        unchanged()
    assert first.value == 77
    # a borrower is refused, in every form; its own frame and the owner's stay
    b = _mk(rec, W, H, ts, share_with=r)
    b.render_uniforms(u)
    b.wait()
    np.testing.assert_array_equal(b.read_rgba8(), img)
    for fn in (lambda: insert.append(b, one, 0), lambda: insert.append_ply(b, empty, 0), lambda: insert.duplicate(b, 0, 0, 0)):
        c, msg = code_of(fn)
        assert c == _abi.GS_ERR_INVALID_ARGUMENT and "owner" in msg
        np.testing.assert_array_equal(b.read_rgba8(), img)
        unchanged()
    b.destroy()
    r.destroy()
    # a non-zero new_state needs the plane; before any upload there is no scene; an empty scene accepts insertions
    x = _mk(rec, W, H, ts, state=False)
    for fn in (lambda: insert.append(x, one, NEW), lambda: insert.append_ply(x, empty, 1), lambda: insert.duplicate(x, 0, 0, SEL),
               lambda: insert.duplicate(x, SEL, SEL, 0)):
        c, msg = code_of(fn)
        assert c == _abi.GS_ERR_INVALID_ARGUMENT and "GS_FLAG_SPLAT_STATE" in msg
        held(x, er.zero_padding(rec), None)
    x.destroy()
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(cfg), 64, 64, 8, _abi.GS_FLAG_SPLAT_STATE
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    cnt = ctypes.c_uint64()
    assert L.gs_append_splats(ctx, one.ctypes.data, 1, 0, ctypes.byref(first)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_append_splats_device(ctx, None, 0, 0, ctypes.byref(first)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_append_ply(ctx, empty.encode(), 0, ctypes.byref(first), ctypes.byref(cnt)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_duplicate_splats(ctx, 0, 0, 0, ctypes.byref(first), ctypes.byref(cnt), None) == _abi.GS_ERR_NO_SCENE
    _abi.check(L.gs_upload_splats(ctx, None, 0))
    _abi.check(L.gs_append_splats(ctx, one.ctypes.data, 1, NEW, ctypes.byref(first)))
    assert first.value == 0
    _abi.check(L.gs_duplicate_splats(ctx, 0, 0, 0x11, ctypes.byref(first), ctypes.byref(cnt), None))
    assert (first.value, cnt.value) == (1, 1)
    st = np.zeros(2, np.uint8)
    got = ctypes.c_uint64()
    _abi.check(L.gs_read_buffer(ctx, _abi.GS_BUF_SPLAT_STATE, st.ctypes.data, 2, ctypes.byref(got)))
    assert st.tolist() == [NEW, 0x11]
    _abi.check(L.gs_destroy(ctx))


@pytest.mark.gpu
def test_planes_and_scratch_after_insertion():
    """The coverage, neighbour-count and cluster planes read as their initial values after an insertion and the capacities are kept;
    a count, a labelling, a grade and a transform then run on the grown scene and match their own restatements."""
    from gpu_checks import orbit_uniforms
    from gsplat import _abi, clusters, colours, insert, neighbours
    rec = scene(10000)[:2001]
    k, W, H, ts, radius = 1501, 128, 128, 16, 0.2
    head, tail = np.ascontiguousarray(rec[:k]), np.ascontiguousarray(rec[k:])
    n = rec.shape[0]
    u = orbit_uniforms(W, H)
    r = _mk(head, W, H, ts)
    r.render_uniforms(u)
    r.wait()
    assert r.accumulate_coverage() == W * H
    neighbours.count(r, radius)
    clusters.label(r, radius)
    assert r.read_coverage()["hits"].any() and neighbours.read(r).any() and (clusters.read(r)[0] != clusters.NONE).all()
    st = r.stats()
    cap = st["capacity"], st["row_capacity"]
    assert insert.append(r, tail, SEL) == (k, n - k)
    cov = r.read_coverage()
    assert cov.shape == (n,) and not cov["hits"].any() and not cov["sum_q"].any() and not cov["max_weight"].any()
    cnt = neighbours.read(r)
    assert cnt.shape == (n,) and not cnt.any()
    labels, sizes = clusters.read(r)
    assert labels.shape == (n,) and (labels == clusters.NONE).all() and not sizes.any()
    r.render_uniforms(u)
    r.wait()
    st = r.stats()
    assert st["num_gaussians"] == n and st["capacity"] >= cap[0] and st["row_capacity"] >= cap[1]
    # the planes and the scratch are sized for the grown scene
    assert r.accumulate_coverage() == W * H and r.read_coverage()["hits"].any()
    info = neighbours.count(r, radius)
    assert info["queried"] == n
    want = nr.counts(rec, radius)
    np.testing.assert_array_equal(neighbours.read(r), want)
    assert want[k:].any()
    info = clusters.label(r, radius)
    assert info["members"] == n
    want_label, want_size = cr.components(rec, radius)
    got_label, got_size = clusters.read(r)
    np.testing.assert_array_equal(got_label, want_label)
    np.testing.assert_array_equal(got_size, want_size)
    assert (want_size[k:] > 1).any()
    sel = np.arange(n) >= k
    g = colours.compose(gain=(1.2, 1.2, 1.2))
    assert colours.brighten(r, 1.2) == n - k
    want_rec = gr.apply(er.zero_padding(rec), gr.Grade.from_struct(g), sel)
    np.testing.assert_array_equal(er.bits(r.export_splats()), er.bits(want_rec))
    t = (0.5, -0.25, 1.0)
    assert r.translate_selected(t) == n - k
    want_rec = xr.apply(want_rec, xr.Xform.from_struct(_abi.compose_xform(translate=t)), sel)
    np.testing.assert_array_equal(er.bits(r.export_splats()), er.bits(want_rec))
    assert (er.bits(want_rec)[k:, :3] != er.bits(rec)[k:, :3]).any()
    r.destroy()


# ---- verbs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_merge_ply_then_translate(tmp_path):
    """merge_ply clears the selection and brings the file in selected: translate_selected then moves exactly the new splats."""
    from gsplat import _abi, insert
    rec = scene(10000)[:1201]
    k = 801
    head, tail = np.ascontiguousarray(rec[:k]), np.ascontiguousarray(rec[k:])
    plane = old_plane(k) | np.where(np.arange(k) % 5 == 0, SEL, 0).astype(np.uint8)
    path = str(tmp_path / "second.ply")
    _abi.save_ply(path, tail, 3)
    r = _mk(head, 64, 64, 8)
    r.write_state(plane)
    assert insert.merge_ply(r, path) == (k, rec.shape[0] - k)
    state = np.concatenate([plane & np.uint8(0xFF ^ SEL), np.full(rec.shape[0] - k, SEL, np.uint8)])
    held(r, er.zero_padding(rec), state)
    t = (3.0, 0.125, -2.0)
    assert r.translate_selected(t) == rec.shape[0] - k
    want = xr.apply(er.zero_padding(rec), xr.Xform.from_struct(_abi.compose_xform(translate=t)), np.arange(rec.shape[0]) >= k)
    held(r, want, state)
    np.testing.assert_array_equal(er.bits(want)[:k], er.bits(er.zero_padding(head)))
    assert (er.bits(want)[k:, :3] != er.bits(tail)[:, :3]).all()
    r.destroy()


@pytest.mark.gpu
def test_duplicate_selected():
    """The originals stay bit-equal and end up deselected; the copies are selected and equal the transform's restatement of the
    originals.  Once on a Renderer with a transform, once on a PipelinedRenderer without."""
    import gsplat
    from gsplat import _abi, insert
    rec = scene(10000)[:1030]
    n = rec.shape[0]
    plane = old_plane(n) | np.where(np.arange(n) % 3 == 0, SEL, 0).astype(np.uint8)
    ids = er.ids_of(plane, SEL, SEL)
    assert 0 < ids.size < n
    cleared = plane & np.uint8(0xFF ^ SEL)
    x = _abi.compose_xform(rot=(0.9, 0.1, -0.3, 0.2), translate=(1.0, 2.0, -0.5), scale=1.5, pivot=(0.1, 0.2, 0.3))
    r = _mk(rec, 64, 64, 8)
    r.write_state(plane)
    assert insert.duplicate_selected(r, x) == (n, ids.size)
    copies = xr.apply(er.zero_padding(rec[ids]), xr.Xform.from_struct(x))
    state = np.concatenate([cleared, np.full(ids.size, SEL, np.uint8)])
    held(r, np.concatenate([er.zero_padding(rec), copies]), state)
    assert (er.bits(copies)[:, :12] != er.bits(rec[ids])[:, :12]).any()
    r.destroy()
    p = gsplat.PipelinedRenderer(gsplat.Canvas(64, 64), None, 0, gsplat.PackedGaussians(rec), 8, frames_in_flight=2,
                                 flags=_abi.GS_FLAG_EXACT_BLEND | _abi.GS_FLAG_F32_TAP | _abi.GS_FLAG_SPLAT_STATE)
    p.write_state(plane)
    assert insert.duplicate_selected(p) == (n, ids.size)
    np.testing.assert_array_equal(p.read_state(), state)
    np.testing.assert_array_equal(er.bits(p.export_splats()), er.bits(er.zero_padding(np.concatenate([rec, rec[ids]]))))
    assert [m.numGaussians for m in p.renderers] == [n + ids.size] * 2
    p.destroy()
