"""gs_pick: per-pixel splat queries (front, dominant, median) on the last frame (include/gsplat/gs_abi.h).

The reference the GPU answers are held to is tests/pick_restate.py, a numpy restatement of the blend's expression tree with
the books a query keeps.  The CPU tests prove that the restatement IS the oracle's blend (its alpha and accumulated depth
are bit-equal to aux_restate, which is bit-equal to the oracle's colour) and that the query sets reach every class of answer;
the GPU tests hold every field of every result, and every contributor record, to it bit for bit -- in EXACT and fused
frames, every binning, emission order and frame path --, and prove that a pick disturbs nothing.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import scene
from support import GOLDEN, NODE, c_layout, host_sources, lattice, mk, pick_case, run_node, timeless
MARGIN = ("transmittance_edge", "live_box", "degenerate_conic")
# (scene, tile size): config A at every tile size, the ragged golden, the three scenes of test_blend_culls.py, and a scene built
# so that two accepted entries of a pixel have the SAME weight (the earliest must win; random scenes hold no such pixel)
CASES = [("cfgA", 8), ("cfgA", 16), ("cfgA", 32), ("ragged", 8)] + [(name, 16) for name in MARGIN] + [("weight_ties", 16)]
CASE_IDS = ["%s-t%d" % c for c in CASES]
MAX_CONTRIBS = (0, 4, 256)

_CACHE = {}


def _restated(oracle, name, ts):
    """The restatement of the case's queries with the largest max_contrib (a smaller one is its leading columns)."""
    from pick_restate import restate_ref
    k = ("restate", name, ts)
    if k not in _CACHE:
        s, u, W, H, ref, xy = pick_case(oracle, name, ts)
        _CACHE[k] = restate_ref(ref, W, H, ts, xy, max(MAX_CONTRIBS))
    return _CACHE[k]


def _words(a):
    """A structured array of 4-byte fields as its u32 words (floats compared as bits: NaN and -0 count)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(a.shape + (a.dtype.itemsize // 4,))


# ---- CPU: the restatement is the oracle's blend, and the queries reach every class -----------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_restatement_is_the_oracle(oracle, case):
    """alpha and depth_acc of every query pixel are bit-equal to aux_restate (itself bit-equal to the C oracle's colour:
    test_aux_planes.py), which applies EVERY entry of the list as written."""
    from aux_restate import restate_ref as planes
    name, ts = case
    s, u, W, H, ref, xy = pick_case(oracle, name, ts)
    res, con, _ = _restated(oracle, name, ts)
    _, A, D = planes(ref, W, H, ts)
    ys, xs = xy[:, 1].astype(np.int64), xy[:, 0].astype(np.int64)
    np.testing.assert_array_equal(res["alpha"].view(np.uint32), np.ascontiguousarray(A[ys, xs]).view(np.uint32))
    np.testing.assert_array_equal(res["depth_acc"].view(np.uint32), np.ascontiguousarray(D[ys, xs]).view(np.uint32))
    assert (res["status"] == 0).all() and (res["reserved"] == 0).all()
    # the books are consistent with themselves
    hit = res["hit_count"] > 0
    assert ((res["first_id"] != 0xFFFFFFFF) == hit).all() and ((res["max_id"] != 0xFFFFFFFF) == hit).all()
    assert (res["max_weight"][hit] > 0).all() and (res["max_weight"][~hit] == 0).all()
    assert (res["hit_count"] <= res["list_length"]).all()
    filled = (con["id"] != 0xFFFFFFFF).sum(axis=1)
    np.testing.assert_array_equal(filled, np.minimum(res["hit_count"], max(MAX_CONTRIBS)))
    np.testing.assert_array_equal(con["id"][hit, 0], res["first_id"][hit])
    np.testing.assert_array_equal(con["weight"].max(axis=1), res["max_weight"])
    med = res["median_id"] != 0xFFFFFFFF
    assert (res["alpha"][med] >= 0.5).all() and (res["alpha"][hit & ~med] < 0.5).all()


def test_query_sets_reach_every_class(oracle):
    """Over the union of the query sets: no hit; hits but no median; a median; max != first; median != max; an accepted entry
    AFTER one rejected by test < 1e-4; more hits than the smallest max_contrib tested; a LATER accepted entry with exactly the
    largest weight (a tie the earliest entry must win)."""
    NONE = 0xFFFFFFFF
    seen = dict.fromkeys(("empty", "no_median", "median", "max_not_first", "median_not_max", "rejected_then_accepted", "over_contrib",
                         "weight_tie"), 0)
    for name, ts in CASES:
        res, con, cls = _restated(oracle, name, ts)
        h = res["hit_count"]
        seen["empty"] += int((h == 0).sum())
        seen["no_median"] += int(((h > 0) & (res["median_id"] == NONE)).sum())
        seen["median"] += int((res["median_id"] != NONE).sum())
        seen["max_not_first"] += int(((h > 0) & (res["max_id"] != res["first_id"])).sum())
        seen["median_not_max"] += int(((res["median_id"] != NONE) & (res["median_id"] != res["max_id"])).sum())
        seen["rejected_then_accepted"] += int(cls["rejected_then_accepted"].sum())
        seen["over_contrib"] += int((h > min(m for m in MAX_CONTRIBS if m)).sum())
        assert h.max() <= max(MAX_CONTRIBS)  # (so the contributor records hold every accepted entry)
        top = (con["weight"].view(np.uint32) == res["max_weight"].view(np.uint32)[:, None]) & (con["id"] != NONE)
        seen["weight_tie"] += int(((top.sum(axis=1) >= 2) & (con["id"][np.arange(h.size), np.argmax(top, axis=1)] == res["max_id"])).sum())
    print("\npick classes:", seen)
    assert all(v > 0 for v in seen.values()), seen


def test_pick_abi(tmp_path):
    """gs_pick is exported without a GPU; the record layouts and constants agree between the header, ctypes and the Node host;
    a null context is refused with a message."""
    from gsplat import _abi
    from pick_restate import RESULT_DTYPE, CONTRIB_DTYPE
    L = _abi.load()
    assert hasattr(L, "gs_pick") and "gs_pick" in _abi.ABI_SYMBOLS
    assert ctypes.sizeof(_abi.GsPickResult) == 48 and ctypes.sizeof(_abi.GsPickQuery) == 8 and ctypes.sizeof(_abi.GsPickContrib) == 8
    fields = [n for n, _ in _abi.GsPickResult._fields_]
    prog = 'printf("%zu %zu %zu", sizeof(gs_pick_result), sizeof(gs_pick_query), sizeof(gs_pick_contrib));'
    prog += "".join('printf(" %%zu", offsetof(gs_pick_result, %s));' % n for n in fields)
    prog += 'printf(" %zu %zu %zu %zu", offsetof(gs_pick_query, x), offsetof(gs_pick_query, y), offsetof(gs_pick_contrib, id), offsetof(gs_pick_contrib, weight));'
    prog += 'printf(" %u %u %u %u %u", GS_PICK_OK, GS_PICK_OUTSIDE_SLAB, GS_PICK_NONE, GS_PICK_MAX_QUERIES, GS_PICK_MAX_CONTRIB);'
    out = c_layout(tmp_path, "pick_layout", prog)
    assert out[:3] == [48, 8, 8]
    assert out[3:15] == [getattr(_abi.GsPickResult, n).offset for n in fields] == [4 * k for k in range(12)]
    assert out[15:19] == [_abi.GsPickQuery.x.offset, _abi.GsPickQuery.y.offset, _abi.GsPickContrib.id.offset, _abi.GsPickContrib.weight.offset]
    consts = out[19:]
    assert consts == [0, 1, 0xFFFFFFFF, 65536, 256]
    assert consts == [_abi.GS_PICK_OK, _abi.GS_PICK_OUTSIDE_SLAB, _abi.GS_PICK_NONE, _abi.GS_PICK_MAX_QUERIES, _abi.GS_PICK_MAX_CONTRIB]
    # the numpy views of the records: the same names, offsets and kinds (and the restatement's own)
    for dt in (_abi.PICK_RESULT_DTYPE, RESULT_DTYPE):
        assert dt.itemsize == 48 and list(dt.names) == fields
        for n, t in _abi.GsPickResult._fields_:
            assert dt.fields[n][1] == getattr(_abi.GsPickResult, n).offset
            assert dt.fields[n][0] == (np.float32 if t is ctypes.c_float else np.uint32)
    assert _abi.PICK_CONTRIB_DTYPE == CONTRIB_DTYPE and CONTRIB_DTYPE.itemsize == 8
    rjs, idx, dts, napi, hdr = host_sources()
    assert re.search(r"#define GS_ABI_VERSION 3\b", hdr) and "compute_tiles.wgsl:44-66" in hdr
    assert re.search(r"PICK = \{ OK: 0, OUTSIDE_SLAB: 1, NONE: 0xFFFFFFFF, MAX_QUERIES: 65536, MAX_CONTRIB: 256 \}", rjs)
    assert re.search(r"\bPICK\b", idx) and "OK: 0, OUTSIDE_SLAB: 1, NONE: 0xFFFFFFFF, MAX_QUERIES: 65536, MAX_CONTRIB: 256" in idx
    assert "pick(queries: Uint32Array, maxContrib?: number): PickResult" in dts
    assert "OK: 0; OUTSIDE_SLAB: 1; NONE: 0xFFFFFFFF; MAX_QUERIES: 65536; MAX_CONTRIB: 256" in dts
    m = re.search(r"PICK_FIELD = \{([^}]*)\}", rjs)
    words = [int(v) for v in re.findall(r":\s*(\d+)", m.group(1))]
    assert words == list(range(12))  # the JS field table walks the record word by word, in the header's order
    for name in ("PICK_OK", "PICK_OUTSIDE_SLAB", "PICK_NONE", "PICK_MAX_QUERIES", "PICK_MAX_CONTRIB"):
        assert '"%s", GS_%s' % (name, name) in napi
    # no context: refused, with a message, before anything else is looked at
    q = (_abi.GsPickQuery * 1)()
    r = (_abi.GsPickResult * 1)()
    assert L.gs_pick(None, q, 1, r, 0, None) == -1
    assert b"gs_pick" in L.gs_last_error()


def test_merge_picks():
    from gsplat import _abi
    from gsplat.multigpu import merge_picks
    dt = _abi.PICK_RESULT_DTYPE
    n, world = 9, 3
    owner = np.array([0, 2, 1, 1, 0, 2, 2, 0, 1])
    full = np.zeros(n, dt)
    full["hit_count"] = np.arange(n) + 1
    full["first_id"] = 100 + np.arange(n)
    full["alpha"] = np.linspace(0.1, 0.9, n, dtype=np.float32)
    ranks = []
    for g in range(world):
        r = np.zeros(n, dt)
        r["first_id"] = r["max_id"] = r["median_id"] = _abi.GS_PICK_NONE
        r["status"] = _abi.GS_PICK_OUTSIDE_SLAB
        r[owner == g] = full[owner == g]
        ranks.append(r)
    merged = merge_picks(ranks)
    assert merged.dtype == dt
    np.testing.assert_array_equal(_words(merged), _words(full))
    np.testing.assert_array_equal(_words(merge_picks(np.stack(ranks))), _words(full))
    both = [r.copy() for r in ranks]
    both[1][0] = full[0]  # two ranks claim query 0
    with pytest.raises(ValueError, match="query 0 .* 2 ranks"):
        merge_picks(both)
    none = [r.copy() for r in ranks]
    none[2]["status"][1] = _abi.GS_PICK_OUTSIDE_SLAB  # nobody answers query 1
    with pytest.raises(ValueError, match="query 1 .* 0 ranks"):
        merge_picks(none)
    with pytest.raises(ValueError):
        merge_picks([ranks[0], ranks[1][:4]])
    with pytest.raises(ValueError):
        merge_picks([])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _check(got, want, tight, cell, ref_len=None):
    """Every field bit-equal; list_length equal for the reference's binning, at most the reference's for tight lists."""
    res, con = got if isinstance(got, tuple) else (got, None)
    wres, wcon = want
    g, w = _words(res), _words(wres)
    cols = [k for k in range(12) if k != 1]
    np.testing.assert_array_equal(g[:, cols], w[:, cols], err_msg="results " + str(cell))
    ref_len = wres["list_length"] if ref_len is None else ref_len
    if tight:
        assert (res["list_length"] <= ref_len).all(), cell
        assert (res["list_length"] >= res["hit_count"]).all(), cell
    else:
        np.testing.assert_array_equal(res["list_length"], ref_len, err_msg="list_length " + str(cell))
    if con is not None:
        mc = con.shape[1]
        np.testing.assert_array_equal(_words(con), _words(wcon[:, :mc]), err_msg="contributors " + str(cell))


# (GS_OPT_TILE_CULL, gs_render_debug, GS_OPT_EMIT_ORDER, GS_OPT_FRAME_GRAPH): every value of every knob, the product path first
FRAME_PATHS = [(1, False, 2, 0), (0, False, 1, 0), (0, False, 0, 0), (0, True, 1, 0), (1, False, 0, 1), (0, False, 1, 1), (1, False, 1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fused"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_pick_bit_equal(oracle, case, exact):
    """Every field of every result and every contributor record equals the restatement bit for bit, whatever blend, binning,
    emission order and frame path rendered the frame."""
    from gsplat import _abi
    name, ts = case
    s, u, W, H, ref, xy = pick_case(oracle, name, ts)
    wres, wcon, _ = _restated(oracle, name, ts)
    r = mk(s, W, H, ts, exact=exact)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    for tight, debug, order, graph in FRAME_PATHS:
        r.set_option(_abi.GS_OPT_TILE_CULL, tight)
        r.set_option(_abi.GS_OPT_EMIT_ORDER, order)
        r.set_option(_abi.GS_OPT_FRAME_GRAPH, graph)
        for rep in range(2 if graph else 1):  # with the graph: the frame that captures it, then a replay
            r.render_uniforms(u, debug=debug)
            r.wait()
            st = r.stats()
            is_tight = bool(st["tight_binning"])
            assert is_tight == bool(tight and not debug)
            for mc in MAX_CONTRIBS:
                _check(r.pick(xy, mc), (wres, wcon), is_tight, (name, ts, exact, tight, debug, order, graph, rep, mc))
        if graph:
            assert r.stats()["graph_frames"] >= 1
    r.destroy()


@pytest.mark.gpu
def test_pick_agrees_with_the_planes_and_pick_rect(oracle):
    """AUX | EXACT: alpha and depth_acc of a whole-canvas pick equal read_alpha() / read_depth() bit for bit; every field of the
    65536 answers equals the restatement; pick_rect over the canvas is np.unique of the restatement's field."""
    from pick_restate import restate_ref
    s, u, W, H, ref, _ = pick_case(oracle, "cfgA", 16)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    xy = np.stack([xx.ravel(), yy.ravel()], axis=1)
    assert xy.shape[0] == 65536
    r = mk(s, W, H, 16, exact=True, aux=True)
    r.render_uniforms(u)
    r.wait()
    res = r.pick(xy)
    np.testing.assert_array_equal(res["alpha"].view(np.uint32).reshape(H, W), r.read_alpha().view(np.uint32))
    np.testing.assert_array_equal(res["depth_acc"].view(np.uint32).reshape(H, W), r.read_depth().view(np.uint32))
    wres, wcon, _ = restate_ref(ref, W, H, 16, xy, 0)
    _check(res, (wres, wcon), True, "whole canvas")
    for which in ("first", "max", "median"):
        f = wres[which + "_id"]
        want = np.unique(f[f != 0xFFFFFFFF])
        got = r.pick_rect(0, 0, W, H, which)
        assert got.dtype == np.uint32 and want.size > 10
        np.testing.assert_array_equal(got, want, err_msg=which)
    # a rectangle: the same, from its own pixels; one wider than a call's 65536 queries is chunked (the ragged split is exercised
    # by a 200-pixel-wide rectangle: 327 rows per call)
    x0, y0, x1, y1 = 37, 50, 237, 201
    inside = (xy[:, 0] >= x0) & (xy[:, 0] < x1) & (xy[:, 1] >= y0) & (xy[:, 1] < y1)
    f = wres["max_id"][inside]
    np.testing.assert_array_equal(r.pick_rect(x0, y0, x1, y1, "max"), np.unique(f[f != 0xFFFFFFFF]))
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_pick_disturbs_nothing(oracle, graph):
    from gsplat import _abi, synth
    s, _, W, H, _, xy = pick_case(oracle, "cfgA", 16)
    u0, u1 = (synth.orbit_camera(k, W, H).uniforms(W, H) for k in (2, 6))
    a = mk(s, W, H, 16, exact=False)  # picks between its frames
    b = mk(s, W, H, 16, exact=False)  # never picks
    for r in (a, b):
        r.set_option(_abi.GS_OPT_FRAME_GRAPH, graph)
        r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
        r.render_uniforms(u0)
        r.wait()
    before = (a.read_rgba8(), a.read_buffer(_abi.GS_BUF_VALUES), a.read_buffer(_abi.GS_BUF_RANGES), timeless(a.stats()))
    first = a.pick(xy, 4)
    again = a.pick(xy, 4)  # a second pick: the same answer
    np.testing.assert_array_equal(_words(first[0]), _words(again[0]))
    np.testing.assert_array_equal(_words(first[1]), _words(again[1]))
    after = (a.read_rgba8(), a.read_buffer(_abi.GS_BUF_VALUES), a.read_buffer(_abi.GS_BUF_RANGES), timeless(a.stats()))
    for x, y in zip(before[:3], after[:3]):
        np.testing.assert_array_equal(x, y)
    assert before[3] == after[3]
    for k in range(3):  # frames after a pick equal frames without one; the captured graph keeps being replayed
        for r in (a, b):
            r.render_uniforms(u1 if k % 2 == 0 else u0)
            r.wait()
        a.pick(xy[:7])
        np.testing.assert_array_equal(a.read_rgba8(), b.read_rgba8())
        np.testing.assert_array_equal(a.read_buffer(_abi.GS_BUF_RGB_F32), b.read_buffer(_abi.GS_BUF_RGB_F32))
        np.testing.assert_array_equal(a.read_buffer(_abi.GS_BUF_VALUES), b.read_buffer(_abi.GS_BUF_VALUES))
        assert timeless(a.stats()) == timeless(b.stats())
        assert a.stats()["graph_frames"] == (k + 2 if graph else 0)  # keeps counting up across the picks, as without them
    a.destroy()
    b.destroy()


@pytest.mark.gpu
def test_pick_ring_and_slabs(oracle):
    from pick_restate import restate
    from gsplat import _abi, synth
    from gsplat.multigpu import merge_picks
    import gsplat
    W, H, ts = 256, 256, 16
    s = scene(10000)
    xy = lattice(W, H, 5, 13, 3, 17)
    us = [synth.orbit_camera(k, W, H).uniforms(W, H) for k in (1, 4, 7)]
    refs = [oracle.render(s, u, W, H, ts) for u in us]
    want = [restate(f["gdata"], f["sorted_values"], f["ranges"], W, H, ts, xy, 4)[:2] for f in refs]
    assert not np.array_equal(_words(want[0][0]), _words(want[2][0]))  # the cameras see different splats
    # three frames enqueued, no gs_wait: the pick waits for and answers the LAST one
    r = mk(s, W, H, ts, exact=False)
    for u in us:
        r.render_uniforms(u)
    got = r.pick(xy, 4)
    _check(got, want[2], True, "three frames in flight")
    assert r.stats()["frames_in_flight"] == 3 and r.stats()["frames"] == 3
    r.destroy()
    # PipelinedRenderer: a pick addresses a slot's frame
    p = gsplat.PipelinedRenderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(s), ts, frames_in_flight=2)
    slots = [p.render_uniforms(u) for u in us[:2]]
    for k, slot in enumerate(slots):
        _check(p.pick(slot, xy, 4), want[k], True, "pipelined slot %d" % slot)
    p.destroy()
    # two slab contexts over one scene: each refuses the other's pixels; merged, they are the whole-canvas context's answer
    whole = mk(s, W, H, ts, exact=False)
    whole.render_uniforms(us[1])
    full = whole.pick(xy)
    whole.destroy()
    _check(full, want[1], True, "whole canvas")
    ntx = W // ts
    parts = []
    for cols in ((0, 5), (5, ntx)):
        sl = mk(s, W, H, ts, exact=False, cols=cols)
        sl.render_uniforms(us[1])
        res = sl.pick(xy)
        sl.destroy()
        x0, x1 = cols[0] * ts, min(W, cols[1] * ts)
        mine = (xy[:, 0] >= x0) & (xy[:, 0] < x1)
        assert mine.any() and (~mine).any()
        assert (res["status"][mine] == _abi.GS_PICK_OK).all() and (res["status"][~mine] == _abi.GS_PICK_OUTSIDE_SLAB).all()
        blank = np.zeros(1, _abi.PICK_RESULT_DTYPE)
        blank["status"] = _abi.GS_PICK_OUTSIDE_SLAB
        blank["first_id"] = blank["max_id"] = blank["median_id"] = _abi.GS_PICK_NONE
        np.testing.assert_array_equal(_words(res[~mine]), np.repeat(_words(blank), int((~mine).sum()), axis=0))
        # the restatement of the slab's own oracle frame (its lists hold the slab's instances only)
        sref = oracle.render(s, us[1], W, H, ts, cols=cols)
        swant = restate(sref["gdata"], sref["sorted_values"], sref["ranges"], W, H, ts, xy, 0, cols=cols)
        _check(res, swant[:2], True, "slab %s" % (cols,))
        parts.append(res)
    merged = merge_picks(parts)
    g, w = _words(merged), _words(full)
    keep = [k for k in range(12) if k != 1]  # (list_length: a slab's tight lists are its own)
    np.testing.assert_array_equal(g[:, keep], w[:, keep])


@pytest.mark.gpu
def test_pick_errors(oracle):
    from gsplat import _abi
    s, u, W, H, ref, xy = pick_case(oracle, "ragged", 8)
    wres, wcon, _ = _restated(oracle, "ragged", 8)
    r = mk(s, W, H, 8, exact=True)
    L = _abi.load()

    def code(fn):
        with pytest.raises(_abi.GsError) as e:
            fn()
        return e.value.code, str(e.value)

    assert code(lambda: r.pick(xy))[0] == _abi.GS_ERR_NO_FRAME  # before any frame
    r.render_uniforms(u)
    r.wait()
    c, msg = code(lambda: r.pick(np.array([[3, 4], [5, H]])))
    assert c == _abi.GS_ERR_INVALID_ARGUMENT and "query 1" in msg
    c, msg = code(lambda: r.pick(np.array([[3, 4], [5, 6], [W, 0]])))
    assert c == _abi.GS_ERR_INVALID_ARGUMENT and "query 2" in msg
    assert code(lambda: r.pick(np.zeros((0, 2), np.uint32)))[0] == _abi.GS_ERR_INVALID_ARGUMENT
    assert code(lambda: r.pick(np.zeros((65537, 2), np.uint32)))[0] == _abi.GS_ERR_INVALID_ARGUMENT
    assert code(lambda: r.pick(xy, 257))[0] == _abi.GS_ERR_INVALID_ARGUMENT
    q = np.ascontiguousarray(xy[:2], np.uint32)
    res = np.zeros(2, _abi.PICK_RESULT_DTYPE)
    con = np.zeros((2, 4), _abi.PICK_CONTRIB_DTYPE)
    assert L.gs_pick(r._ctx, q.ctypes.data, 2, res.ctypes.data, 0, con.ctypes.data) == -1  # contrib without max_contrib
    assert b"max_contrib" in L.gs_last_error()
    assert L.gs_pick(r._ctx, q.ctypes.data, 2, res.ctypes.data, 4, None) == -1            # max_contrib without contrib
    assert L.gs_pick(r._ctx, None, 2, res.ctypes.data, 0, None) == -1
    assert L.gs_pick(r._ctx, q.ctypes.data, 2, None, 0, None) == -1
    with pytest.raises(ValueError):
        r.pick(np.array([[-1, 0]]))
    with pytest.raises(ValueError):
        r.pick(np.array([1, 2, 3]))
    # the context is unharmed: the frame is still there, picks and frames work
    np.testing.assert_array_equal(r.read_rgba8(), np.load(os.path.join(GOLDEN, "ragged_3001_200x120_t8.npz"))["rgba8"])
    _check(r.pick(xy, 4), (wres, wcon), True, "after the errors")
    r.render_uniforms(u, debug=True)
    r.wait()
    np.testing.assert_array_equal(r.read_rgba8(), np.load(os.path.join(GOLDEN, "ragged_3001_200x120_t8.npz"))["rgba8"])
    _check(r.pick(xy, 4), (wres, wcon), False, "a frame after the errors")
    # a new upload takes the frame away again
    r2 = mk(s, W, H, 8, exact=True)
    r2.render_uniforms(u)
    r2.wait()
    arr = np.ascontiguousarray(s, dtype=np.float32)
    _abi.check(L.gs_upload_splats(r2._ctx, arr.ctypes.data, arr.shape[0]))
    assert code(lambda: r2.pick(xy))[0] == _abi.GS_ERR_NO_FRAME
    r2.destroy()
    r.destroy()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_node_host_pick_matches_python(tmp_path):
    from gsplat import synth
    n, W, H, ts, mc = 8000, 200, 120, 16, 4
    s = scene(n)
    u = synth.orbit_camera(4, W, H).uniforms(W, H)
    xy = lattice(W, H, 3, 11, 2, 7)
    rec, ub, qb, out = (str(tmp_path / f) for f in ("rec.bin", "u.bin", "q.bin", "pick.bin"))
    s.tofile(rec)
    u.tofile(ub)
    np.ascontiguousarray(xy, np.uint32).tofile(qb)
    info = run_node("pick_check.js", (rec, n, W, H, ts, ub, qb, mc, out))
    r = mk(s, W, H, ts, exact=False)
    r.render_uniforms(u)
    r.wait()
    pres, pcon = r.pick(xy, mc)
    r.destroy()
    raw = np.fromfile(out, dtype=np.uint32)
    nq = xy.shape[0]
    assert info["n"] == nq and raw.size == nq * 12 + nq * mc * 2
    np.testing.assert_array_equal(raw[: nq * 12].reshape(nq, 12), _words(pres))
    np.testing.assert_array_equal(raw[nq * 12:].reshape(nq, mc, 2), _words(pcon))
    # the accessor decodes the same record
    k = int(np.argmax(pres["hit_count"]))
    assert info["most_hits"]["q"] == k and info["most_hits"]["hitCount"] == int(pres["hit_count"][k]) > 0
    assert info["most_hits"]["firstId"] == int(pres["first_id"][k]) and info["most_hits"]["maxId"] == int(pres["max_id"][k])
    assert np.float32(info["most_hits"]["alpha"]) == pres["alpha"][k]
    assert [c["id"] for c in info["most_hits"]["contrib"]] == [int(v) for v in pcon["id"][k] if v != 0xFFFFFFFF]
    assert info["errors"] == {"outside": "-1", "odd": "TypeError"}


@pytest.mark.gpu
def test_pick_config_b_full_size(oracle):
    """Config B (6.1 M splats, 1080p; the scene, camera and oracle frame of test_gpu_scale.py::test_config_B_full_frame), the
    product path -- fused, tight, three frames in flight: 4096 seeded random pixels, every field bit-equal to the restatement."""
    import torch
    import gsplat
    from gsplat import synth
    from gpu_checks import make_renderer, orbit_uniforms
    from pick_restate import restate_ref
    n, W, H, ts = 6_100_000, 1920, 1080, 16
    dev = synth.bicycle_like_torch(n, synth.BASE_SEED + 1, "cuda")
    torch.cuda.synchronize()
    host = dev.cpu().numpy()
    u = orbit_uniforms(W, H, step=0)
    ref = oracle.render(host, u, W, H, ts)
    rng = np.random.default_rng(20240607)
    xy = np.stack([rng.integers(0, W, 4096), rng.integers(0, H, 4096)], axis=1).astype(np.uint32)
    wres, wcon, cls = restate_ref(ref, W, H, ts, xy, 256)
    pg = gsplat.PackedGaussians.__new__(gsplat.PackedGaussians)
    pg.numGaussians, pg.gaussiansBuffer, pg.sphericalHarmonicsDegree = n, dev, 3
    r = make_renderer(pg, W, H, ts)
    r.render_uniforms(u)
    r.wait()  # the first frame grows the capacity
    others = [orbit_uniforms(W, H, step=k) for k in (5, 9)]
    for uu in others + [u]:  # three frames in flight, the last one at the oracle's camera
        r.render_uniforms(uu)
    got = r.pick(xy, 256)
    st = r.stats()
    assert st["tight_binning"] == 1 and st["frames_in_flight"] == 3
    print("\ncfg-B pick: hits up to %d, lists up to %d (reference %d), %d with a median, %d rejected-then-accepted"
          % (int(wres["hit_count"].max()), int(got[0]["list_length"].max()), int(wres["list_length"].max()),
             int((wres["median_id"] != 0xFFFFFFFF).sum()), int(cls["rejected_then_accepted"].sum())))
    _check(got, (wres, wcon), True, "config B")
    _check(r.pick(xy[:100]), (wres[:100], wcon[:100]), True, "config B, no contributors")
    r.destroy()
    del dev
