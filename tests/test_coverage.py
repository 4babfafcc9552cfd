"""Coverage: per-splat contribution of the last frame, select by what is seen (include/gsplat/gs_abi.h "coverage").

The reference the GPU planes are held to is tests/coverage_restate.py: pick_restate (the oracle's blend, test_pick.py) over
every pixel of the region, folded per splat with integer and f32 numpy arithmetic.  The CPU tests pin the ABI, prove that the
fold is the pick's and that the cases reach every class of pair; the GPU tests hold all three planes to the restatement bit for
bit -- EXACT and fused frames, every binning, emission order and frame path --, and cover accumulation, gs_state_coverage, the
editor verbs, the ring, slabs, the lifecycle and the Node host.
"""
import ctypes
import re

import numpy as np
import pytest

from conftest import scene
from support import NODE, c_layout, code_of, host_sources, mk as _mk, pick_case, run_node, timeless
MARGIN = ("transmittance_edge", "live_box", "degenerate_conic")
RECT_A = (37, 51, 98, 96)    # [37,98) x [51,96): aligned to neither 8 nor a tile, crosses tile borders at every tile size
RECT_M = (3, 2, 60, 45)      # the margin scenes' first rect; their second is the canvas's bottom-right corner ("corner")
# (scene, tile size, rect or None for the whole canvas or "corner", mask or None)
CASES = ([("cfgA", ts, RECT_A, None) for ts in (8, 16, 32)] + [(name, 16, RECT_M, None) for name in MARGIN] +
         [(name, 16, "corner", None) for name in MARGIN] + [("weight_ties", 16, None, None), ("cfgA", 16, RECT_A, "checker3")])
CASE_IDS = ["%s-t%d-%s%s" % (c[0], c[1], "whole" if c[2] is None else c[2] if isinstance(c[2], str) else "rect", "-mask" if c[3] else "") for c in CASES]

_CACHE = {}


def _scene_of(oracle, name, ts):
    """(splats, uniforms, W, H, oracle frame) of a case: the scenes and frames of test_pick.py."""
    s, u, W, H, ref, _ = pick_case(oracle, name, ts)
    return s, u, W, H, ref


def _rect_of(rect, W, H):
    return (W - 21, H - 19, W, H) if rect == "corner" else rect


def _mask_of(kind, W, H):
    """checker3: a checkerboard of 3 x 3 pixel squares."""
    if kind is None:
        return None
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (((xx // 3 + yy // 3) % 2) == 0).astype(np.uint8)


def _records(oracle, name, ts, rect):
    """The per-pixel restatement of every pixel of the rect (shared by the masked and the unmasked case)."""
    import coverage_restate as cr
    k = ("records", name, ts, rect)
    if k not in _CACHE:
        s, u, W, H, ref = _scene_of(oracle, name, ts)
        xy = cr.region_pixels(W, H, _rect_of(rect, W, H))
        _CACHE[k] = (xy, cr.pixel_records(ref, W, H, ts, xy))
    return _CACHE[k]


def _restated(oracle, case):
    """(planes, classes, per-pixel results of P) of a case."""
    import coverage_restate as cr
    if case not in _CACHE:
        name, ts, rect, mk = case
        s, u, W, H, ref = _scene_of(oracle, name, ts)
        xy, rec = _records(oracle, name, ts, rect)
        mask = _mask_of(mk, W, H)
        keep = None if mask is None else mask[xy[:, 1], xy[:, 0]] != 0
        planes, classes = cr.fold(s.shape[0], xy, rec, W, ts, ref, keep)
        _CACHE[case] = (planes, classes, rec[0] if keep is None else rec[0][keep])
    return _CACHE[case]


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_coverage_abi(tmp_path):
    """The four symbols are exported without a GPU; the record and region layouts agree between the compiled header, ctypes,
    COVERAGE_DTYPE and the Node tables; GS_ABI_VERSION is still 3; a null context is refused with a message."""
    from gsplat import _abi
    import coverage_restate as cr
    L = _abi.load()
    names = ("gs_coverage_accumulate", "gs_coverage_reset", "gs_coverage_read", "gs_state_coverage")
    for name in names:
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    rec_fields = [n for n, _ in _abi.GsCoverageRec._fields_]
    reg_fields = [n for n, _ in _abi.GsCoverRegion._fields_]
    assert rec_fields == ["sum_q", "hits", "max_weight"] and reg_fields == ["struct_size", "x0", "y0", "x1", "y1", "mask"]
    prog = 'printf("%d %zu %zu", GS_ABI_VERSION, sizeof(gs_coverage_rec), sizeof(gs_cover_region));'
    prog += "".join('printf(" %%zu", offsetof(gs_coverage_rec, %s));' % n for n in rec_fields)
    prog += "".join('printf(" %%zu", offsetof(gs_cover_region, %s));' % n for n in reg_fields)
    out = c_layout(tmp_path, "coverage_layout", prog)
    assert out[0] == 3 and L.gs_abi_version() == 3
    assert out[1] == 16 == ctypes.sizeof(_abi.GsCoverageRec) == _abi.COVERAGE_DTYPE.itemsize == cr.COVERAGE_DTYPE.itemsize
    assert out[2] == ctypes.sizeof(_abi.GsCoverRegion) == 32
    assert out[3:6] == [getattr(_abi.GsCoverageRec, n).offset for n in rec_fields] == [0, 8, 12]
    assert out[6:12] == [getattr(_abi.GsCoverRegion, n).offset for n in reg_fields] == [0, 4, 8, 12, 16, 24]
    for dt in (_abi.COVERAGE_DTYPE, cr.COVERAGE_DTYPE):
        assert list(dt.names) == rec_fields and [dt.fields[n][1] for n in rec_fields] == [0, 8, 12]
        assert [dt.fields[n][0] for n in rec_fields] == [np.uint64, np.uint32, np.float32]
    rjs, idx, dts, napi, hdr = host_sources()
    assert re.search(r"#define GS_ABI_VERSION 3\b", hdr)
    for name in names:
        assert re.search(r"int32_t %s\(gs_ctx\*" % name, hdr)
    assert "2^64" in hdr and "2^32 accepted pairs" in hdr  # the wrap-around is documented
    assert re.search(r"COVERAGE = \{ REC_BYTES: 16 \}", rjs)
    m = re.search(r"COVERAGE_FIELD = \{([^}]*)\}", rjs)
    assert [(k, int(v)) for k, v in re.findall(r"(\w+):\s*(\d+)", m.group(1))] == [("sumQ", 0), ("hits", 8), ("maxWeight", 12)]
    assert re.search(r"\bCOVERAGE\b", idx) and "sumQ: 0, hits: 8, maxWeight: 12" in idx
    assert "COVERAGE_FIELD: { sumQ: 0; hits: 8; maxWeight: 12 }" in dts and "REC_BYTES: 16" in dts
    for fn in ("accumulateCoverage", "resetCoverage", "readCoverage", "stateCoverage"):
        assert re.search(r"\b%s\(" % fn, dts) and re.search(r"\b%s\(" % fn, rjs)
    for fn in ("accumulateCoverage", "resetCoverage", "readCoverage", "stateCoverage"):
        assert '{"%s", js_' % fn in napi
    assert '"COVERAGE_REC_BYTES", (double)sizeof(gs_coverage_rec)' in napi
    # no context: refused, with a message, before anything else is looked at
    n = ctypes.c_uint64()
    for rc, who in ((L.gs_coverage_accumulate(None, None, None), b"gs_coverage_accumulate"), (L.gs_coverage_reset(None), b"gs_coverage_reset"),
                    (L.gs_coverage_read(None, None, 0, ctypes.byref(n)), b"gs_coverage_read"),
                    (L.gs_state_coverage(None, 1, 0.0, 1, 0, 0, 1, 2, None), b"gs_state_coverage")):
        assert rc == -1
    assert b"gs_state_coverage" in L.gs_last_error()
    assert L.gs_coverage_reset(None) == -1 and b"gs_coverage_reset" in L.gs_last_error()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_restatement_is_the_picks(oracle, case):
    """hits summed over splats is hit_count summed over pixels; the largest max_weight is the largest of the pixels'."""
    planes, classes, res = _restated(oracle, case)
    assert classes["pixels"] == res.size > 0
    assert int(planes["hits"].astype(np.uint64).sum()) == int(res["hit_count"].astype(np.uint64).sum()) > 0
    assert planes["max_weight"].max().view(np.uint32) == res["max_weight"].max().view(np.uint32)
    assert classes["max_hits_per_pixel"] <= 256
    seen = planes["hits"] > 0
    assert (planes["max_weight"][seen] > 0).all() and (planes["max_weight"][~seen] == 0).all() and (planes["sum_q"][~seen] == 0).all()
    # floor(w 2^32) summed: at most hits * max_weight * 2^32, at least one pair's worth
    assert (planes["sum_q"][seen].astype(np.float64) <= planes["hits"][seen] * planes["max_weight"][seen].astype(np.float64) * 2.0 ** 32).all()
    assert (planes["sum_q"][seen] > 0).all()
    if case[:3] == ("cfgA", 16, RECT_A) and case[3] is None:
        assert classes["pixels"] == 2745


def test_cases_reach_every_class(oracle):
    """Asserted, not assumed: a list longer than one chunk of 64; a splat hit from two or more tiles; from two or more blocks of one
    tile at tile sizes 16 and 32; a listed but never accepted splat; a pixel that accepts an entry behind a rejected one; a pixel
    without a hit; a splat with more pairs than P has pixels (it sits twice in a list)."""
    keys = ("multi_tile", "listed_never_accepted", "rejected_then_accepted", "zero_hit_pixels", "more_hits_than_pixels")
    seen = dict.fromkeys(keys + ("long_list", "blocks_t16", "blocks_t32", "overhang"), 0)
    for case in CASES:
        planes, classes, res = _restated(oracle, case)
        for k in keys:
            seen[k] += classes[k]
        seen["long_list"] += int(classes["max_list"] > 64)
        if case[1] in (16, 32):
            seen["blocks_t%d" % case[1]] += classes["multi_block_one_tile"]
        if case[2] == "corner":
            s, u, W, H, ref = _scene_of(oracle, case[0], case[1])
            seen["overhang"] += int(W % 8 != 0 and H % 8 != 0)  # the corner's blocks overhang the canvas
        print("\n%s: %s" % ("-".join(str(c) for c in case[:2]), classes))
    assert all(v > 0 for v in seen.values()), seen


def test_merge_coverage():
    from gsplat import _abi
    from gsplat.multigpu import merge_coverage
    rng = np.random.default_rng(11)
    n, world = 1000, 3
    parts = []
    for g in range(world):
        p = np.zeros(n, _abi.COVERAGE_DTYPE)
        hit = rng.random(n) < 0.4
        p["hits"][hit] = rng.integers(1, 5000, int(hit.sum()))
        p["max_weight"][hit] = rng.random(int(hit.sum())).astype(np.float32) * np.float32(0.99)
        p["sum_q"][hit] = rng.integers(1, 2 ** 45, int(hit.sum()), dtype=np.uint64)
        parts.append(p)
    parts[0]["sum_q"][0], parts[1]["sum_q"][0] = np.uint64(2 ** 64 - 5), np.uint64(9)  # wraps modulo 2^64, as the device's adds do
    parts[0]["hits"][0], parts[1]["hits"][0] = np.uint32(2 ** 32 - 1), np.uint32(3)
    want = np.zeros(n, _abi.COVERAGE_DTYPE)
    for i in range(n):  # a single-array fold, record by record
        sq, h, mw = 0, 0, np.float32(0)
        for p in parts:
            sq, h, mw = (sq + int(p["sum_q"][i])) % 2 ** 64, (h + int(p["hits"][i])) % 2 ** 32, max(mw, p["max_weight"][i])
        want[i] = (sq, h, mw)
    got = merge_coverage(parts)
    assert got.dtype == _abi.COVERAGE_DTYPE
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(merge_coverage(np.stack(parts)).view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(merge_coverage([parts[1]]).view(np.uint32), parts[1].view(np.uint32))
    with pytest.raises(ValueError):
        merge_coverage([])
    with pytest.raises(ValueError):
        merge_coverage([parts[0], parts[1][:10]])
    with pytest.raises(ValueError):
        merge_coverage([parts[0], np.zeros(n, np.uint32)])


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def _same(got, want, cell=""):
    import coverage_restate as cr
    np.testing.assert_array_equal(cr.words(got), cr.words(want), err_msg=str(cell))


# (GS_OPT_TILE_CULL, gs_render_debug, GS_OPT_EMIT_ORDER, GS_OPT_FRAME_GRAPH): every value of every knob, the product path first
FRAME_PATHS = [(1, False, 2, 0), (0, False, 1, 0), (0, False, 0, 0), (0, True, 1, 0), (1, False, 0, 1), (0, False, 1, 1), (1, False, 1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fused"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_coverage_bit_equal(oracle, case, exact):
    """All three planes of every resident splat equal the restatement bit for bit -- splats outside the touched tiles are exactly
    zero --, whatever blend, binning, emission order and frame path rendered the frame."""
    from gsplat import _abi
    name, ts, rect, mk = case
    s, u, W, H, ref = _scene_of(oracle, name, ts)
    want, classes, _ = _restated(oracle, case)
    rect, mask = _rect_of(rect, W, H), _mask_of(mk, W, H)
    r = _mk(s, W, H, ts, exact=exact)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    for tight, debug, order, graph in FRAME_PATHS:
        r.set_option(_abi.GS_OPT_TILE_CULL, tight)
        r.set_option(_abi.GS_OPT_EMIT_ORDER, order)
        r.set_option(_abi.GS_OPT_FRAME_GRAPH, graph)
        for rep in range(2 if graph else 1):  # with the graph: the frame that captures it, then a replay
            r.render_uniforms(u, debug=debug)
            r.wait()
            assert bool(r.stats()["tight_binning"]) == bool(tight and not debug)
            r.reset_coverage()
            assert r.accumulate_coverage(rect, mask) == classes["pixels"]
            got = r.read_coverage()
            assert got.dtype == _abi.COVERAGE_DTYPE and got.shape == (s.shape[0],)
            _same(got, want, (case, exact, tight, debug, order, graph, rep))
        if graph:
            assert r.stats()["graph_frames"] >= 1
    r.destroy()


@pytest.mark.gpu
def test_coverage_accumulates(oracle):
    """Read before any accumulate is zeros; the same call twice doubles sum_q and hits and keeps max_weight; two different views
    add up to the restated sum; gs_coverage_reset zeroes."""
    import coverage_restate as cr
    from gsplat import synth
    case = ("cfgA", 16, RECT_A, None)
    s, u, W, H, ref = _scene_of(oracle, "cfgA", 16)
    want, classes, _ = _restated(oracle, case)
    u2, rect2 = synth.orbit_camera(6, W, H).uniforms(W, H), (70, 60, 94, 83)  # a second camera, a rect across a tile corner
    want2, _ = cr.restate(oracle.render(s, u2, W, H, 16), s.shape[0], W, H, 16, rect2)
    assert (want2["hits"] > 0).sum() > 10 and not np.array_equal(want2["hits"] > 0, want["hits"] > 0)
    r = _mk(s, W, H, 16)
    zero = np.zeros(s.shape[0], cr.COVERAGE_DTYPE)
    _same(r.read_coverage(), zero, "before any frame")
    r.render_uniforms(u)
    r.wait()
    _same(r.read_coverage(), zero, "before any accumulate")
    assert r.accumulate_coverage(RECT_A) == classes["pixels"]
    _same(r.read_coverage(), want, "once")
    r.accumulate_coverage(RECT_A)
    twice = want.copy()
    twice["sum_q"] *= np.uint64(2)
    twice["hits"] *= np.uint32(2)
    _same(r.read_coverage(), twice, "twice")
    r.reset_coverage()
    _same(r.read_coverage(), zero, "reset")
    r.accumulate_coverage(RECT_A)
    r.render_uniforms(u2)
    r.wait()
    assert r.accumulate_coverage(rect2) == (rect2[2] - rect2[0]) * (rect2[3] - rect2[1])
    both = want.copy()
    both["sum_q"] += want2["sum_q"]
    both["hits"] += want2["hits"]
    both["max_weight"] = np.maximum(want["max_weight"], want2["max_weight"])
    _same(r.read_coverage(), both, "two views")
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("length", [10000, 9997], ids=["whole", "n9997"])
def test_state_coverage(oracle, length):
    """gs_state_coverage against a numpy predicate on the read-back planes: covered 1 and 0, both thresholds, the where filter,
    *matched, every op; and the refusals.  On cfgA whole (N a multiple of four) and on its first 9997 splats (N mod 4 = 1: the
    last thread of the pass goes splat by splat)."""
    from gsplat import _abi
    s, u, W, H, ref = _scene_of(oracle, "cfgA", 16)
    assert s.shape[0] == 10000
    s = np.ascontiguousarray(s[:length])
    n = s.shape[0]
    r = _mk(s, W, H, 16, state=True)
    r.render_uniforms(u)
    r.wait()
    r.accumulate_coverage()
    p = r.read_coverage()
    assert 100 < (p["hits"] > 0).sum() < n
    rng = np.random.default_rng(3)
    st = rng.integers(0, 256, n).astype(np.uint8)
    mw = np.float32(np.median(p["max_weight"][p["hits"] > 0]))
    ops = {_abi.GS_STATE_SET: lambda v, b: v | b, _abi.GS_STATE_CLEAR: lambda v, b: v & (~b & 0xFF), _abi.GS_STATE_TOGGLE: lambda v, b: v ^ b,
           _abi.GS_STATE_ASSIGN: lambda v, b: np.full_like(v, b)}
    cells = [(1, 0.0, True, (0, 0)), (1, 0.0, False, (0, 0)), (5, 0.0, True, (0, 0)), (1, float(mw), True, (0, 0)), (3, float(mw), False, (0x0C, 0x04)),
             (0, 0.0, True, (0, 0)), (1, 0.0, True, (0x30, 0x10))]
    for op, fn in ops.items():
        for bits in (0x02, 0xA4):
            for min_hits, min_weight, covered, where in cells:
                r.write_state(st)
                member = ((p["hits"] >= min_hits) & (p["max_weight"] >= np.float32(min_weight))) == covered
                member &= (st & where[0]) == where[1]
                matched = r.state_coverage(op, bits, min_hits, min_weight, covered, where)
                assert matched == int(member.sum()), (op, bits, min_hits, min_weight, covered, where)
                want = st.copy()
                want[member] = fn(st[member].astype(np.uint32), bits).astype(np.uint8)
                np.testing.assert_array_equal(r.read_state(), want, err_msg=str((op, bits, min_hits, min_weight, covered, where)))
    assert any(((p["hits"] >= c[0]) & (p["max_weight"] >= np.float32(c[1]))).sum() not in (0, n) for c in cells)
    # the planes and the frame are untouched by it
    np.testing.assert_array_equal(r.read_coverage().view(np.uint32), p.view(np.uint32))
    # refusals: nothing is applied
    r.write_state(st)
    L = _abi.load()
    m = ctypes.c_uint64(77)
    bad = [(1, float("nan"), 1, 0, 0, 1, 2), (1, -0.5, 1, 0, 0, 1, 2), (1, 0.0, 1, 0, 0, 1, 0x100), (1, 0.0, 1, 0, 0, 0, 2), (1, 0.0, 1, 0, 0, 5, 2),
           (1, 0.0, 1, 0x100, 0, 1, 2)]
    for a in bad:
        assert L.gs_state_coverage(r._ctx, *a, ctypes.byref(m)) == _abi.GS_ERR_INVALID_ARGUMENT, a
        assert b"gs_state_coverage" in L.gs_last_error()
    assert m.value == 77
    np.testing.assert_array_equal(r.read_state(), st)
    r.destroy()
    # a context without the plane: the state call is refused like the others, the accumulation and the read work
    q = _mk(s, W, H, 16)
    q.render_uniforms(u)
    q.wait()
    q.accumulate_coverage()
    np.testing.assert_array_equal(q.read_coverage().view(np.uint32), p.view(np.uint32))
    c, msg = code_of(lambda: q.state_coverage(_abi.GS_STATE_SET, 2))
    assert c == _abi.GS_ERR_INVALID_ARGUMENT and "GS_FLAG_SPLAT_STATE" in msg
    q.destroy()


@pytest.mark.gpu
def test_select_visible_and_hide_unseen(oracle):
    """select_visible then hide_selected: the next frame's lists hold exactly the splats they held minus the restated covered
    set.  hide_unseen after a whole-canvas accumulate: the next EXACT frame's rgba8 is bit-equal to the frame before (every
    removed splat has no accepted pair, and an entry with cond = 0 changes nothing)."""
    from gsplat import _abi
    case = ("cfgA", 16, RECT_A, "checker3")
    s, u, W, H, ref = _scene_of(oracle, "cfgA", 16)
    want, classes, _ = _restated(oracle, case)
    covered = np.flatnonzero(want["hits"] > 0)
    r = _mk(s, W, H, 16, exact=True, state=True)
    r.set_option(_abi.GS_OPT_TILE_CULL, 0)  # the reference's binning: a splat's instances depend on nothing but the splat
    r.render_uniforms(u)
    r.wait()
    listed = np.unique(r.read_buffer(_abi.GS_BUF_VALUES))
    assert np.isin(covered, listed).all()
    assert r.select_visible(RECT_A, _mask_of("checker3", W, H)) == covered.size > 50
    np.testing.assert_array_equal(np.flatnonzero(r.read_state() & _abi.GS_SPLAT_SELECTED), covered)
    assert r.hide_selected() == covered.size
    r.render_uniforms(u)
    r.wait()
    np.testing.assert_array_equal(np.unique(r.read_buffer(_abi.GS_BUF_VALUES)), np.setdiff1d(listed, covered))
    # a heavier threshold selects a subset
    r.unhide_all()
    r.clear_selection()
    r.render_uniforms(u)
    r.wait()
    heavy = np.flatnonzero(want["max_weight"] >= np.float32(0.2))
    assert 0 < heavy.size < covered.size
    assert r.select_visible(RECT_A, _mask_of("checker3", W, H), min_weight=0.2) == heavy.size
    np.testing.assert_array_equal(np.flatnonzero(r.read_state() & _abi.GS_SPLAT_SELECTED), heavy)
    r.clear_selection()
    # hide_unseen over the whole canvas changes no bit of the image
    r.set_option(_abi.GS_OPT_TILE_CULL, 1)
    r.render_uniforms(u)
    r.wait()
    before = r.read_rgba8()
    r.reset_coverage()
    assert r.accumulate_coverage() == W * H
    p = r.read_coverage()
    hidden = r.hide_unseen()
    assert hidden == int((p["hits"] == 0).sum()) and 0 < hidden < s.shape[0]
    assert int((p["hits"] == 0)[listed].sum()) > 0  # splats that were in a list and contributed to no pixel go too
    r.render_uniforms(u)
    r.wait()
    np.testing.assert_array_equal(r.read_rgba8(), before)
    assert r.stats()["num_visible"] <= int((p["hits"] > 0).sum())
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_coverage_disturbs_nothing(oracle, graph):
    from gsplat import _abi, synth
    s, _, W, H, _ = _scene_of(oracle, "cfgA", 16)
    u0, u1 = (synth.orbit_camera(k, W, H).uniforms(W, H) for k in (2, 6))
    a = _mk(s, W, H, 16)  # accumulates between its frames
    b = _mk(s, W, H, 16)  # never does
    for r in (a, b):
        r.set_option(_abi.GS_OPT_FRAME_GRAPH, graph)
        r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
        r.render_uniforms(u0)
        r.wait()
    taps = (_abi.GS_BUF_VALUES, _abi.GS_BUF_RANGES, _abi.GS_BUF_TILE_COUNTS, _abi.GS_BUF_GAUSSIAN_DATA, _abi.GS_BUF_RGB_F32)
    before = [a.read_rgba8()] + [a.read_buffer(t) for t in taps] + [timeless(a.stats())]
    a.accumulate_coverage(RECT_A)
    first = a.read_coverage()
    a.reset_coverage()
    a.accumulate_coverage(RECT_A)  # a second run: the same planes, whatever order the adds arrived in
    _same(a.read_coverage(), first, "two runs")
    after = [a.read_rgba8()] + [a.read_buffer(t) for t in taps] + [timeless(a.stats())]
    for x, y in zip(before[:-1], after[:-1]):
        np.testing.assert_array_equal(x, y)
    assert before[-1] == after[-1]
    for k in range(3):  # frames after an accumulate equal frames without one; the captured graph keeps being replayed
        for r in (a, b):
            r.render_uniforms(u1 if k % 2 == 0 else u0)
            r.wait()
        a.accumulate_coverage()
        np.testing.assert_array_equal(a.read_rgba8(), b.read_rgba8())
        np.testing.assert_array_equal(a.read_buffer(_abi.GS_BUF_RGB_F32), b.read_buffer(_abi.GS_BUF_RGB_F32))
        np.testing.assert_array_equal(a.read_buffer(_abi.GS_BUF_VALUES), b.read_buffer(_abi.GS_BUF_VALUES))
        assert timeless(a.stats()) == timeless(b.stats())
        assert a.stats()["graph_frames"] == (k + 2 if graph else 0)
    a.destroy()
    b.destroy()


@pytest.mark.gpu
def test_coverage_ring_and_slabs(oracle):
    """Three frames in flight: the call waits for and describes the LAST one.  Two slab contexts and a rect across their
    boundary: each reports its own pixels, and the merged planes are the whole-canvas restatement."""
    import gsplat
    from gsplat import synth
    from gsplat.multigpu import merge_coverage
    case = ("cfgA", 16, RECT_A, None)
    s, u, W, H, ref = _scene_of(oracle, "cfgA", 16)
    want, classes, _ = _restated(oracle, case)
    others = [synth.orbit_camera(k, W, H).uniforms(W, H) for k in (1, 7)]
    r = _mk(s, W, H, 16)
    for uu in others + [u]:
        r.render_uniforms(uu)
    assert r.accumulate_coverage(RECT_A) == classes["pixels"]
    assert r.stats()["frames_in_flight"] == 3 and r.stats()["frames"] == 3
    _same(r.read_coverage(), want, "three frames in flight")
    r.destroy()
    # PipelinedRenderer forwards to the owner of the splats: slot 0's frame
    p = gsplat.PipelinedRenderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(s), 16, frames_in_flight=2)
    p.render_uniforms(u)
    p.render_uniforms(others[0])
    assert p.accumulate_coverage(RECT_A) == classes["pixels"]
    _same(p.read_coverage(), want, "pipelined")
    p.reset_coverage()
    assert int(p.read_coverage()["hits"].sum()) == 0
    p.destroy()
    ntx = W // 16
    parts, px = [], []
    for cols in ((0, 5), (5, ntx)):
        sl = _mk(s, W, H, 16, cols=cols)
        sl.render_uniforms(u)
        px.append(sl.accumulate_coverage(RECT_A))
        parts.append(sl.read_coverage())
        assert sl.accumulate_coverage((0, 0, 8, 8) if cols[0] else (W - 8, 0, W, 8)) == 0  # a region that misses the slab: OK, nothing added
        _same(sl.read_coverage(), parts[-1], "missed slab")
        sl.destroy()
    bx = 5 * 16
    assert px == [(bx - RECT_A[0]) * (RECT_A[3] - RECT_A[1]), (RECT_A[2] - bx) * (RECT_A[3] - RECT_A[1])] and sum(px) == classes["pixels"]
    assert all(int(q["hits"].sum()) > 0 for q in parts)
    _same(merge_coverage(parts), want, "slabs merged")


@pytest.mark.gpu
def test_coverage_lifecycle_and_errors(oracle):
    from gsplat import _abi
    import coverage_restate as cr
    s, u, W, H, ref = _scene_of(oracle, "cfgA", 16)
    want, classes, _ = _restated(oracle, ("cfgA", 16, RECT_A, None))
    L = _abi.load()
    # before any upload: GS_ERR_NO_SCENE from all four
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(_abi.GsConfig), W, H, 16, _abi.GS_FLAG_SPLAT_STATE
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    n = ctypes.c_uint64()
    assert L.gs_coverage_accumulate(ctx, None, None) == _abi.GS_ERR_NO_SCENE
    assert L.gs_coverage_reset(ctx) == _abi.GS_ERR_NO_SCENE
    assert L.gs_coverage_read(ctx, None, 0, ctypes.byref(n)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_state_coverage(ctx, 1, 0.0, 1, 0, 0, 1, 2, None) == _abi.GS_ERR_NO_SCENE
    L.gs_destroy(ctx)
    r = _mk(s, W, H, 16, state=True)
    assert code_of(lambda: r.accumulate_coverage())[0] == _abi.GS_ERR_NO_FRAME  # after the upload, before any frame
    r.render_uniforms(u)
    r.wait()
    # bad regions: the message names the numbers; nothing is added
    reg = _abi.GsCoverRegion()
    reg.struct_size, reg.x0, reg.y0, reg.x1, reg.y1 = 8, 0, 0, 4, 4
    assert L.gs_coverage_accumulate(r._ctx, ctypes.byref(reg), None) == _abi.GS_ERR_INVALID_ARGUMENT and b"struct_size 8" in L.gs_last_error()
    c, msg = code_of(lambda: r.accumulate_coverage((0, 0, W + 1, H)))
    assert c == _abi.GS_ERR_INVALID_ARGUMENT and str(W + 1) in msg and "%u x %u" % (W, H) in msg
    c, msg = code_of(lambda: r.accumulate_coverage((0, 3, W, H + 2)))
    assert c == _abi.GS_ERR_INVALID_ARGUMENT and str(H + 2) in msg
    c, msg = code_of(lambda: r.accumulate_coverage((40, 7, 40, 9)))
    assert c == _abi.GS_ERR_INVALID_ARGUMENT and "empty" in msg and "[40, 40)" in msg
    assert code_of(lambda: r.accumulate_coverage((9, 30, 12, 20)))[0] == _abi.GS_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        r.accumulate_coverage(mask=np.zeros((H, W + 1), np.uint8))
    zero = np.zeros(s.shape[0], cr.COVERAGE_DTYPE)
    _same(r.read_coverage(), zero, "after the refusals")
    # the read's conventions are gs_state_list's
    assert L.gs_coverage_read(r._ctx, None, 0, None) == _abi.GS_ERR_INVALID_ARGUMENT
    _abi.check(L.gs_coverage_read(r._ctx, None, 0, ctypes.byref(n)))
    assert n.value == s.shape[0]
    buf = np.full(s.shape[0], 7, cr.COVERAGE_DTYPE)
    assert L.gs_coverage_read(r._ctx, buf.ctypes.data, s.shape[0] - 1, ctypes.byref(n)) == _abi.GS_ERR_INVALID_ARGUMENT
    assert str(s.shape[0]).encode() in L.gs_last_error() and (buf["hits"] == 7).all()
    # an all-zero mask: pixels 0, nothing added; then the real thing
    assert r.accumulate_coverage(RECT_A, np.zeros((H, W), np.uint8)) == 0
    _same(r.read_coverage(), zero, "empty mask")
    assert r.accumulate_coverage(RECT_A) == classes["pixels"]
    _same(r.read_coverage(), want, "after the errors")
    # state calls and transforms leave the planes alone
    r.select_sphere((0, 0, 0), 1.0)
    r.translate_selected((0.1, 0, 0))
    _same(r.read_coverage(), want, "after a state call and a transform")
    r.clear_selection()
    # an upload drops the planes and the frame
    arr = np.ascontiguousarray(s, dtype=np.float32)
    _abi.check(L.gs_upload_splats(r._ctx, arr.ctypes.data, arr.shape[0]))
    assert code_of(lambda: r.accumulate_coverage())[0] == _abi.GS_ERR_NO_FRAME
    _same(r.read_coverage(), zero, "after an upload")
    r.render_uniforms(u)
    r.wait()
    r.accumulate_coverage(RECT_A)
    _same(r.read_coverage(), want, "a frame after the upload")
    # so does a compaction (the records are not carried)
    keep = r.state_coverage(_abi.GS_STATE_SET, 0x40, 1, 0.0, True)
    assert keep == int((want["hits"] > 0).sum())
    ids = r.compact(0x40, 0x40)
    assert ids.size == keep
    assert code_of(lambda: r.accumulate_coverage())[0] == _abi.GS_ERR_NO_FRAME
    _same(r.read_coverage(), np.zeros(keep, cr.COVERAGE_DTYPE), "after a compaction")
    r.render_uniforms(u)
    r.wait()
    r.accumulate_coverage(RECT_A)
    got = r.read_coverage()
    assert got.shape == (keep,)
    _same(got, want[ids], "the compacted scene shows what the covered splats showed")
    r.destroy()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_node_host_coverage_matches_python(tmp_path):
    from gsplat import _abi, synth
    n, W, H, ts = 8000, 200, 120, 16
    s = scene(n)
    u = synth.orbit_camera(4, W, H).uniforms(W, H)
    rect = (13, 9, 171, 103)
    mask = _mask_of("checker3", W, H)
    rec, ub, mb, out = (str(tmp_path / f) for f in ("rec.bin", "u.bin", "mask.bin", "cov.bin"))
    s.tofile(rec)
    u.tofile(ub)
    mask.tofile(mb)
    info = run_node("coverage_check.js", (rec, n, W, H, ts, ub) + rect + (mb, out))
    r = _mk(s, W, H, ts, state=True)
    r.render_uniforms(u)
    r.wait()
    pixels = r.accumulate_coverage(rect, mask)
    p = r.read_coverage()
    matched = r.state_coverage(_abi.GS_STATE_SET, _abi.GS_SPLAT_SELECTED, 2, 0.05, True)
    unseen = r.state_coverage(_abi.GS_STATE_SET, _abi.GS_SPLAT_HIDDEN, covered=False)
    state = r.read_state()
    r.destroy()
    raw = np.fromfile(out, dtype=np.uint8)
    assert raw.size == n * 16 + n and info["n"] == n
    np.testing.assert_array_equal(raw[: n * 16].view(np.uint32), p.view(np.uint32))
    np.testing.assert_array_equal(raw[n * 16:], state)
    assert info["whole"] == W * H and info["pixels"] == pixels == int(mask[rect[1]:rect[3], rect[0]:rect[2]].sum())
    assert info["matched"] == matched > 0 and info["unseen"] == unseen > 0
    assert info["zeroBefore"] is True and info["zeroAfterReset"] is True
    k = int(np.argmax(p["hits"]))
    assert info["most_hits"]["id"] == k and info["most_hits"]["hits"] == int(p["hits"][k]) > 0
    assert int(info["most_hits"]["sumQ"]) == int(p["sum_q"][k]) and np.float32(info["most_hits"]["maxWeight"]) == p["max_weight"][k]
    assert info["errors"] == {"outside": "-1", "empty": "-1"}


@pytest.mark.gpu
def test_coverage_config_b_full_size():
    """Config B (6.1 M splats, 1080p), the product path, the whole canvas.  A consistency check, not a restatement: over a lattice
    of pixels given as the mask, hits summed over the splats equals hit_count summed over gs_pick's answers for the same pixels
    and the largest max_weight is the largest of theirs; the unmasked whole-canvas planes dominate the lattice's record by
    record and stay the same from run to run."""
    import torch
    import gsplat
    from gsplat import synth
    from gpu_checks import make_renderer, orbit_uniforms
    n, W, H, ts = 6_100_000, 1920, 1080, 16
    dev = synth.bicycle_like_torch(n, synth.BASE_SEED + 1, "cuda")
    torch.cuda.synchronize()
    pg = gsplat.PackedGaussians.__new__(gsplat.PackedGaussians)
    pg.numGaussians, pg.gaussiansBuffer, pg.sphericalHarmonicsDegree = n, dev, 3
    r = make_renderer(pg, W, H, ts)
    u = orbit_uniforms(W, H, step=0)
    r.render_uniforms(u)
    r.wait()  # the first frame grows the capacity
    r.render_uniforms(u)
    r.wait()
    assert r.stats()["tight_binning"] == 1
    ys, xs = np.arange(3, H, 7), np.arange(5, W, 9)  # 154 x 213 = 32 802 pixels: one gs_pick call
    mask = np.zeros((H, W), np.uint8)
    mask[np.ix_(ys, xs)] = 1
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    res = r.pick(np.stack([xx.ravel(), yy.ravel()], axis=1).astype(np.uint32))
    assert r.accumulate_coverage(mask=mask) == ys.size * xs.size == res.size
    lat = r.read_coverage()
    assert int(lat["hits"].astype(np.uint64).sum()) == int(res["hit_count"].astype(np.uint64).sum()) > 100000
    assert lat["max_weight"].max().view(np.uint32) == res["max_weight"].max().view(np.uint32)
    r.reset_coverage()
    assert r.accumulate_coverage() == W * H
    full = r.read_coverage()
    print("\ncfg-B coverage: %d pairs over the canvas, %d covered splats of %d, most pairs of one splat %d"
          % (int(full["hits"].astype(np.uint64).sum()), int((full["hits"] > 0).sum()), n, int(full["hits"].max())))
    assert (full["hits"] >= lat["hits"]).all() and (full["sum_q"] >= lat["sum_q"]).all() and (full["max_weight"] >= lat["max_weight"]).all()
    assert full["max_weight"].max() <= np.float32(0.99)
    r.reset_coverage()
    r.accumulate_coverage()
    np.testing.assert_array_equal(r.read_coverage().view(np.uint32), full.view(np.uint32))
    r.destroy()
    del dev
