"""Neighbourhoods: count the splats within a radius, select by that count (include/gsplat/gs_abi.h "neighbourhoods").

The reference every GPU answer is held to is tests/neigh_restate.py: a numpy brute force over all pairs with the header's f32
expression.  The CPU tests pin the restatement by hand (a lattice whose neighbours sit exactly on the radius, the 3-4-5 pair) and
the ABI.  The GPU tests compare with np.array_equal on uint32 -- there is no tolerance anywhere -- over grids of many cells and of
one, filters, special floats, the lifecycle of the plane, the selection by count, the editor's verbs, the work budget, the refusals
and the Node host.
"""
import ctypes
import functools
import re

import numpy as np
import pytest

import neigh_restate as nr
import state_restate as sr
from conftest import scene
from support import F, NODE, SLAB_COLS, c_layout, cached, code_of, frame_taps, host_sources, mk, run_node, state_ref, state_scene, timeless

_mk = functools.partial(mk, state=True)
NONE = 2**32 - 1
LIMITS = (1, 3, NONE)
OPS = (sr.SET, sr.CLEAR, sr.TOGGLE, sr.ASSIGN)


def lattice_pos():
    """6 x 6 x 6 points, spacing 0.25, offset 3.0: every coordinate and every difference is exact in f32."""
    k = np.arange(6, dtype=F) * F(0.25) + F(3.0)
    return np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3).astype(F)


def records(pos):
    """Records of the synthetic scene with their centres replaced by `pos`."""
    pos = np.asarray(pos, F)
    rec = np.array(scene(10000)[:pos.shape[0]], dtype=F, copy=True)
    rec[:, 0:3] = pos
    return np.ascontiguousarray(rec)


def want_counts(key, pos, radius, src=None, qry=None):
    """The restatement without a limit, once per key and session (a limit is a minimum on top of it)."""
    return cached(("neigh", key, float(radius)), lambda: nr.counts(pos, radius, src, qry))


def limited(c, limit):
    return np.minimum(c.astype(np.uint64), limit).astype(np.uint32)


def special_pos():
    """1000 centres of the ragged scene with a NaN, +inf and -inf coordinate, -0.0, a denormal coordinate, two pairs of exact
    duplicates (one of them of non-finite splats, which count nothing)."""
    from gsplat import synth
    p = np.array(synth.bicycle_like(3001)[:1000, 0:3], dtype=F, copy=True)
    p[10, 0] = np.nan
    p[20, 1] = np.inf
    p[30, 2] = -np.inf
    p[40, 0] = -0.0
    p[50, 1] = 1e-45
    p[60] = p[61]
    p[70] = p[71] = (np.nan, 0.0, 0.0)
    p[80] = p[81] = p[82]
    return p


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_restatement_is_pinned():
    """The lattice at radius 0.25 counts 6 inside, 5 on faces, 4 on edges, 3 at corners, and nothing at the float below 0.25; the
    pair (1, 1, 1), (1.375, 1.5, 1) is 0.625 apart exactly; and the restatement equals a float64 per-point loop on the lattice."""
    p = lattice_pos()
    c = nr.counts(p, 0.25)
    assert c.dtype == np.uint32
    assert dict(zip(*[x.tolist() for x in np.unique(c, return_counts=True)])) == {3: 8, 4: 48, 5: 96, 6: 64}
    assert not nr.counts(p, np.nextafter(F(0.25), F(0))).any()
    pair = np.array([[1, 1, 1], [1.375, 1.5, 1]], F)
    assert nr.counts(pair, 0.625).tolist() == [1, 1]
    assert nr.counts(pair, np.nextafter(F(0.625), F(0))).tolist() == [0, 0]
    p64 = p.astype(np.float64)
    for radius in (0.25, 0.36, 0.5, 0.75):
        loop = [int(sum(1 for j in range(len(p64)) if j != i and ((p64[j] - p64[i]) ** 2).sum() <= radius * radius)) for i in range(len(p64))]
        assert nr.counts(p, radius).tolist() == loop, radius
    # limit, filters, self-exclusion by index, special floats
    assert nr.counts(p, 0.25, limit=4).tolist() == np.minimum(c, 4).tolist()
    src = np.arange(216) % 2 == 0
    got = nr.counts(p, 0.25, src=src, qry=~src)
    assert not got[src].any() and got.tolist() == np.where(src, 0, nr.counts(p, 0.25, src=src)).tolist() and got.any()
    dup = np.array([[1, 2, 3], [1, 2, 3], [np.nan, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [np.inf, 0, 0]], F)
    assert nr.counts(dup, 0.0).tolist() == [1, 1, 0, 0, 0, 0]
    assert nr.counts(dup, 1e-40).tolist() == [1, 1, 0, 0, 0, 0]  # a denormal radius: its square is 0
    assert nr.counts(dup, 0.0, src=[1, 0, 0, 0, 0, 0], qry=[0, 1, 0, 0, 0, 0]).tolist() == [0, 1, 0, 0, 0, 0]
    assert nr.member([0, 1, 2, 3], 1, 2).tolist() == [False, True, True, False]
    assert nr.member([0, 1, 2, 3], 2, 1, inside=False).all()


def test_neigh_abi(tmp_path):
    """The three symbols are exported and listed; gs_neigh and gs_neigh_info are 40 bytes with the same offsets in the compiled
    header and in ctypes; GS_ABI_VERSION is still 3 and GS_ATTR_COUNT still 16; the header states the expression, the inclusive
    comparison and the plane's lifetime; the hosts declare the calls; a null context is refused by name."""
    import gsplat
    from gsplat import _abi, neighbours
    L = _abi.load()
    names = ("gs_neigh_count", "gs_neigh_read", "gs_state_neigh")
    for name in names:
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    q_fields = [n for n, _ in _abi.GsNeigh._fields_]
    i_fields = [n for n, _ in _abi.GsNeighInfo._fields_]
    assert q_fields == ["struct_size", "radius", "limit", "src_mask", "src_value", "qry_mask", "qry_value", "reserved", "max_candidates"]
    assert i_fields == ["queried", "sources", "candidates", "cells", "cell_edge"]
    prog = 'printf("%d %d %zu %zu", GS_ABI_VERSION, (int)GS_ATTR_COUNT, sizeof(gs_neigh), sizeof(gs_neigh_info));'
    prog += "".join('printf(" %%zu", offsetof(gs_neigh, %s));' % n for n in q_fields)
    prog += "".join('printf(" %%zu", offsetof(gs_neigh_info, %s));' % n for n in i_fields)
    prog += 'printf(" %d %d", GS_NEIGH_DEFAULT_CANDIDATES >= GS_NEIGH_SLICE_CANDIDATES, (int)GS_ERR_CAPACITY);'
    out = c_layout(tmp_path, "neigh_layout", prog)
    assert out[0] == 3 and L.gs_abi_version() == 3 and out[1] == 16 == _abi.GS_ATTR_COUNT
    assert out[2] == 40 == ctypes.sizeof(_abi.GsNeigh) and out[3] == 40 == ctypes.sizeof(_abi.GsNeighInfo)
    assert out[4:13] == [getattr(_abi.GsNeigh, n).offset for n in q_fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32]
    assert out[13:18] == [getattr(_abi.GsNeighInfo, n).offset for n in i_fields] == [0, 8, 16, 24, 36]
    assert out[18:] == [1, _abi.GS_ERR_CAPACITY]
    rjs, idx, dts, napi, hdr = host_sources()
    assert re.search(r"#define GS_ABI_VERSION 3\b", hdr)
    for name in names:
        assert re.search(r"int32_t %s\(gs_ctx\*" % name, hdr)
    sec = hdr[hdr.index("---- neighbourhoods"):hdr.index("Tuning / profiling knobs")]
    for text in ("d2 = (dx dx + dy dy) + dz dz", "d = p_j - p_i", "r2 = radius * radius", "INCLUSIVE", "u32[N]", "DROPPED", "gs_upload_*",
                 "gs_share_splats", "gs_compact", "counts again", "GS_ERR_CAPACITY"):
        assert text in sec, text
    for fn in ("neighCount", "neighRead", "stateNeigh"):
        assert re.search(r"\b%s\(" % fn, dts) and re.search(r"\b%s\(" % fn, rjs) and '{"%s", js_' % fn in napi
    q, info, n = _abi.GsNeigh(), _abi.GsNeighInfo(), ctypes.c_uint64()
    calls = {"gs_neigh_count": lambda: L.gs_neigh_count(None, ctypes.byref(q), ctypes.byref(info)),
             "gs_neigh_read": lambda: L.gs_neigh_read(None, None, 0, ctypes.byref(n)),
             "gs_state_neigh": lambda: L.gs_state_neigh(None, 0, 1, 1, 0, 0, 1, 2, None)}
    for name, call in calls.items():
        assert call() == _abi.GS_ERR_INVALID_ARGUMENT
        msg = L.gs_last_error()
        assert name.encode() in msg and b"null ctx" in msg
    assert gsplat.neighbours is neighbours
    for fn in ("count", "read", "select", "select_isolated", "grow_selection", "shrink_selection"):
        assert callable(getattr(neighbours, fn))
    for cls in (gsplat.Renderer, gsplat.PipelinedRenderer):
        assert not [m for m in dir(cls) if not m.startswith("_") and "neigh" in m.lower()]


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def _check_scene(key, rec, radii_cells):
    """count + read against the restatement for every radius and limit; radii_cells: radius -> whether the grid must have more
    than one cell on every axis (True) or exactly one (False)."""
    from gsplat import neighbours
    n = rec.shape[0]
    r = _mk(rec, 64, 64, 16)
    assert not neighbours.read(r).any() and neighbours.read(r).shape == (n,)  # before any count
    for radius, many in radii_cells.items():
        want = want_counts(key, rec, radius)
        for limit in LIMITS:
            info = neighbours.count(r, radius, limit)
            got = neighbours.read(r)
            assert got.dtype == np.uint32
            assert np.array_equal(got, limited(want, limit)), (key, radius, limit, int((got != limited(want, limit)).sum()))
            assert info["queried"] == info["sources"] == n
            assert info["candidates"] >= int(want.sum()) + n  # every neighbour and self were candidates
            cells = info["cells"]
            assert (min(cells) > 1) if many else (cells == (1, 1, 1)), (radius, cells)
            assert info["cell_edge"] >= 1.001 * radius
        print("%s radius %g: mean count %.3f, cells %s, candidates %d" % (key, radius, want.mean(), info["cells"], info["candidates"]))
    r.destroy()


@pytest.mark.gpu
def test_counts_ragged_scene():
    """synth.bicycle_like(3001) at radii that give hundreds of cells per axis, tens, a few, and one (1e3: the all-pairs path)."""
    from gsplat import synth
    rec = synth.bicycle_like(3001)
    _check_scene("ragged", rec, {0.1: True, 0.5: True, 2.0: True, 1e3: False})
    assert want_counts("ragged", rec, 0.1).mean() < 1 < want_counts("ragged", rec, 0.5).mean()
    assert (want_counts("ragged", rec, 1e3) == 3000).all()


@pytest.mark.gpu
def test_counts_length_no_multiple():
    """scene(10000)[:9997]: the length is no multiple of 4, 64 or 256."""
    rec = np.ascontiguousarray(scene(10000)[:9997])
    _check_scene("cfgA9997", rec, {0.25: True})
    assert want_counts("cfgA9997", rec, 0.25).max() > 3


@pytest.mark.gpu
def test_lattice_and_345_pair():
    """Equality at r2, and neighbours exactly one cell edge apart across cell borders."""
    from gsplat import neighbours
    p = lattice_pos()
    r = _mk(records(p), 64, 64, 16)
    for radius in (0.25, float(np.nextafter(F(0.25), F(0))), 0.36, 0.5):
        neighbours.count(r, radius)
        assert np.array_equal(neighbours.read(r), nr.counts(p, radius)), radius
    neighbours.count(r, 0.25)
    c = neighbours.read(r)
    assert dict(zip(*[x.tolist() for x in np.unique(c, return_counts=True)])) == {3: 8, 4: 48, 5: 96, 6: 64}
    neighbours.count(r, float(np.nextafter(F(0.25), F(0))))
    assert not neighbours.read(r).any()
    r.destroy()
    pair = np.array([[1, 1, 1], [1.375, 1.5, 1]], F)
    r = _mk(records(pair), 64, 64, 16)
    neighbours.count(r, 0.625)
    assert neighbours.read(r).tolist() == [1, 1]
    neighbours.count(r, float(np.nextafter(F(0.625), F(0))))
    assert neighbours.read(r).tolist() == [0, 0]
    r.destroy()


@pytest.mark.gpu
def test_blocked_table():
    """More than 2^24 cells: the cell table is indexed by blocks of consecutive keys and a cell's run is found by binary search inside
    its block.  The lattice with two far splats (about 970 cells per axis, neighbours exactly one cell edge apart), and the ragged
    scene shrunk to a fifth between two far splats (a dense core in a fine grid), with and without filters."""
    from gsplat import neighbours, synth
    ends = np.array([[-120, -121, -122], [123, 122, 121]], F)
    # ... and 200 splats within 0.005 of (5, 5, 5), the middle of a cell at these radii: whole waves whose queries share a cell
    knot = (F(5.0) + np.random.default_rng(11).uniform(-0.005, 0.005, (200, 3))).astype(F)
    p = np.concatenate([lattice_pos(), knot, ends])
    r = _mk(records(p), 64, 64, 16)
    for radius in (0.25, float(np.nextafter(F(0.25), F(0))), 0.36, 0.5):
        want = nr.counts(p, radius)
        assert (want[216:416] == 199).all()
        for limit in LIMITS:
            info = neighbours.count(r, radius, limit)
            assert min(info["cells"]) > 256 and info["cells"][0] * info["cells"][1] * info["cells"][2] > 2**24, info
            assert np.array_equal(neighbours.read(r), limited(want, limit)), (radius, limit)
    r.destroy()
    p = np.concatenate([synth.bicycle_like(3001)[:, 0:3] * F(0.2), ends / F(4)]).astype(F)
    n = p.shape[0]
    st = (np.arange(n) % 5).astype(np.uint8)
    r = _mk(records(p), 64, 64, 16)
    r.write_state(st)
    for radius in (0.06, 0.1):
        want = nr.counts(p, radius)
        for limit in LIMITS:
            info = neighbours.count(r, radius, limit)
            assert min(info["cells"]) > 256 and info["cells"][0] * info["cells"][1] * info["cells"][2] > 2**24, info
            assert np.array_equal(neighbours.read(r), limited(want, limit)), (radius, limit)
            neighbours.count(r, radius, limit, source=(7, 1), query=(7, 2))
            assert np.array_equal(neighbours.read(r), nr.counts(p, radius, st == 1, st == 2, limit)), (radius, limit)
        assert want.mean() > 0.5
        print("blocked table, radius %g: mean count %.3f, cells %s, candidates %d" % (radius, want.mean(), info["cells"], info["candidates"]))
    r.destroy()


@pytest.mark.gpu
def test_filters():
    from gsplat import neighbours, synth
    rec = synth.bicycle_like(3001)
    n = rec.shape[0]
    st = (np.arange(n) % 5).astype(np.uint8)
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    for radius in (0.5, 2.0):
        for limit in LIMITS:
            # disjoint sources and queries
            info = neighbours.count(r, radius, limit, source=(7, 1), query=(7, 2))
            want = nr.counts(rec, radius, st == 1, st == 2, limit)
            assert np.array_equal(neighbours.read(r), want) and want.any()
            assert (info["sources"], info["queried"]) == (int((st == 1).sum()), int((st == 2).sum()))
            # the same filter on both sides
            info = neighbours.count(r, radius, limit, source=(1, 0), query=(1, 0))
            even = (st & 1) == 0
            assert np.array_equal(neighbours.read(r), nr.counts(rec, radius, even, even, limit))
            assert info["sources"] == info["queried"] == int(even.sum())
    # no source at all: GS_OK and zeros
    info = neighbours.count(r, 0.5, source=(0xFF, 0xEE))
    assert info["sources"] == 0 and info["queried"] == n and not neighbours.read(r).any()
    info = neighbours.count(r, 0.5, query=(0xFF, 0xEE))
    assert info["queried"] == 0 and not neighbours.read(r).any()
    np.testing.assert_array_equal(r.read_state(), st)
    r.destroy()
    # a query that is no source is not self-excluded by accident: a duplicate pair, one a source, one a query
    p = np.array(rec[:100, 0:3], copy=True)
    p[1] = p[0]
    r = _mk(records(p), 64, 64, 16)
    st = np.zeros(100, np.uint8)
    st[0], st[1] = 1, 2
    r.write_state(st)
    neighbours.count(r, 0.0, source=(3, 1), query=(3, 2))
    got = neighbours.read(r)
    assert got[1] == 1 and got.sum() == 1
    r.destroy()


@pytest.mark.gpu
def test_special_floats():
    from gsplat import neighbours
    p = special_pos()
    n = p.shape[0]
    far = np.concatenate([p, np.array([[1e6, 1e6, -1e6]], F)])  # a far outlier coarsens (or is clamped by) the grid
    r, rf = _mk(records(p), 64, 64, 16), _mk(records(far), 64, 64, 16)
    for radius in (0.5, 0.1, 0.0, 1e-40):
        want = nr.counts(p, radius)
        for limit in (1, NONE):
            neighbours.count(r, radius, limit)
            got = neighbours.read(r)
            assert np.array_equal(got, limited(want, limit)), (radius, limit)
            neighbours.count(rf, radius, limit)
            gf = neighbours.read(rf)
            assert np.array_equal(gf[:n], got) and gf[n] == 0, (radius, limit)
        for i in (10, 20, 30, 70, 71):  # non-finite: no neighbours, nobody's neighbour
            assert got[i] == 0
    neighbours.count(r, 0.0)
    got = neighbours.read(r)
    assert got[60] == got[61] == 1 and got[80] == got[81] == got[82] == 2 and got.sum() == 8  # radius 0: only the duplicates
    neighbours.count(r, 1e-40)  # a denormal radius whose square is 0 behaves as radius 0
    assert np.array_equal(neighbours.read(r), got)
    r.destroy()
    rf.destroy()


@pytest.mark.gpu
def test_lifecycle():
    """The plane on a slab context and on a borrower; after translate_selected the counts are those of the exported positions; the
    plane reads zero after compact and after a re-upload."""
    from gsplat import _abi, neighbours, synth
    rec = synth.bicycle_like(3001)
    n = rec.shape[0]
    want = want_counts("ragged", rec, 0.5)
    owner = _mk(rec, 64, 64, 16)
    assert not neighbours.read(owner).any()
    slab = _mk(rec, 256, 256, 16, cols=SLAB_COLS[16])
    neighbours.count(slab, 0.5)
    assert np.array_equal(neighbours.read(slab), want)
    slab.destroy()
    borrower = _mk(rec, 64, 64, 16, share_with=owner)
    assert not neighbours.read(borrower).any()
    neighbours.count(borrower, 0.5)
    assert np.array_equal(neighbours.read(borrower), want)
    assert not neighbours.read(owner).any()  # the borrower keeps its own plane
    borrower.destroy()
    # state calls and transforms leave the plane; a new count sees the moved splats
    neighbours.count(owner, 0.5)
    assert owner.select_sphere((0, 0, 0), 1.5) > 100
    owner.translate_selected((0.3, -0.2, 0.1))
    assert np.array_equal(neighbours.read(owner), want)
    moved = owner.export_splats()
    assert not np.array_equal(moved[:, 0:3], rec[:, 0:3])
    neighbours.count(owner, 0.5)
    assert np.array_equal(neighbours.read(owner), nr.counts(moved, 0.5))
    # compact and a re-upload drop the plane
    st = (np.arange(n) % 3 == 0).astype(np.uint8) * 4
    owner.write_state(st)
    kept = owner.compact(4, 4)
    assert kept.size == int((st == 4).sum())
    assert neighbours.read(owner).shape == (kept.size,) and not neighbours.read(owner).any()
    neighbours.count(owner, 0.5)
    assert np.array_equal(neighbours.read(owner), nr.counts(moved[kept], 0.5)) and neighbours.read(owner).any()
    arr = np.ascontiguousarray(rec[:2000])
    _abi.check(owner._L.gs_upload_splats(owner._ctx, arr.ctypes.data, 2000))
    assert neighbours.read(owner).shape == (2000,) and not neighbours.read(owner).any()
    owner.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_counts_disturb_no_frame(graph):
    """A frame rendered before and after a count (and a selection by it that changes nothing), direct and graph-replayed, is
    byte-identical in every tap, and its statistics are unchanged."""
    from gsplat import _abi, neighbours
    s, u, W, H = state_scene("ragged")
    a, b = _mk(s, W, H, 8), _mk(s, W, H, 8)
    for r in (a, b):
        r.set_option(_abi.GS_OPT_FRAME_GRAPH, graph)
    want = want_counts("ragged", s, 0.5)
    for rep in range(2):
        before = frame_taps(a, u, False)
        frame_taps(b, u, False)
        for _ in range(3):  # three frames in flight on both; no wait: the count drains the ring
            a.render_uniforms(u)
            b.render_uniforms(u)
        neighbours.count(a, 0.5)
        assert np.array_equal(neighbours.read(a), want)
        assert neighbours.select(a, 5, 1, op=sr.SET, bits=sr.HIDDEN) == 0  # the empty range
        ta, tb = frame_taps(a, u, False), frame_taps(b, u, False)
        for k in ta:
            np.testing.assert_array_equal(ta[k], tb[k], err_msg=k)
            np.testing.assert_array_equal(ta[k], before[k], err_msg=k)
        assert timeless(a.stats()) == timeless(b.stats())
    if graph:
        assert a.stats()["graph_frames"] == b.stats()["graph_frames"] > 0
    a.destroy()
    b.destroy()


@pytest.mark.gpu
def test_state_neigh():
    """matched and the plane against the restatement for every op, inside 0 and 1, a where filter and the empty range."""
    from gsplat import neighbours, synth
    rec = synth.bicycle_like(3001)
    n = rec.shape[0]
    c = want_counts("ragged", rec, 0.5)
    st = np.random.default_rng(7).integers(0, 256, n).astype(np.uint8)
    r = _mk(rec, 64, 64, 16)
    neighbours.count(r, 0.5)
    ranges = [(0, 0), (1, 4), (5, NONE), (0, NONE), (4, 1), (int(c.max()), int(c.max()))]
    for k, (lo, hi) in enumerate(ranges):
        for inside in (True, False):
            for op in OPS:
                bits = (0x02, 0xA4)[(k + op) % 2]
                where = ((0, 0), (0x0C, 0x04), (0x30, 0x10))[(k + op + int(inside)) % 3]
                r.write_state(st)
                member = nr.member(c, lo, hi, inside)
                new, matched = sr.apply_region(st, member, op, bits, where)
                cell = (lo, hi, inside, op, bits, where)
                assert neighbours.select(r, lo, hi, inside, where, op, bits) == matched, cell
                np.testing.assert_array_equal(r.read_state(), new, err_msg=str(cell))
                if lo > hi:
                    assert member.sum() == (0 if inside else n)
    assert np.array_equal(neighbours.read(r), c)  # the selection only reads the plane
    r.destroy()


@pytest.mark.gpu
def test_verbs():
    from gsplat import neighbours, synth
    rec = synth.bicycle_like(3001)
    n = rec.shape[0]
    r = _mk(rec, 64, 64, 16)
    # floaters: fewer than k others within the radius, among the splats that pass `where`
    c = want_counts("ragged", rec, 0.5)
    for k in (1, 3):
        r.write_state(np.zeros(n, np.uint8))
        assert neighbours.select_isolated(r, 0.5, k) == int((c < k).sum()) > 0
        np.testing.assert_array_equal(r.read_state(), np.where(c < k, sr.SELECTED, 0).astype(np.uint8))
    st = ((np.arange(n) % 4 == 0) * 8).astype(np.uint8)
    keep = st == 8
    r.write_state(st)
    ck = nr.counts(rec, 0.5, keep, keep)
    assert neighbours.select_isolated(r, 0.5, 2, where=(8, 8)) == int((keep & (ck < 2)).sum()) > 0
    np.testing.assert_array_equal(r.read_state(), np.where(keep & (ck < 2), st | sr.SELECTED, st).astype(np.uint8))
    assert neighbours.select_isolated(r, 0.5, 0) == 0
    # grow and shrink: hidden splats are neither added nor do they hold the rim back
    hidden = np.arange(n) % 7 == 3
    inside = sr.member(sr.SPHERE, rec, 64, 64, a=(0, 0, 0), b=(1.5, 0, 0))
    st = np.where(hidden, sr.HIDDEN, 0).astype(np.uint8)
    st[inside & ~hidden] |= sr.SELECTED
    sel, free = (st & sr.SELECTED) != 0, st == 0
    r.write_state(st)
    near = nr.counts(rec, 0.4, sel, free, 1) == 1
    assert neighbours.grow_selection(r, 0.4) == int(near.sum()) > 0
    grown = np.where(near, st | sr.SELECTED, st).astype(np.uint8)
    np.testing.assert_array_equal(r.read_state(), grown)
    r.write_state(st)
    rim = nr.counts(rec, 0.4, free, sel, 1) == 1
    assert 0 < int(rim.sum()) < int(sel.sum())
    assert neighbours.shrink_selection(r, 0.4) == int(rim.sum())
    np.testing.assert_array_equal(r.read_state(), np.where(rim, st & ~np.uint8(sr.SELECTED), st).astype(np.uint8))
    r.destroy()


@pytest.mark.gpu
def test_grow_then_hide_frame(oracle):
    """select_sphere, grow_selection, hide_selected on the ragged scene at tile 8: the next EXACT frame equals the oracle's frame of
    the scene with those splats hidden, in every tap."""
    from gpu_checks import check_stages
    from gsplat import _abi, neighbours
    s, u, W, H = state_scene("ragged")
    inside = sr.member(sr.SPHERE, s, W, H, a=(0, 0, 0), b=(1.0, 0, 0))
    near = nr.counts(s, 0.3, inside, ~inside, 1) == 1
    assert 0 < inside.sum() and 0 < near.sum() and (inside | near).sum() < s.shape[0]
    state = np.where(inside | near, sr.HIDDEN | sr.SELECTED, 0).astype(np.uint8)
    ref = state_ref(oracle, "ragged", 8, "neigh_grown_sphere", state)
    r = _mk(s, W, H, 8, exact=True)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    assert r.select_sphere((0, 0, 0), 1.0) == int(inside.sum())
    assert neighbours.grow_selection(r, 0.3) == int(near.sum())
    assert r.hide_selected() == int((inside | near).sum())
    np.testing.assert_array_equal(r.read_state(), state)
    r.render_uniforms(u, debug=True)
    r.wait()
    check_stages(r, ref, True, debug=True)
    r.destroy()


@pytest.mark.gpu
def test_budget():
    """max_candidates = 1 on a scene with two coincident splats is refused with GS_ERR_CAPACITY, the message carries both numbers
    and the plane still holds the previous count; the default budget accepts the same call."""
    from gsplat import _abi, neighbours, synth
    p = np.array(synth.bicycle_like(3001)[:500, 0:3], copy=True)
    p[1] = p[0]
    r = _mk(records(p), 64, 64, 16)
    info = neighbours.count(r, 0.5)
    prev = neighbours.read(r)
    assert np.array_equal(prev, nr.counts(p, 0.5)) and prev.any()
    code, msg = code_of(lambda: neighbours.count(r, 0.0, max_candidates=1))
    info0 = neighbours.count(r, 0.0, max_candidates=0)
    assert info0["candidates"] >= 502  # every splat is its own candidate, the pair each other's
    assert code == _abi.GS_ERR_CAPACITY and "gs_neigh_count" in msg
    assert str(info0["candidates"]) in msg and "max_candidates = 1 " in msg + " ", msg
    got = neighbours.read(r)
    assert got[0] == got[1] == 1 and got.sum() == 2
    neighbours.count(r, 0.5)
    code, msg = code_of(lambda: neighbours.count(r, 0.5, max_candidates=info["candidates"] - 1))
    assert code == _abi.GS_ERR_CAPACITY and str(info["candidates"]) in msg and str(info["candidates"] - 1) in msg
    assert np.array_equal(neighbours.read(r), prev)  # the plane is left as it was
    assert neighbours.count(r, 0.5, max_candidates=info["candidates"])["candidates"] == info["candidates"]
    r.destroy()


@pytest.mark.gpu
def test_neigh_refusals():
    from gsplat import _abi, neighbours, synth
    L = _abi.load()
    INV = _abi.GS_ERR_INVALID_ARGUMENT
    rec = synth.bicycle_like(3001)
    n = rec.shape[0]
    info, nn, m = _abi.GsNeighInfo(), ctypes.c_uint64(), ctypes.c_uint64(77)

    def query(**kw):
        q = _abi.GsNeigh()
        q.struct_size, q.radius, q.limit = ctypes.sizeof(_abi.GsNeigh), 0.5, 3
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    # before any upload: GS_ERR_NO_SCENE; N == 0: zero results, GS_OK
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(_abi.GsConfig), 64, 64, 16, _abi.GS_FLAG_SPLAT_STATE
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    q = query()
    assert L.gs_neigh_count(ctx, ctypes.byref(q), ctypes.byref(info)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_neigh_read(ctx, None, 0, ctypes.byref(nn)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_state_neigh(ctx, 0, 1, 1, 0, 0, 1, 2, None) == _abi.GS_ERR_NO_SCENE
    _abi.check(L.gs_upload_splats(ctx, None, 0))
    info.queried = info.candidates = 9
    _abi.check(L.gs_neigh_count(ctx, ctypes.byref(q), ctypes.byref(info)))
    assert (info.queried, info.sources, info.candidates) == (0, 0, 0)
    _abi.check(L.gs_neigh_count(ctx, ctypes.byref(q), None))
    nn.value = 9
    _abi.check(L.gs_neigh_read(ctx, None, 0, ctypes.byref(nn)))
    assert nn.value == 0
    _abi.check(L.gs_state_neigh(ctx, 0, 1, 1, 0, 0, 1, 2, ctypes.byref(m)))
    assert m.value == 0
    L.gs_destroy(ctx)

    r = _mk(rec, 64, 64, 16)
    st = (np.arange(n) % 5).astype(np.uint8)
    r.write_state(st)
    neighbours.count(r, 0.5)
    plane = neighbours.read(r)
    assert plane.any()

    def refused(name, call, *fragments, code=INV):
        assert call() == code, name
        msg = L.gs_last_error().decode()
        assert name in msg and all(f in msg for f in fragments), msg
        assert np.array_equal(neighbours.read(r), plane)
        np.testing.assert_array_equal(r.read_state(), st)

    cnt = lambda q: (lambda: L.gs_neigh_count(r._ctx, ctypes.byref(q) if q is not None else None, ctypes.byref(info)))
    refused("gs_neigh_count", cnt(None), "null query")
    refused("gs_neigh_count", cnt(query(struct_size=36)), "struct_size 36")
    refused("gs_neigh_count", cnt(query(radius=float("nan"))), "radius nan")
    refused("gs_neigh_count", cnt(query(radius=float("inf"))), "radius inf")
    refused("gs_neigh_count", cnt(query(radius=-0.5)), "radius -0.5")
    refused("gs_neigh_count", cnt(query(radius=2e19)), "radius 2e+19", "squared")
    refused("gs_neigh_count", cnt(query(limit=0)), "limit 0")
    refused("gs_neigh_count", cnt(query(reserved=5)), "reserved 5")
    refused("gs_neigh_count", cnt(query(src_mask=0x100)), "0x100", "does not fit the state byte")
    refused("gs_neigh_count", cnt(query(src_value=0x1FF)), "0x1ff", "does not fit the state byte")
    refused("gs_neigh_count", cnt(query(qry_mask=0x100)), "0x100", "does not fit the state byte")
    refused("gs_neigh_count", cnt(query(qry_value=0x1FF)), "0x1ff", "does not fit the state byte")
    # the read's conventions are gs_coverage_read's
    refused("gs_neigh_read", lambda: L.gs_neigh_read(r._ctx, None, 0, None), "null n")
    buf = np.full(n, 0xA5A5A5A5, np.uint32)
    refused("gs_neigh_read", lambda: L.gs_neigh_read(r._ctx, buf.ctypes.data, n - 1, ctypes.byref(nn)), "%d counts needed" % n)
    assert nn.value == n and (buf == 0xA5A5A5A5).all()
    # gs_state_neigh's own: nothing is applied
    sel = lambda op, bits, wm=0: (lambda: L.gs_state_neigh(r._ctx, 0, 5, 1, wm, 0, op, bits, ctypes.byref(m)))
    m.value = 77
    refused("gs_state_neigh", sel(0, 2), "unknown op 0")
    refused("gs_state_neigh", sel(5, 2), "unknown op 5")
    refused("gs_state_neigh", sel(1, 0x100), "0x100")
    refused("gs_state_neigh", sel(1, 2, 0x100), "where_mask 0x100")
    assert m.value == 77
    r.destroy()
    # a context without the state plane: (0, 0) works, any other filter and gs_state_neigh are refused
    q = mk(rec, 64, 64, 16)
    neighbours.count(q, 0.5)
    assert np.array_equal(neighbours.read(q), want_counts("ragged", rec, 0.5))
    for fn in (lambda: neighbours.count(q, 0.5, source=(1, 0)), lambda: neighbours.count(q, 0.5, query=(1, 1)), lambda: neighbours.select(q, 0, 1)):
        code, msg = code_of(fn)
        assert code == INV and "GS_FLAG_SPLAT_STATE" in msg
    assert np.array_equal(neighbours.read(q), want_counts("ragged", rec, 0.5))
    q.destroy()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_node_host_neighbours_match_python(tmp_path):
    """neigh_check.js on the ragged golden scene: its counts, info and stateNeigh result are the Python host's."""
    from gsplat import _abi, neighbours
    s, u, W, H = state_scene("ragged")
    n = s.shape[0]
    rec = str(tmp_path / "rec.bin")
    np.ascontiguousarray(s, dtype=F).tofile(rec)
    out = run_node("neigh_check.js", (rec, n, W, H, 8))
    r = _mk(s, W, H, 8)
    info = neighbours.count(r, 0.5, 7)
    c = neighbours.read(r)
    assert np.array_equal(c, limited(want_counts("ragged", s, 0.5), 7))
    assert out["info"] == {"queried": info["queried"], "sources": info["sources"], "candidates": info["candidates"], "cells": list(info["cells"]),
                           "cellEdge": info["cell_edge"]}
    assert out["length"] == n and out["sum"] == int(c.sum()) and out["first"] == [int(x) for x in c[:16]]
    assert out["histogram"] == np.bincount(c, minlength=8).tolist()
    assert out["stateNeigh"] == neighbours.select(r, 0, 2) == int((c <= 2).sum()) > 0
    assert out["selected"] == r.state_count(_abi.GS_SPLAT_SELECTED, _abi.GS_SPLAT_SELECTED)
    r.state_region(_abi.GS_REGION_SPHERE, _abi.GS_STATE_SET, 0x04, a=(0, 0, 0), b=(1.5, 0, 0))
    neighbours.count(r, 0.5, 1, source=(4, 4), query=(4, 0))
    assert out["filteredSum"] == int(neighbours.read(r).sum()) > 0
    assert out["errors"] == {"radius": "-1", "limit": "-1", "budget": "-8"}
    r.destroy()
