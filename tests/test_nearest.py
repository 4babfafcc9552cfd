"""Nearest neighbours: the k-th nearest distance and the nearest id per splat (include/gsplat/gs_abi.h "nearest neighbours").

The reference every GPU answer is held to is tests/knn_restate.py: a numpy brute force over all pairs with the header's f32
expression.  The CPU tests pin the restatement by hand (a lattice whose neighbours sit exactly on the radius, a hand-checked pair,
exact duplicates) and the ABI.  The GPU tests compare both planes as uint32 views with np.array_equal -- there is no tolerance
anywhere -- over grids of many cells and of one, the blocked table, filters, special floats, the refinement, the radius-free search,
the selection by distance, the lifecycle of the planes, the frames around a search, the work budget and the refusals.
"""
import ctypes
import functools
import re

import numpy as np
import pytest

import knn_restate as kr
import state_restate as sr
from conftest import scene
from support import F, SLAB_COLS, c_layout, cached, code_of, frame_taps, host_sources, mk, state_ref, state_scene, timeless

_mk = functools.partial(mk, state=True)
NONE = kr.NONE
KS = (1, 2, 8, 32)
OPS = (sr.SET, sr.CLEAR, sr.TOGGLE, sr.ASSIGN)
INF = float("inf")


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


def special_pos():
    """1000 centres of the ragged scene with a NaN, +inf and -inf coordinate, -0.0, a denormal coordinate, two groups of exact
    duplicates and a pair of duplicates of non-finite splats (which are nobody's neighbours)."""
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


def want(key, pos, radius, src=None, qry=None, ks=KS):
    """The restatement for every k of ks, once per key and session; the key names the positions and the filters."""
    return cached(("knn", key, float(radius), tuple(ks)), lambda: kr.planes_multi(pos, ks, radius, src, qry))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, exp):
    """Both planes bit for bit; got = nearest.read(r), exp = (dist2, nearest, ...) of the restatement."""
    return np.array_equal(bits(got[0]), bits(exp[0])) and np.array_equal(got[1], exp[1])


def face_neighbour(i):
    """The smallest-index face neighbour of lattice point i = 36 a + 6 b + c."""
    a, b, c = i // 36, (i // 6) % 6, i % 6
    out = [36 * x + 6 * y + z for x, y, z in ((a - 1, b, c), (a + 1, b, c), (a, b - 1, c), (a, b + 1, c), (a, b, c - 1), (a, b, c + 1))
           if 0 <= x < 6 and 0 <= y < 6 and 0 <= z < 6]
    return min(out)


CORNERS = [36 * a + 6 * b + c for a in (0, 5) for b in (0, 5) for c in (0, 5)]


def check_lattice(plane_of):
    """The hand-made expectations on the lattice; plane_of(k, radius) -> (dist2, nearest, unresolved)."""
    d2, near, unresolved = plane_of(1, 0.25)
    assert d2.dtype == F and near.dtype == np.uint32
    assert (bits(d2) == bits(np.full(216, 0.0625, F))).all() and unresolved == 0
    assert near.tolist() == [face_neighbour(i) for i in range(216)]
    d2, _, unresolved = plane_of(3, 0.25)
    assert unresolved == 0 and (d2 == F(0.0625)).all()
    d2, _, unresolved = plane_of(4, 0.25)
    assert unresolved == 8 and np.flatnonzero(np.isinf(d2)).tolist() == CORNERS
    d2, near, unresolved = plane_of(7, 0.25)
    assert unresolved == 216 and np.isinf(d2).all() and near.tolist() == [face_neighbour(i) for i in range(216)]  # D_i is not empty
    d2, near, unresolved = plane_of(1, float(np.nextafter(F(0.25), F(0))))
    assert unresolved == 216 and (bits(d2) == kr.INF_BITS).all() and (near == NONE).all()


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_restatement_is_pinned():
    """The lattice at radius 0.25: k = 1 gives 0.0625 everywhere and the smallest-index face neighbour, k = 3 is resolved everywhere,
    k = 4 unresolved at exactly the 8 corners, k = 7 everywhere, and at the float below 0.25 everything is unresolved; the pair
    (1, 1, 1), (1.375, 1.5, 1) is 0.390625 apart squared, exactly; exact duplicates read +0.0 and the smaller index; the restatement
    equals a float64 per-point loop on the lattice; filters, self-exclusion by index, special floats, the REFINE rule, the range."""
    p = lattice_pos()
    check_lattice(lambda k, radius: kr.planes(p, k, radius))
    pair = np.array([[1, 1, 1], [1.375, 1.5, 1]], F)
    d2, near, unresolved = kr.planes(pair, 1, 0.625)
    assert bits(d2).tolist() == bits(np.array([0.390625, 0.390625], F)).tolist() and near.tolist() == [1, 0] and unresolved == 0
    d2, near, unresolved = kr.planes(pair, 1, float(np.nextafter(F(0.625), F(0))))
    assert np.isinf(d2).all() and (near == NONE).all() and unresolved == 2
    dup = np.array([[1, 2, 3], [5, 5, 5], [1, 2, 3], [1, 2, 3], [np.nan, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [np.inf, 0, 0]], F)
    d2, near, unresolved = kr.planes(dup, 1, 0.0)
    assert bits(d2).tolist() == [0, kr.INF_BITS, 0, 0] + [kr.INF_BITS] * 4  # +0.0, never -0.0
    assert near.tolist() == [2, NONE, 0, 0, NONE, NONE, NONE, NONE] and unresolved == 5
    d2, near, _ = kr.planes(dup, 2, 100.0)
    assert d2[:4].tolist() == [0.0, 29.0, 0.0, 0.0] and near[:4].tolist() == [2, 0, 0, 0] and np.isinf(d2[4:]).all()
    p64 = p.astype(np.float64)
    for radius in (0.25, 0.36, 0.5, 0.75):
        m = kr.planes_multi(p, (1, 5, 12), radius)
        for k in m:
            loop = []
            for i in range(len(p64)):
                d = sorted(v for j, v in enumerate(((p64 - p64[i]) ** 2).sum(axis=1)) if j != i and v <= radius * radius)
                loop.append(d[k - 1] if len(d) >= k else INF)
            assert m[k][0].astype(np.float64).tolist() == loop, (radius, k)
    # filters: a query that is no source is not self-excluded by accident; a splat that is no query reads the NaN with these bits
    src = np.arange(216) % 2 == 0
    d2, near, unresolved = kr.planes(p, 1, 0.25, src=src, qry=~src)
    assert (bits(d2)[src] == kr.NAN_BITS).all() and (near[src] == NONE).all() and (d2[~src] == F(0.0625)).all() and src[near[~src]].all()
    d2, near, _ = kr.planes(dup, 1, 0.0, src=[1, 0, 0, 0, 0, 0, 0, 0], qry=[0, 0, 1, 0, 0, 0, 0, 0])
    assert bits(d2).tolist() == [kr.NAN_BITS] * 2 + [0] + [kr.NAN_BITS] * 5 and near[2] == 0
    # the REFINE rule: only what reads +inf is queried and written, the rest keeps its value
    first = kr.planes(p, 4, 0.25)
    d2, near, queried, unresolved = kr.refine(first, p, 4, 0.36)
    assert queried == 8 and unresolved == 0 and (d2[CORNERS] == F(0.125)).all()
    others = np.setdiff1d(np.arange(216), CORNERS)
    assert np.array_equal(bits(d2)[others], bits(first[0])[others]) and same((d2, near), kr.planes(p, 4, 0.36))
    assert kr.member([0.0, 1.0, INF, np.nan], 1.0, INF).tolist() == [False, True, True, False]
    assert kr.member([0.0, 1.0, INF, np.nan], 2.0, 1.0, inside=False).all()
    assert kr.member([0.0, np.nan], -INF, INF, inside=False).tolist() == [False, True]


def test_knn_abi(tmp_path):
    """The three symbols are exported and listed; gs_knn and gs_knn_info are 48 bytes with the same offsets in the compiled header
    and in ctypes; the constants agree; GS_ABI_VERSION is still 3 and GS_ATTR_COUNT still 16; the header states the expression, the
    tie rule, the encodings and the radius-independence; a null context is refused by name; no Renderer methods, no Node exports."""
    import gsplat
    from gsplat import _abi, nearest
    L = _abi.load()
    names = ("gs_knn_search", "gs_knn_read", "gs_state_knn")
    for name in names:
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    q_fields = [n for n, _ in _abi.GsKnn._fields_]
    i_fields = [n for n, _ in _abi.GsKnnInfo._fields_]
    assert q_fields == ["struct_size", "radius", "k", "flags", "src_mask", "src_value", "qry_mask", "qry_value", "max_candidates", "reserved"]
    assert i_fields == ["queried", "sources", "candidates", "unresolved", "cells", "cell_edge"]
    prog = 'printf("%d %d %zu %zu", GS_ABI_VERSION, (int)GS_ATTR_COUNT, sizeof(gs_knn), sizeof(gs_knn_info));'
    prog += "".join('printf(" %%zu", offsetof(gs_knn, %s));' % n for n in q_fields)
    prog += "".join('printf(" %%zu", offsetof(gs_knn_info, %s));' % n for n in i_fields)
    prog += 'printf(" %u %u %u", GS_KNN_MAX_K, GS_KNN_REFINE, (unsigned)(GS_KNN_NONE == 0xFFFFFFFFu));'
    out = c_layout(tmp_path, "knn_layout", prog)
    assert out[0] == 3 and L.gs_abi_version() == 3 and out[1] == 16 == _abi.GS_ATTR_COUNT
    assert out[2] == 48 == ctypes.sizeof(_abi.GsKnn) and out[3] == 48 == ctypes.sizeof(_abi.GsKnnInfo)
    assert out[4:14] == [getattr(_abi.GsKnn, n).offset for n in q_fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    assert out[14:20] == [getattr(_abi.GsKnnInfo, n).offset for n in i_fields] == [0, 8, 16, 24, 32, 44]
    assert out[20:] == [32, 1, 1] and (_abi.GS_KNN_MAX_K, _abi.GS_KNN_REFINE, _abi.GS_KNN_NONE) == (32, 1, 0xFFFFFFFF)
    assert nearest.NONE == kr.NONE == _abi.GS_KNN_NONE and nearest.MAX_K == 32
    rjs, idx, dts, napi, hdr = host_sources()
    assert re.search(r"#define GS_ABI_VERSION 3\b", hdr)
    for name in names:
        assert re.search(r"int32_t %s\(gs_ctx\*" % name, hdr)
        assert name not in napi  # no Node exports: the N-API surface is pinned
    assert hdr.index("---- clusters") < hdr.index("---- nearest neighbours") < hdr.index("Tuning / profiling knobs")
    sec = hdr[hdr.index("---- nearest neighbours"):hdr.index("Tuning / profiling knobs")]
    for text in ("d2 = (dx dx + dy dy) + dz dz", "d = p_j - p_i", "r2 = radius * radius", "INCLUSIVE", "k-th smallest", "TIE RULE", "smallest index j",
                 "0x7F800000", "0x7FC00000", "GS_KNN_NONE (0xFFFFFFFF)", "UNRESOLVED", "DO NOT DEPEND\n * ON THE RADIUS", "27 cells", "GS_KNN_REFINE",
                 "f32[N]", "u32[N]", "DROPPED", "gs_upload_*", "gs_share_splats", "gs_compact", "searches again", "GS_ERR_CAPACITY", "as they were"):
        assert text in sec, text
    q, info, n = _abi.GsKnn(), _abi.GsKnnInfo(), ctypes.c_uint64()
    calls = {"gs_knn_search": lambda: L.gs_knn_search(None, ctypes.byref(q), ctypes.byref(info)),
             "gs_knn_read": lambda: L.gs_knn_read(None, None, None, 0, ctypes.byref(n)),
             "gs_state_knn": lambda: L.gs_state_knn(None, 0.0, 1.0, 1, 0, 0, 1, 2, None)}
    for name, call in calls.items():
        assert call() == _abi.GS_ERR_INVALID_ARGUMENT
        msg = L.gs_last_error()
        assert name.encode() in msg and b"null ctx" in msg
    assert gsplat.nearest is nearest
    for fn in ("search", "read", "select", "distances", "select_outliers"):
        assert callable(getattr(nearest, fn))
    for cls in (gsplat.Renderer, gsplat.PipelinedRenderer):
        assert not [m for m in dir(cls) if not m.startswith("_") and ("knn" in m.lower() or "nearest" in m.lower())]


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def _check_scene(key, rec, radii_cells, ks=KS):
    """search + read against the restatement for every radius and k; radii_cells: radius -> whether the grid must have more than
    one cell on every axis (True) or exactly one (False).  Returns {(k, radius): unresolved}."""
    from gsplat import nearest
    n = rec.shape[0]
    r = _mk(rec, 64, 64, 16)
    d2, near = nearest.read(r)  # before any search
    assert d2.shape == near.shape == (n,) and (bits(d2) == kr.NAN_BITS).all() and (near == NONE).all()
    out = {}
    for radius, many in radii_cells.items():
        w = want(key, rec, radius, ks=ks)
        for k in ks:
            info = nearest.search(r, k, radius)
            got = nearest.read(r)
            assert got[0].dtype == F and got[1].dtype == np.uint32
            assert same(got, w[k]), (key, radius, k, int((bits(got[0]) != bits(w[k][0])).sum()), int((got[1] != w[k][1]).sum()))
            assert info["unresolved"] == w[k][2], (key, radius, k, info)
            assert info["queried"] == info["sources"] == n
            cells = info["cells"]
            assert (min(cells) > 1) if many else (cells == (1, 1, 1)), (radius, cells)
            assert info["cell_edge"] >= 1.001 * radius
            out[(k, radius)] = w[k][2]
        print("%s radius %g: unresolved %s, cells %s, candidates %d" % (key, radius, [w[k][2] for k in ks], info["cells"], info["candidates"]))
    r.destroy()
    return out


@pytest.mark.gpu
def test_search_ragged_scene():
    """synth.bicycle_like(3001) at radii that give hundreds of cells per axis, tens, a few, and one (1e3: the all-pairs path and,
    with 64 queries sharing a cell, the uniform path): all unresolved, mixed and none."""
    from gsplat import synth
    rec = synth.bicycle_like(3001)
    u = _check_scene("ragged", rec, {0.1: True, 0.5: True, 2.0: True, 1e3: False})
    assert u[(32, 0.5)] == 3001 and u[(8, 0.5)] == 2111 and u[(1, 2.0)] == 420
    assert all(u[(k, 1e3)] == 0 for k in KS)


@pytest.mark.gpu
def test_search_length_no_multiple():
    """scene(10000)[:9997]: the length is no multiple of 4, 64 or 256."""
    rec = np.ascontiguousarray(scene(10000)[:9997])
    u = _check_scene("cfgA9997", rec, {0.25: True, 1.0: True}, ks=(1, 8, 32))
    assert 0 < u[(8, 0.25)] < 9997


@pytest.mark.gpu
def test_lattice():
    """The CPU case's expectations on the device: equality at r2, neighbours exactly one cell edge apart across cell borders, ties in
    d2 resolved to the smallest id; then the restatement at radii with more ties (0.36: face diagonals, 0.5)."""
    from gsplat import nearest
    p = lattice_pos()
    r = _mk(records(p), 64, 64, 16)

    def plane_of(k, radius):
        info = nearest.search(r, k, radius)
        d2, near = nearest.read(r)
        return d2, near, info["unresolved"]
    check_lattice(plane_of)
    for radius in (0.25, float(np.nextafter(F(0.25), F(0))), 0.36, 0.5):
        w = kr.planes_multi(p, (1, 4, 7, 19), radius)
        for k in w:
            info = nearest.search(r, k, radius)
            assert same(nearest.read(r), w[k]) and info["unresolved"] == w[k][2], (radius, k)
    r.destroy()
    pair = np.array([[1, 1, 1], [1.375, 1.5, 1]], F)
    r = _mk(records(pair), 64, 64, 16)
    nearest.search(r, 1, 0.625)
    d2, near = nearest.read(r)
    assert bits(d2).tolist() == bits(np.array([0.390625, 0.390625], F)).tolist() and near.tolist() == [1, 0]
    assert nearest.search(r, 1, float(np.nextafter(F(0.625), F(0))))["unresolved"] == 2
    r.destroy()


@pytest.mark.gpu
def test_blocked_table():
    """More than 2^24 cells: the cell table is indexed by blocks of consecutive keys and a cell's run is found by binary search
    inside its block.  test_neighbours.test_blocked_table's constructions: the lattice with a 200-splat knot (whole waves whose
    queries share a cell) and two far ends, and the ragged scene shrunk to a fifth between two far splats, with and without filters."""
    from gsplat import nearest, synth
    ends = np.array([[-120, -121, -122], [123, 122, 121]], F)
    knot = (F(5.0) + np.random.default_rng(11).uniform(-0.005, 0.005, (200, 3))).astype(F)
    p = np.concatenate([lattice_pos(), knot, ends])
    true = kr.planes_multi(p, (1, 8, 32), 1e3)
    r = _mk(records(p), 64, 64, 16)
    for radius in (0.25, 0.36):
        w = kr.planes_multi(p, (1, 8, 32), radius)
        for k in w:
            info = nearest.search(r, k, radius)
            assert min(info["cells"]) > 256 and info["cells"][0] * info["cells"][1] * info["cells"][2] > 2**24, info
            got = nearest.read(r)
            assert same(got, w[k]) and info["unresolved"] == w[k][2], (radius, k)
            # in the knot every k is resolved, at its true value
            assert np.isfinite(got[0][216:416]).all() and np.array_equal(bits(got[0])[216:416], bits(true[k][0])[216:416])
    r.destroy()
    p = np.concatenate([synth.bicycle_like(3001)[:, 0:3] * F(0.2), ends / F(4)]).astype(F)
    n = p.shape[0]
    st = (np.arange(n) % 5).astype(np.uint8)
    r = _mk(records(p), 64, 64, 16)
    r.write_state(st)
    for radius in (0.06, 0.1):
        w, wf = kr.planes_multi(p, (1, 8, 32), radius), kr.planes_multi(p, (1, 8, 32), radius, st == 1, st == 2)
        for k in w:
            info = nearest.search(r, k, radius)
            assert min(info["cells"]) > 256 and info["cells"][0] * info["cells"][1] * info["cells"][2] > 2**24, info
            assert same(nearest.read(r), w[k]) and info["unresolved"] == w[k][2], (radius, k)
            info = nearest.search(r, k, radius, source=(7, 1), query=(7, 2))
            assert same(nearest.read(r), wf[k]) and info["unresolved"] == wf[k][2], (radius, k)
        assert 0 < w[1][2] < n
    r.destroy()


@pytest.mark.gpu
def test_filters():
    """Source and query differ, overlap, are empty and are equal; non-queries read 0x7FC00000 / NONE; (0, 0) on a ctx without the
    state plane."""
    from gsplat import nearest, synth
    rec = synth.bicycle_like(3001)
    n = rec.shape[0]
    st = (np.arange(n) % 5).astype(np.uint8)
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    even, low = (st & 1) == 0, st < 3
    cases = {"differ": ((7, 1), (7, 2), st == 1, st == 2), "equal": ((1, 0), (1, 0), even, even), "overlap": ((1, 0), (4, 0), even, st < 4),
             "all_sources": ((0, 0), (7, 3), None, st == 3)}
    for radius in (0.5, 2.0):
        for name, (source, query, sm, qm) in cases.items():
            w = kr.planes_multi(rec, (1, 8), radius, sm, qm)
            for k in w:
                info = nearest.search(r, k, radius, source=source, query=query)
                got = nearest.read(r)
                assert same(got, w[k]) and info["unresolved"] == w[k][2], (name, radius, k)
                assert (bits(got[0])[~qm] == kr.NAN_BITS).all() and (got[1][~qm] == NONE).all()
                assert (info["sources"], info["queried"]) == (n if sm is None else int(sm.sum()), int(qm.sum()))
    assert low.any()
    # no source at all: every query unresolved; no query at all: everything NaN
    info = nearest.search(r, 1, 0.5, source=(0xFF, 0xEE))
    d2, near = nearest.read(r)
    assert info["sources"] == 0 and info["queried"] == info["unresolved"] == n and (bits(d2) == kr.INF_BITS).all() and (near == NONE).all()
    info = nearest.search(r, 1, 0.5, query=(0xFF, 0xEE))
    d2, near = nearest.read(r)
    assert info["queried"] == info["unresolved"] == 0 and (bits(d2) == kr.NAN_BITS).all() and (near == NONE).all()
    np.testing.assert_array_equal(r.read_state(), st)
    r.destroy()
    # a query that is no source is not self-excluded by accident: a duplicate pair, one a source, one a query
    p = np.array(rec[:100, 0:3], copy=True)
    p[1] = p[0]
    r = _mk(records(p), 64, 64, 16)
    st = np.zeros(100, np.uint8)
    st[0], st[1] = 1, 2
    r.write_state(st)
    assert nearest.search(r, 1, 0.0, source=(3, 1), query=(3, 2))["unresolved"] == 0
    d2, near = nearest.read(r)
    assert bits(d2)[1] == 0 and near[1] == 0 and (bits(d2)[np.arange(100) != 1] == kr.NAN_BITS).all()
    r.destroy()
    q = mk(rec, 64, 64, 16)  # without GS_FLAG_SPLAT_STATE
    nearest.search(q, 8, 0.5)
    assert same(nearest.read(q), want("ragged", rec, 0.5)[8])
    for fn in (lambda: nearest.search(q, 8, 0.5, source=(1, 0)), lambda: nearest.search(q, 8, 0.5, query=(1, 1)), lambda: nearest.select(q, 0, 1)):
        code, msg = code_of(fn)
        assert code == -1 and "GS_FLAG_SPLAT_STATE" in msg
    assert same(nearest.read(q), want("ragged", rec, 0.5)[8])
    q.destroy()


@pytest.mark.gpu
def test_special_floats():
    from gsplat import nearest
    p = special_pos()
    n = p.shape[0]
    far = np.concatenate([p, np.array([[1e6, 1e6, -1e6]], F)])  # a far outlier coarsens (or is clamped by) the grid
    r, rf = _mk(records(p), 64, 64, 16), _mk(records(far), 64, 64, 16)
    for radius in (0.5, 0.1, 0.0, 1e-40, 100.0):
        w = kr.planes_multi(p, (1, 2), radius)
        for k in w:
            info = nearest.search(r, k, radius)
            got = nearest.read(r)
            assert same(got, w[k]) and info["unresolved"] == w[k][2], (radius, k)
            nearest.search(rf, k, radius)
            gf = nearest.read(rf)
            assert np.array_equal(bits(gf[0])[:n], bits(got[0])) and np.array_equal(gf[1][:n], got[1]), (radius, k)
            assert bits(gf[0])[n] == kr.INF_BITS and gf[1][n] == NONE
            for i in (10, 20, 30, 70, 71):  # non-finite: no neighbours, nobody's neighbour, counted as unresolved
                assert bits(got[0])[i] == kr.INF_BITS and got[1][i] == NONE
            assert not np.isin(got[1], (10, 20, 30, 70, 71)).any()
    nearest.search(r, 1, 0.0)
    d2, near = nearest.read(r)
    assert bits(d2)[[60, 61, 80, 81, 82]].tolist() == [0] * 5 and near[[60, 61, 80, 81, 82]].tolist() == [61, 60, 81, 80, 80]
    assert int(np.isfinite(d2).sum()) == 5  # radius 0: only the duplicates
    nearest.search(r, 2, 0.0)
    d2, near = nearest.read(r)
    assert bits(d2)[[80, 81, 82]].tolist() == [0] * 3 and np.isinf(d2[[60, 61]]).all() and near[[60, 61]].tolist() == [61, 60]
    r.destroy()
    rf.destroy()


@pytest.mark.gpu
def test_refine():
    """A search at 0.5, a refine at 2.0, a refine at 1e3: after each step the planes equal the restated REFINE rule and every entry
    resolved earlier is bit-identical to before; the final planes equal a single search at 1e3; a refine with another k, or before
    any search, is refused and changes nothing."""
    from gsplat import nearest, synth
    rec = synth.bicycle_like(3001)
    n = rec.shape[0]
    for k in (1, 8):
        r = _mk(rec, 64, 64, 16)
        code, msg = code_of(lambda: nearest.search(r, k, 0.5, refine=True))
        assert code == -1 and "gs_knn_search" in msg and "GS_KNN_REFINE" in msg and "before any search" in msg
        d2, near = nearest.read(r)
        assert (bits(d2) == kr.NAN_BITS).all() and (near == NONE).all()
        info = nearest.search(r, k, 0.5)
        prev = want("ragged", rec, 0.5)[k]
        assert same(nearest.read(r), prev) and info["unresolved"] == prev[2] > 0
        code, msg = code_of(lambda: nearest.search(r, k + 1, 2.0, refine=True))
        assert code == -1 and "k %d" % (k + 1) in msg and "k %d" % k in msg
        assert same(nearest.read(r), prev)
        unresolved = prev[2]
        for radius in (2.0, 1e3):
            exp = kr.refine(prev, rec, k, radius)
            info = nearest.search(r, k, radius, refine=True)
            got = nearest.read(r)
            assert same(got, exp), (k, radius)
            assert info["queried"] == unresolved == exp[2] and info["unresolved"] == exp[3] and info["sources"] == n
            done = bits(prev[0]) != kr.INF_BITS
            assert np.array_equal(bits(got[0])[done], bits(prev[0])[done]) and np.array_equal(got[1][done], prev[1][done])
            prev, unresolved = exp, exp[3]
        assert unresolved == 0 and same(nearest.read(r), want("ragged", rec, 1e3)[k])
        # a refine with nothing left to do queries nothing and writes nothing
        info = nearest.search(r, k, 5.0, refine=True)
        assert info["queried"] == info["unresolved"] == 0 and same(nearest.read(r), want("ragged", rec, 1e3)[k])
        r.destroy()
    # a filter: the gate restricts the queries of the filter, non-queries keep their NaN
    st = (np.arange(n) % 3).astype(np.uint8)
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    nearest.search(r, 2, 0.5, source=(3, 0), query=(3, 1))
    prev = kr.planes(rec, 2, 0.5, st == 0, st == 1)
    assert same(nearest.read(r), prev)
    exp = kr.refine(prev, rec, 2, 3.0, st == 0, st == 1)
    info = nearest.search(r, 2, 3.0, source=(3, 0), query=(3, 1), refine=True)
    assert same(nearest.read(r), exp) and (info["queried"], info["unresolved"]) == (prev[2], exp[3]) and 0 < prev[2]
    r.destroy()


@pytest.mark.gpu
def test_distances(monkeypatch):
    """From three different starting radii the final planes are identical and equal the restatement at a radius beyond the scene; a
    start whose first round exceeds a small max_candidates is halved and retried; a scene with fewer than k + 1 finite members
    leaves exactly those queries +inf."""
    from gsplat import _abi, nearest, synth
    rec = synth.bicycle_like(3001)
    n = rec.shape[0]
    w = want("ragged", rec, 1e3)[8]
    r = _mk(rec, 64, 64, 16)
    for start in (1e-3, None, 50.0):
        out = nearest.distances(r, 8, radius=start)
        assert same(nearest.read(r), w), start
        assert out["unresolved"] == 0 and out["rounds"] >= 1 and out["radius"] > 0 and out["candidates"] > 0
        print("distances from %s: %s" % (start, out))
    calls = []
    search = nearest.search

    def spy(r_, k, radius, **kw):
        try:
            info = search(r_, k, radius, **kw)
        except _abi.GsError as e:
            calls.append((radius, kw.get("refine", False), e.code))
            raise
        calls.append((radius, kw.get("refine", False), 0))
        return info
    monkeypatch.setattr(nearest, "search", spy)
    out = nearest.distances(r, 8, radius=50.0, max_candidates=n * n // 4)
    assert same(nearest.read(r), w) and out["unresolved"] == 0
    refused = [c for c in calls if c[2] == _abi.GS_ERR_CAPACITY]
    assert refused and calls[0] == (50.0, False, _abi.GS_ERR_CAPACITY) and calls[1][0] == 25.0 and not any(c[1] for c in refused)
    assert [c[2] for c in calls[len(refused):]] == [0] * (len(calls) - len(refused)) and out["rounds"] == len(calls) - len(refused)
    monkeypatch.undo()
    r.destroy()
    # 6 members, one of them with a NaN coordinate: k = 8 leaves all six +inf, k = 2 only the NaN one
    p = np.array(rec[:6, 0:3], copy=True)
    p[3, 1] = np.nan
    r = _mk(records(p), 64, 64, 16)
    out = nearest.distances(r, 8)
    d2, near = nearest.read(r)
    assert out["unresolved"] == 6 and (bits(d2) == kr.INF_BITS).all() and near[3] == NONE and (near[[0, 1, 2, 4, 5]] != NONE).all()
    out = nearest.distances(r, 2, radius=0.01)
    assert out["unresolved"] == 1 and same(nearest.read(r), kr.planes(p, 2, 1e3)) and np.flatnonzero(np.isinf(nearest.read(r)[0])).tolist() == [3]
    r.destroy()


@pytest.mark.gpu
def test_state_knn():
    """matched and the state plane against the restated membership for every op, inside 0 and 1, a where filter, hi = +inf (the
    unresolved are in), the NaN splats never in range, and the empty range."""
    from gsplat import nearest, synth
    rec = synth.bicycle_like(3001)
    n = rec.shape[0]
    qm = np.arange(n) % 4 != 0
    st0 = np.where(qm, 0, 0x40).astype(np.uint8)
    d2 = kr.planes(rec, 8, 2.0, None, qm)[0]
    assert np.isnan(d2).sum() == n - qm.sum() and np.isinf(d2).any() and np.isfinite(d2).any()
    st = (np.random.default_rng(7).integers(0, 256, n) & 0xBF).astype(np.uint8) | st0
    r = _mk(rec, 64, 64, 16)
    r.write_state(st0)
    nearest.search(r, 8, 2.0, query=(0x40, 0))
    assert np.array_equal(bits(nearest.read(r)[0]), bits(d2))
    med = float(np.median(d2[np.isfinite(d2)]))
    ranges = [(0.0, med), (med, INF), (0.0, INF), (-INF, INF), (INF, INF), (med, 0.0), (float(np.nextafter(F(med), F(INF))), 3.0e38)]
    for k, (lo, hi) in enumerate(ranges):
        for inside in (True, False):
            for op in OPS:
                b = (0x02, 0xA4)[(k + op) % 2]
                where = ((0, 0), (0x0C, 0x04), (0x30, 0x10))[(k + op + int(inside)) % 3]
                r.write_state(st)
                member = kr.member(d2, lo, hi, inside)
                new, matched = sr.apply_region(st, member, op, b, where)
                cell = (lo, hi, inside, op, b, where)
                assert nearest.select(r, lo, hi, inside, where, op, b) == matched, cell
                np.testing.assert_array_equal(r.read_state(), new, err_msg=str(cell))
                if inside:
                    assert not member[~qm].any()  # a NaN is in no range
                if lo > hi:
                    assert member.sum() == (0 if inside else n)
                if hi == INF and lo <= med and inside:
                    assert member[np.isinf(d2)].all()
    assert np.array_equal(bits(nearest.read(r)[0]), bits(d2))  # the selection only reads the plane
    r.destroy()


@pytest.mark.gpu
def test_select_outliers_then_hide_frame(oracle):
    """select_outliers against the same arithmetic on the restated plane; after hide_selected the next EXACT frame equals the
    oracle's frame of the scene with those splats hidden, in every tap."""
    from gpu_checks import check_stages
    from gsplat import _abi, nearest
    s, u, W, H = state_scene("ragged")
    n = s.shape[0]
    d2 = want("ragged", s, 1e3)[8][0]
    out = d2 >= kr.outlier_threshold(d2, 1.0)
    assert 0 < out.sum() < n // 4
    state = np.where(out, sr.HIDDEN | sr.SELECTED, 0).astype(np.uint8)
    ref = state_ref(oracle, "ragged", 8, "knn_outliers_k8_s1", state)
    r = _mk(s, W, H, 8, exact=True)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    assert nearest.select_outliers(r, 8, 1.0) == int(out.sum())
    assert same(nearest.read(r), want("ragged", s, 1e3)[8])
    assert r.hide_selected() == int(out.sum())
    np.testing.assert_array_equal(r.read_state(), state)
    r.render_uniforms(u, debug=True)
    r.wait()
    check_stages(r, ref, True, debug=True)
    # among a filter's members: the others are neither sources nor selected; the unresolved are outliers
    keep = np.arange(n) % 3 != 0
    st = np.where(keep, 0, 8).astype(np.uint8)
    r.write_state(st)
    dk = kr.planes(s, 4, 1e3, keep, keep)[0]
    outk = keep & (dk >= kr.outlier_threshold(dk, 2.0))
    assert nearest.select_outliers(r, 4, 2.0, where=(8, 0)) == int(outk.sum()) > 0
    np.testing.assert_array_equal(r.read_state(), np.where(outk, st | sr.SELECTED, st).astype(np.uint8))
    r.destroy()


@pytest.mark.gpu
def test_lifecycle():
    """The planes read NaN / NONE before the first search and after an upload, compact and share_splats; state calls and transforms
    leave them; a borrower and a slab ctx answer the same as a fresh ctx; the count plane and the cluster planes are unchanged by a
    search, and the search's planes by a count and a labelling."""
    from gsplat import _abi, clusters, nearest, neighbours, synth
    rec = synth.bicycle_like(3001)
    n = rec.shape[0]
    w = want("ragged", rec, 0.5)[8]

    def blank(r, m):
        d2, near = nearest.read(r)
        return d2.shape == near.shape == (m,) and bool((bits(d2) == kr.NAN_BITS).all()) and bool((near == NONE).all())
    owner = _mk(rec, 64, 64, 16)
    assert blank(owner, n)
    slab = _mk(rec, 256, 256, 16, cols=SLAB_COLS[16])
    assert nearest.search(slab, 8, 0.5)["unresolved"] == w[2] and same(nearest.read(slab), w)
    slab.destroy()
    borrower = _mk(rec, 64, 64, 16, share_with=owner)
    assert blank(borrower, n)
    assert nearest.search(borrower, 8, 0.5)["unresolved"] == w[2] and same(nearest.read(borrower), w)
    assert blank(owner, n)  # the borrower keeps its own planes
    nearest.search(owner, 8, 0.5)
    _abi.check(borrower._L.gs_share_splats(borrower._ctx, owner._ctx))  # sharing again drops the borrower's planes ...
    assert blank(borrower, n) and same(nearest.read(owner), w)          # ... and not the owner's
    code, _ = code_of(lambda: nearest.search(borrower, 8, 2.0, refine=True))  # ... and the k to refine with them
    assert code == -1
    borrower.destroy()
    # the count plane and the cluster planes are unchanged by a search, and vice versa
    neighbours.count(owner, 0.5)
    clusters.label(owner, 0.5)
    cnt, (lab, siz) = neighbours.read(owner), clusters.read(owner)
    assert cnt.any() and same(nearest.read(owner), w)
    nearest.search(owner, 1, 2.0)
    assert np.array_equal(neighbours.read(owner), cnt) and np.array_equal(clusters.read(owner)[0], lab) and np.array_equal(clusters.read(owner)[1], siz)
    nearest.search(owner, 8, 0.5)
    # state calls and transforms leave the planes; a new search sees the moved splats
    assert owner.select_sphere((0, 0, 0), 1.5) > 100
    owner.translate_selected((0.3, -0.2, 0.1))
    assert same(nearest.read(owner), w)
    moved = owner.export_splats()
    assert not np.array_equal(moved[:, 0:3], rec[:, 0:3])
    nearest.search(owner, 8, 0.5)
    assert same(nearest.read(owner), kr.planes(moved, 8, 0.5))
    # compact and a re-upload drop the planes
    st = (np.arange(n) % 3 == 0).astype(np.uint8) * 4
    owner.write_state(st)
    kept = owner.compact(4, 4)
    assert kept.size == int((st == 4).sum()) and blank(owner, kept.size)
    code, _ = code_of(lambda: nearest.search(owner, 8, 2.0, refine=True))
    assert code == -1 and blank(owner, kept.size)
    nearest.search(owner, 8, 0.5)
    assert same(nearest.read(owner), kr.planes(moved[kept], 8, 0.5))
    arr = np.ascontiguousarray(rec[:2000])
    _abi.check(owner._L.gs_upload_splats(owner._ctx, arr.ctypes.data, 2000))
    assert blank(owner, 2000)
    owner.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_search_disturbs_no_frame(graph):
    """A frame rendered before and after a search (and a selection by it that changes nothing), direct and graph-replayed, is
    byte-identical in every tap and in gs_pick, and its statistics are unchanged."""
    from gsplat import _abi, nearest
    s, u, W, H = state_scene("ragged")
    a, b = _mk(s, W, H, 8), _mk(s, W, H, 8)
    for r in (a, b):
        r.set_option(_abi.GS_OPT_FRAME_GRAPH, graph)
    w = want("ragged", s, 0.5)[8]
    xy = np.array([(x, y) for y in range(1, H, 11) for x in range(2, W, 13)], np.uint32)
    for rep in range(2):
        before = frame_taps(a, u, False)
        pick_before = a.pick(xy)
        frame_taps(b, u, False)
        for _ in range(3):  # three frames in flight on both; no wait: the search drains the ring
            a.render_uniforms(u)
            b.render_uniforms(u)
        nearest.search(a, 8, 0.5)
        assert same(nearest.read(a), w)
        assert nearest.select(a, 5.0, 1.0, op=sr.SET, bits=sr.HIDDEN) == 0  # the empty range
        ta, tb = frame_taps(a, u, False), frame_taps(b, u, False)
        for k in ta:
            np.testing.assert_array_equal(ta[k], tb[k], err_msg=k)
            np.testing.assert_array_equal(ta[k], before[k], err_msg=k)
        pa, pb = a.pick(xy), b.pick(xy)
        assert pa.tobytes() == pb.tobytes() == pick_before.tobytes()
        assert timeless(a.stats()) == timeless(b.stats())
    if graph:
        assert a.stats()["graph_frames"] == b.stats()["graph_frames"] > 0
    a.destroy()
    b.destroy()


@pytest.mark.gpu
def test_budget_and_refusals():
    """max_candidates below info["candidates"] gives GS_ERR_CAPACITY with both numbers in the message, the planes as they were and
    info still written; every refusal leaves the planes as they were and the ctx rendering."""
    from gsplat import _abi, nearest, synth
    L = _abi.load()
    INV = _abi.GS_ERR_INVALID_ARGUMENT
    rec = synth.bicycle_like(3001)
    n = rec.shape[0]
    info, nn, m = _abi.GsKnnInfo(), ctypes.c_uint64(), ctypes.c_uint64(77)

    def query(**kw):
        q = _abi.GsKnn()
        q.struct_size, q.radius, q.k = ctypes.sizeof(_abi.GsKnn), 0.5, 3
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    # before any upload: GS_ERR_NO_SCENE; N == 0: zero results, GS_OK
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(_abi.GsConfig), 64, 64, 16, _abi.GS_FLAG_SPLAT_STATE
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    q = query()
    assert L.gs_knn_search(ctx, ctypes.byref(q), ctypes.byref(info)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_knn_read(ctx, None, None, 0, ctypes.byref(nn)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_state_knn(ctx, 0.0, 1.0, 1, 0, 0, 1, 2, None) == _abi.GS_ERR_NO_SCENE
    _abi.check(L.gs_upload_splats(ctx, None, 0))
    info.queried = info.candidates = info.unresolved = 9
    _abi.check(L.gs_knn_search(ctx, ctypes.byref(q), ctypes.byref(info)))
    assert (info.queried, info.sources, info.candidates, info.unresolved) == (0, 0, 0, 0)
    _abi.check(L.gs_knn_search(ctx, ctypes.byref(q), None))
    nn.value = 9
    _abi.check(L.gs_knn_read(ctx, None, None, 0, ctypes.byref(nn)))
    assert nn.value == 0
    _abi.check(L.gs_state_knn(ctx, 0.0, 1.0, 1, 0, 0, 1, 2, ctypes.byref(m)))
    assert m.value == 0
    L.gs_destroy(ctx)

    s, u, W, H = state_scene("ragged")
    r = _mk(rec, W, H, 8)
    st = (np.arange(n) % 5).astype(np.uint8)
    r.write_state(st)
    frame = frame_taps(r, u, False)
    done = nearest.search(r, 8, 0.5)
    plane = nearest.read(r)
    assert same(plane, want("ragged", rec, 0.5)[8])

    # the budget: both numbers in the message, the planes as they were, info written
    code, msg = code_of(lambda: nearest.search(r, 8, 0.5, max_candidates=done["candidates"] - 1))
    assert code == _abi.GS_ERR_CAPACITY and "gs_knn_search" in msg and str(done["candidates"]) in msg and str(done["candidates"] - 1) in msg
    assert same(nearest.read(r), plane)
    q = query(k=8, max_candidates=1)
    info.candidates = info.sources = 0
    assert L.gs_knn_search(r._ctx, ctypes.byref(q), ctypes.byref(info)) == _abi.GS_ERR_CAPACITY
    assert (info.candidates, info.sources, info.queried) == (done["candidates"], n, n) and tuple(info.cells) == done["cells"]
    assert "max_candidates = 1 " in L.gs_last_error().decode() + " " and same(nearest.read(r), plane)
    q = query(k=8, flags=_abi.GS_KNN_REFINE, radius=2.0, max_candidates=1)
    assert L.gs_knn_search(r._ctx, ctypes.byref(q), ctypes.byref(info)) == _abi.GS_ERR_CAPACITY and same(nearest.read(r), plane)
    assert info.queried == done["unresolved"]
    assert nearest.search(r, 8, 0.5, max_candidates=done["candidates"])["candidates"] == done["candidates"]

    def refused(name, call, *fragments, code=INV):
        assert call() == code, name
        msg = L.gs_last_error().decode()
        assert name in msg and all(f in msg for f in fragments), msg
        assert same(nearest.read(r), plane)
        np.testing.assert_array_equal(r.read_state(), st)

    srch = lambda q: (lambda: L.gs_knn_search(r._ctx, ctypes.byref(q) if q is not None else None, ctypes.byref(info)))
    refused("gs_knn_search", srch(None), "null query")
    refused("gs_knn_search", srch(query(struct_size=40)), "struct_size 40")
    refused("gs_knn_search", srch(query(radius=float("nan"))), "radius nan")
    refused("gs_knn_search", srch(query(radius=float("inf"))), "radius inf")
    refused("gs_knn_search", srch(query(radius=-0.5)), "radius -0.5")
    refused("gs_knn_search", srch(query(radius=2e19)), "radius 2e+19", "squared")
    refused("gs_knn_search", srch(query(k=0)), "k 0")
    refused("gs_knn_search", srch(query(k=33)), "k 33")
    refused("gs_knn_search", srch(query(flags=6)), "flags 0x6")
    refused("gs_knn_search", srch(query(flags=3)), "flags 0x2")
    refused("gs_knn_search", srch(query(reserved=5)), "reserved 5")
    refused("gs_knn_search", srch(query(flags=_abi.GS_KNN_REFINE, k=3)), "GS_KNN_REFINE", "k 3", "k 8")
    refused("gs_knn_search", srch(query(src_mask=0x100)), "0x100", "does not fit the state byte")
    refused("gs_knn_search", srch(query(src_value=0x1FF)), "0x1ff", "does not fit the state byte")
    refused("gs_knn_search", srch(query(qry_mask=0x100)), "0x100", "does not fit the state byte")
    refused("gs_knn_search", srch(query(qry_value=0x1FF)), "0x1ff", "does not fit the state byte")
    # the read's conventions are gs_cluster_read's
    refused("gs_knn_read", lambda: L.gs_knn_read(r._ctx, None, None, 0, None), "null n")
    bd, bn = np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, 0xA5A5A5A5, np.uint32)
    refused("gs_knn_read", lambda: L.gs_knn_read(r._ctx, bd.ctypes.data, bn.ctypes.data, n - 1, ctypes.byref(nn)), "%d values per plane needed" % n)
    assert nn.value == n and (bd == 0xA5A5A5A5).all() and (bn == 0xA5A5A5A5).all()
    _abi.check(L.gs_knn_read(r._ctx, bd.ctypes.data, None, n, ctypes.byref(nn)))  # either pointer may be null
    assert np.array_equal(bd, bits(plane[0])) and (bn == 0xA5A5A5A5).all()
    _abi.check(L.gs_knn_read(r._ctx, None, bn.ctypes.data, n, ctypes.byref(nn)))
    assert np.array_equal(bn, plane[1])
    # gs_state_knn's own: nothing is applied
    sel = lambda op, b, wm=0, lo=0.0, hi=5.0: (lambda: L.gs_state_knn(r._ctx, lo, hi, 1, wm, 0, op, b, ctypes.byref(m)))
    m.value = 77
    refused("gs_state_knn", sel(0, 2), "unknown op 0")
    refused("gs_state_knn", sel(5, 2), "unknown op 5")
    refused("gs_state_knn", sel(1, 0x100), "0x100")
    refused("gs_state_knn", sel(1, 2, 0x100), "where_mask 0x100")
    refused("gs_state_knn", sel(1, 2, lo=float("nan")), "not a number")
    refused("gs_state_knn", sel(1, 2, hi=float("nan")), "not a number")
    assert m.value == 77
    after = frame_taps(r, u, False)  # ... and the ctx rendering
    for k in after:
        np.testing.assert_array_equal(after[k], frame[k], err_msg=k)
    r.destroy()
