"""The wave shapes the cell grid's walk decides on, for every call that walks it: the neighbour count, the nearest-neighbour search
(k = 1 and 8), the surface estimate (kept sums) and the cluster labelling.

A query kernel gives a wave 64 consecutive cell-sorted queries and asks three things of it: does any lane hold a query, do all its
queries share a cell (one uniform walk out of scalar registers) or does each lane walk its own spans, and which lanes take part.
The scenes here are the smallest that reach every answer -- a lone lane, a wave short by one, a full wave, waves wholly without a
query behind a single lane, a second workgroup, waves that share a cell next to waves that straddle cells, queries that are no
sources, a query without a record -- once with every splat in the one cell around the origin (where a dead lane's cell is the
dense one) and once scattered over many cells.  Every plane is compared bit for bit with the numpy restatements (neigh_restate,
knn_restate, surface_restate, cluster_restate): there is no tolerance anywhere.
"""
import functools

import numpy as np
import pytest

import cluster_restate as cr
import knn_restate as kr
import neigh_restate as nr
import surface_restate as sfr
from conftest import scene
from support import F, cached, mk

_mk = functools.partial(mk, state=True)
COUNTS = (1, 63, 64, 65, 193, 257)  # a lone lane; a wave short by one; a full wave; a wave, one lane and two empty waves; three waves and one lane; a second workgroup of one lane
KS = (1, 8)
RADIUS = 1.0
SRC, QRY = (7, 1), (7, 2)  # the filters of the scenes whose queries are no sources: state 1 and state 2


def records(pos):
    """Records of the synthetic scene with their centres replaced by `pos`."""
    pos = np.asarray(pos, F)
    rec = np.array(scene(10000)[:pos.shape[0]], dtype=F, copy=True)
    rec[:, 0:3] = pos
    return np.ascontiguousarray(rec)


def one_cell(n, seed=1):
    """n centres within 0.45 of the origin on every axis: at RADIUS the box is narrower than a cell, and a pair can be up to 1.56 apart."""
    return np.random.default_rng(seed).uniform(-0.45, 0.45, (n, 3)).astype(F)


def scattered(n, seed=2):
    """n centres in a box of four cells a side."""
    return np.random.default_rng(seed).uniform(-2.0, 2.0, (n, 3)).astype(F)


def mixed_waves():
    """256 centres whose cell order is: 64 in the first cell of the first row, 64 in the cell beside it, 128 over the rest of an 8^3 box.
    The first point pins the box's corner at the origin."""
    rng = np.random.default_rng(3)
    a = rng.uniform(0.1, 0.9, (64, 3))
    a[0] = 0.0
    b = rng.uniform(0.1, 0.9, (64, 3)) + (1.1, 0.0, 0.0)
    rest = rng.uniform(0.1, 7.9, (128, 3))
    rest[:, 0] = rng.uniform(2.3, 7.9, 128)
    p = np.concatenate([a, b, rest]).astype(F)
    return p[rng.permutation(256)]  # the splat order is not the cell order


def apart(nan_query=False):
    """(centres, state): 300 sources (state 1), 200 of them in one cell, and 65 queries (state 2) in that cell; with nan_query one
    query has a NaN coordinate."""
    rng = np.random.default_rng(4)
    dense = rng.uniform(0.1, 0.9, (200, 3))
    dense[0] = 0.0
    far = rng.uniform(0.1, 4.9, (100, 3))
    far[:, 2] = rng.uniform(1.2, 4.9, 100)
    qry = rng.uniform(0.1, 0.9, (65, 3))
    if nan_query:
        qry[7, 1] = np.nan
    p = np.concatenate([dense, far, qry]).astype(F)
    st = np.concatenate([np.full(300, 1, np.uint8), np.full(65, 2, np.uint8)])
    order = rng.permutation(365)
    return p[order], st[order]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def want(key, pos, src=None, qry=None):
    """The four restatements of a scene, once per session.  The labelling's members are the queries."""
    def make():
        return {"count": nr.counts(pos, RADIUS, src, qry), "count2": nr.counts(pos, RADIUS, src, qry, limit=2),
                "knn": kr.planes_multi(pos, KS, RADIUS, src, qry), "surface": sfr.sums(pos, RADIUS, src, qry),
                "cluster": cr.components(pos, RADIUS, qry)}
    return cached(("grid_walks", key), make)


def check_all(r, key, pos, src=None, qry=None, source=(0, 0), query=(0, 0), cells=None):
    """count, search (k = 1, 8), estimate (kept sums) and label on `r` against the restatements, bit for bit; returns the count's info."""
    from gsplat import clusters, nearest, neighbours, surface
    w = want(key, pos, src, qry)
    n = pos.shape[0]
    nq = n if qry is None else int(qry.sum())
    info = neighbours.count(r, RADIUS, source=source, query=query)
    assert np.array_equal(neighbours.read(r), w["count"]), key
    assert info["queried"] == nq and (cells is None or cells(info["cells"])), (key, info)
    neighbours.count(r, RADIUS, 2, source=source, query=query)  # a limit: the uniform walk stops when every lane has reached it
    assert np.array_equal(neighbours.read(r), w["count2"]), key
    for k in KS:
        d2, near, unresolved = w["knn"][k]
        ki = nearest.search(r, k, RADIUS, source=source, query=query)
        g2, gn = nearest.read(r)
        assert np.array_equal(bits(g2), bits(d2)) and np.array_equal(gn, near), (key, k)
        assert ki["unresolved"] == unresolved and ki["candidates"] == info["candidates"], (key, k, ki)
    count, sums, si = w["surface"]
    ei = surface.estimate(r, RADIUS, source=source, query=query, keep_sums=True)
    assert np.array_equal(surface.read_sums(r), sums) and np.array_equal(surface.read(r)[2], count), key
    assert (ei["queried"], ei["sources"], ei["unresolved"]) == (si["queried"], si["sources"], si["unresolved"]), (key, ei, si)
    label, size = w["cluster"]
    ci = clusters.label(r, RADIUS, members=query)
    gl, gs = clusters.read(r)
    assert np.array_equal(gl, label) and np.array_equal(gs, size) and ci["members"] == nq, (key, ci)
    return info


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
def test_query_counts_in_one_cell(n):
    """1 .. 257 splats in the one cell around the origin: every wave with a query walks uniformly, and the lanes and waves without
    one sit in the same, dense, cell."""
    pos = one_cell(n)
    r = _mk(records(pos), 64, 64, 16)
    check_all(r, ("one_cell", n), pos, cells=lambda c: c == (1, 1, 1))
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
def test_query_counts_scattered(n):
    """The same counts over a box of several cells a side: the waves straddle cells and every lane walks its own spans."""
    pos = scattered(n)
    r = _mk(records(pos), 64, 64, 16)
    check_all(r, ("scattered", n), pos, cells=(lambda c: min(c) >= 3) if n >= 63 else None)
    r.destroy()


@pytest.mark.gpu
def test_mixed_waves():
    """256 queries in cell order: two waves that share a cell each, then two that straddle cells -- both paths in one workgroup."""
    pos = mixed_waves()
    r = _mk(records(pos), 64, 64, 16)
    info = check_all(r, "mixed", pos, cells=lambda c: min(c) >= 7)
    cell = np.floor((pos.astype(np.float64) - pos.min(axis=0)) / info["cell_edge"]).astype(np.int64)
    key = np.sort((cell[:, 2] * 1024 + cell[:, 1]) * 1024 + cell[:, 0])  # the cell order: x lowest
    waves = [np.unique(key[w:w + 64]).size for w in range(0, 256, 64)]
    assert waves[0] == 1 and waves[1] == 1 and waves[2] > 1 and waves[3] > 1 and key[0] != key[64], waves
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("nan_query", (False, True), ids=("finite", "nan_query"))
def test_queries_apart_from_sources(nan_query):
    """65 queries that are no sources in a cell that holds 200 of the 300 sources: the queries have records of their own, a wave of
    them walks the sources uniformly and self-exclusion by id excludes nobody.  With a NaN coordinate one query has no record: it
    keeps the plane value it started with (count 0, +inf / NONE, zero sums, its own label) and every call's `unresolved` counts it."""
    from gsplat import nearest, surface
    pos, st = apart(nan_query)
    src, qry = st == 1, st == 2
    r = _mk(records(pos), 64, 64, 16)
    r.write_state(st)
    check_all(r, ("apart", nan_query), pos, src, qry, SRC, QRY)
    if nan_query:
        i = int(np.flatnonzero(np.isnan(pos).any(axis=1))[0])
        w = want(("apart", nan_query), pos, src, qry)
        assert qry[i] and w["count"][i] == 0 and w["surface"][0][i] == 0 and w["cluster"][0][i] == i and w["cluster"][1][i] == 1
        plain = want(("apart", False), apart(False)[0], src, qry)  # (the same draws: only the one coordinate differs)
        for k in KS:
            assert bits(w["knn"][k][0])[i] == kr.INF_BITS and w["knn"][k][1][i] == kr.NONE and w["knn"][k][2] == plain["knn"][k][2] + 1
        assert w["surface"][2]["unresolved"] == plain["surface"][2]["unresolved"] + 1
        ki = nearest.search(r, 8, RADIUS, source=SRC, query=QRY)
        ei = surface.estimate(r, RADIUS, source=SRC, query=QRY, keep_sums=True)
        assert ki["unresolved"] == w["knn"][8][2] and ei["unresolved"] == w["surface"][2]["unresolved"]
    np.testing.assert_array_equal(r.read_state(), st)
    r.destroy()
