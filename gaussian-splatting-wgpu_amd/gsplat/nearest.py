"""Nearest neighbours: the k-th nearest distance and the nearest splat's id per splat (include/gsplat/gs_abi.h "nearest neighbours").

Free functions over a ``Renderer`` or a ``PipelinedRenderer`` (whose splats, state plane and the two planes live with its first
member: every slot is drained, then that member is asked), like ``gsplat.neighbours``.  A count and a labelling make the caller know
a radius first; these answer with the distance itself, on the device -- what would otherwise take export_splats (320 bytes per
splat), a host k-d tree and state_ids:

    nearest.select_outliers(r, 8, 2.0); r.hide_selected()      # statistical outlier removal: no radius, k and a sigma
    nearest.distances(r, 1); d2, j = nearest.read(r)           # the local spacing sqrt(d2), and each splat's nearest other splat

For a query splat i let D be the multiset of (dx dx + dy dy) + dz dz <= radius * radius over the source splats j != i, d = p_j - p_i,
every operation rounded once to f32 and the comparison inclusive -- the neighbourhoods' expression.  dist2[i] is the k-th smallest
element of D, or +inf when D has fewer than k ("unresolved"); nearest[i] is the smallest index j that attains the minimum of D, or
NONE when D is empty; a splat that is no query reads NaN (0x7FC00000) / NONE.  A splat with a NaN or infinite coordinate has no
neighbours and is nobody's.  A resolved dist2 (and, for k = 1, its nearest) does not depend on the radius: only whether a query is
resolved does, which is what distances() builds the radius-free search on.  The planes describe the positions and states at the time
of the search: move or re-filter the splats and search again.  An upload, a compaction or share_splats drops them (NaN / NONE).
"""
import ctypes

import numpy as np

from . import _abi, attributes
from ._abi import check
from .neighbours import _owner

NONE = _abi.GS_KNN_NONE
MAX_K = _abi.GS_KNN_MAX_K


def search(r, k, radius, source=(0, 0), query=(0, 0), refine=False, max_candidates=0):
    """gs_knn_search: for every splat that passes `query` (mask, value), the k-th smallest squared distance to the splats that pass
    `source` within `radius` of it (itself excluded) and the nearest of them, into the two planes; every other splat gets NaN /
    NONE.  refine: only the splats whose dist2 reads +inf now are queried and written (same k as the last search).  Returns
    {"queried", "sources", "candidates", "unresolved", "cells", "cell_edge"}: how many splats pass the two filters, the distance
    tests the device's grid left to do, the queries that end +inf, and that grid (diagnostic: no result depends on it).
    max_candidates: the work budget (0: the library's default); a call that would exceed it raises GsError(GS_ERR_CAPACITY) and
    leaves the planes as they were."""
    o = _owner(r)
    q = _abi.GsKnn()
    q.struct_size, q.radius, q.k, q.flags = ctypes.sizeof(_abi.GsKnn), float(radius), int(k), _abi.GS_KNN_REFINE if refine else 0
    q.src_mask, q.src_value, q.qry_mask, q.qry_value = int(source[0]), int(source[1]), int(query[0]), int(query[1])
    q.max_candidates, q.reserved = int(max_candidates), 0
    info = _abi.GsKnnInfo()
    check(o._L.gs_knn_search(o._ctx, ctypes.byref(q), ctypes.byref(info)))
    return {"queried": int(info.queried), "sources": int(info.sources), "candidates": int(info.candidates), "unresolved": int(info.unresolved),
            "cells": tuple(int(v) for v in info.cells), "cell_edge": float(info.cell_edge)}


def read(r):
    """gs_knn_read: (dist2 float32[N], nearest uint32[N]) in splat order (NaN / NONE before the first search())."""
    o = _owner(r)
    n = ctypes.c_uint64()
    check(o._L.gs_knn_read(o._ctx, None, None, 0, ctypes.byref(n)))
    dist2, near = np.full(n.value, np.nan, dtype=np.float32), np.full(n.value, NONE, dtype=np.uint32)
    if n.value:
        check(o._L.gs_knn_read(o._ctx, dist2.ctypes.data, near.ctypes.data, n.value, ctypes.byref(n)))
    return dist2, near


def select(r, lo, hi, inside=True, where=(0, 0), op=_abi.GS_STATE_SET, bits=_abi.GS_SPLAT_SELECTED):
    """gs_state_knn: applies `op` (GS_STATE_*) with `bits` to the splats that pass `where` and whose dist2 v of the last search has
    (lo <= v <= hi) == inside; returns how many those are.  A NaN (no query) is in no range, hi = +inf includes the unresolved,
    lo > hi is the empty range."""
    o = _owner(r)
    matched = ctypes.c_uint64()
    check(o._L.gs_state_knn(o._ctx, float(lo), float(hi), 1 if inside else 0, int(where[0]), int(where[1]), int(op), int(bits), ctypes.byref(matched)))
    return int(matched.value)


# ---- the editor's verbs ------------------------------------------------------------------------------------------------------------
def _diagonal(r, where):
    """(diagonal of the bounds of the splats passing `where` in float64 -- inf when a coordinate is, 0 when there is none --, their number)"""
    lo, hi, matched = attributes.bounds(r, where)
    if not matched:
        return 0.0, 0
    with np.errstate(all="ignore"):
        ext = hi.astype(np.float64) - lo.astype(np.float64)
    ext = np.where(np.isnan(ext) | (ext < 0), 0.0, ext)  # (an axis on which every coordinate is NaN)
    return float(np.sqrt((ext * ext).sum())), int(matched)


def distances(r, k, where=(0, 0), radius=None, max_rounds=40, max_candidates=0):
    """The radius-free search among the splats that pass `where` (sources and queries alike): a search at a starting radius -- the
    given one, or one from the members' bounds and number; any positive start is correct, only speed depends on it --, halved (at most
    20 times) while the first round exceeds the work budget, then doubled with refine=True while queries are unresolved, until the
    radius exceeds twice the diagonal of the members' bounds or after max_rounds searches.  What is still unresolved stays +inf:
    queries with fewer than k other members with finite coordinates, or with a non-finite coordinate themselves.  Returns {"rounds",
    "radius", "unresolved", "candidates"}: the searches run, the last radius, the queries left +inf and the distance tests of all
    rounds."""
    k = int(k)
    diag, members = _diagonal(r, where)
    if radius is None or not float(radius) > 0.0:
        # a third of the radius whose ball holds k members were they spread evenly over the box (0.36 diag cbrt(k / m)): a capture is
        # denser than that where most of its splats are, a start too small costs a cheap round and one too large candidates by its cube
        radius = 0.125 * diag * (k / max(members, 1)) ** (1.0 / 3.0)
        if not (np.isfinite(radius) and radius > 0.0):
            radius = 1.0
    radius = float(radius)
    info = None
    for _ in range(21):
        try:
            info = search(r, k, radius, source=where, query=where, max_candidates=max_candidates)
            break
        except _abi.GsError as e:
            if e.code != _abi.GS_ERR_CAPACITY:
                raise
            last = e
            radius *= 0.5
    if info is None:
        raise last
    rounds, candidates = 1, info["candidates"]
    while info["unresolved"] > 0 and rounds < max_rounds and radius <= 2.0 * diag:
        if not np.isfinite(np.float32(2.0 * radius) * np.float32(2.0 * radius)):
            break  # (an infinite coordinate among the members: the diagonal never ends the search, the f32 square does)
        radius *= 2.0
        info = search(r, k, radius, source=where, query=where, refine=True, max_candidates=max_candidates)
        rounds += 1
        candidates += info["candidates"]
    return {"rounds": rounds, "radius": radius, "unresolved": info["unresolved"], "candidates": candidates}


def select_outliers(r, k, sigma, where=(0, 0)):
    """Statistical outlier removal among the splats that pass `where`: distances(), then on the host in float64 the threshold
    t = mean + sigma * std of sqrt(dist2) over the members' finite values, then select(lo = the float32 above float32(t)^2, hi = +inf):
    the members whose k-th nearest member is further than t away, the unresolved among them.  Returns the number selected."""
    distances(r, k, where=where)
    d2, _ = read(r)
    d = np.sqrt(d2[np.isfinite(d2)].astype(np.float64))  # (a splat that is no member reads NaN)
    lo = np.float32(np.inf)
    if d.size:
        t = np.float32(d.mean() + float(sigma) * d.std())
        with np.errstate(all="ignore"):
            lo = np.nextafter(t * t, np.float32(np.inf), dtype=np.float32)
    return select(r, lo, np.inf, where=where)
