"""Thinning: a blue-noise subsample of the resident splats by rank and radius (include/gsplat/gs_abi.h "thinning").

Free functions over a ``Renderer`` or a ``PipelinedRenderer`` (whose splats, state plane and thinning planes live with its first
member: every slot is drained, then that member is asked), like ``gsplat.clusters``.  A sample keeps a subset of the member splats
such that no two kept ones are within `radius` of each other, every dropped one has a kept one within `radius`, and where two compete
the one of higher rank survives -- what would otherwise take export_splats (320 bytes per splat), a host k-d tree, a sequential
greedy loop and state_ids:

    thin.decimate(r, 0.02, priority=attributes.attr(_abi.GS_ATTR_COVER_SUM))   # real splats, the most seen one per neighbourhood
    q = thin.spread(r, 0.1)                                                    # evenly spaced query ids for a registration
    thin.dedupe(r, 1e-4)                                                       # after insert.merge_ply: the resident copy survives

Two member splats i != j are linked when (dx dx + dy dy) + dz dz <= radius * radius with d = p_j - p_i, every operation rounded once
to f32 and the comparison inclusive -- the neighbourhoods' expression --; a member with a NaN or infinite coordinate is linked to
nobody.  The rank is (priority key << 32) | hash of the index (order="hash": an even, seed-dependent choice) or | ~index
(order="index": the lower index wins); a NaN priority never wins.  keeper[i] is i for a kept member, the highest-ranked kept member
linked to i for a dropped one, NONE for a splat that is no member; covers[i] counts the members a kept splat stands for, itself
included, and is 0 for everyone else.  Both are integers a host can restate exactly (host_sample does, by another algorithm).  The
planes describe the positions, states and priorities at the time of sample(); an upload, a compaction or share_splats drops them
(they read NONE / 0).
"""
import ctypes
import math

import numpy as np

from . import _abi
from ._abi import check
from .neighbours import _owner

NONE = _abi.GS_THIN_NONE
DEFAULT_TAG = 0x80  # bit 7 of the state byte: the host's, free in every verb of this package
_ORDERS = {"hash": 0, "index": _abi.GS_THIN_ORDER_INDEX}


def _query(radius, where, priority, ascending, order, seed, max_rounds, max_candidates, host=False):
    if order not in _ORDERS:
        raise ValueError("thin: order %r is not 'hash' or 'index'" % (order,))
    q = _abi.GsThin()
    q.struct_size, q.radius, q.mask, q.value = ctypes.sizeof(_abi.GsThin), float(radius), int(where[0]), int(where[1])
    q.flags = _ORDERS[order] | (_abi.GS_THIN_ASCENDING if ascending else 0)
    q.seed, q.max_rounds, q.max_candidates = int(seed) & 0xFFFFFFFF, int(max_rounds), int(max_candidates)
    if priority is None or host:
        q.priority.struct_size, q.priority.kind = ctypes.sizeof(_abi.GsAttr), _abi.GS_THIN_NO_PRIORITY
    else:
        q.priority = priority
    return q


def _info(info):
    return {"members": int(info.members), "kept": int(info.kept), "dropped": int(info.dropped), "largest": int(info.largest),
            "candidates": int(info.candidates), "rounds": int(info.rounds), "cells": tuple(int(v) for v in info.cells),
            "cell_edge": float(info.cell_edge)}


def sample(r, radius, where=(0, 0), priority=None, ascending=False, order="hash", seed=0, max_rounds=0, max_candidates=0):
    """gs_thin_sample: samples the splats that pass `where` (mask, value) into the keeper and covers planes.  priority: a GsAttr
    (attributes.attr) whose value ranks the members, the larger the better (ascending: the smaller), or None; order: what decides among
    equal priorities, "hash" (of the index and `seed`) or "index" (the lower index wins).  Returns {"members", "kept", "dropped",
    "largest", "candidates", "rounds", "cells", "cell_edge"}.  max_rounds: the cap on the rounds (0: the library's default, enough
    for the hash order; an index order over a spatially sorted scene needs as many rounds as its longest chain); max_candidates: the
    work budget of a round.  A call that would exceed either raises GsError(GS_ERR_CAPACITY) and leaves the planes as they were."""
    o = _owner(r)
    q = _query(radius, where, priority, ascending, order, seed, max_rounds, max_candidates)
    info = _abi.GsThinInfo()
    check(o._L.gs_thin_sample(o._ctx, ctypes.byref(q), ctypes.byref(info)))
    return _info(info)


def read(r):
    """gs_thin_read: (keeper, covers), uint32[N] each in splat order (NONE / 0 before the first sample())."""
    o = _owner(r)
    n = ctypes.c_uint64()
    check(o._L.gs_thin_read(o._ctx, None, None, 0, ctypes.byref(n)))
    keeper, covers = np.full(n.value, NONE, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32)
    if n.value:
        check(o._L.gs_thin_read(o._ctx, keeper.ctypes.data, covers.ctypes.data, n.value, ctypes.byref(n)))
    return keeper, covers


def select(r, min_covers, max_covers, inside=True, where=(0, 0), op=_abi.GS_STATE_SET, bits=_abi.GS_SPLAT_SELECTED):
    """gs_state_thin: applies `op` (GS_STATE_*) with `bits` to the splats that pass `where` and whose covers c of the last sample()
    has (min_covers <= c <= max_covers) == inside; returns how many those are.  A dropped member and a splat that was no member have
    covers 0; min_covers > max_covers is the empty range."""
    o = _owner(r)
    matched = ctypes.c_uint64()
    check(o._L.gs_state_thin(o._ctx, int(min_covers), int(max_covers), 1 if inside else 0, int(where[0]), int(where[1]), int(op), int(bits),
                             ctypes.byref(matched)))
    return int(matched.value)


def host_sample(pos, radius, state=None, where=(0, 0), priority=None, ascending=False, order="hash", seed=0):
    """gs_thin_host: the same sample over host positions float32[n, 3], an optional state plane uint8[n] and optional priority VALUES
    float32[n] -- no renderer, no GPU, another algorithm (a sequential greedy in rank order).  Returns (keeper, covers, info)."""
    p = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    x, y, z = (np.ascontiguousarray(p[:, k]) for k in range(3))
    st = None if state is None else np.ascontiguousarray(state, dtype=np.uint8)
    pr = None if priority is None else np.ascontiguousarray(priority, dtype=np.float32)
    if (st is not None and st.size != n) or (pr is not None and pr.size != n):
        raise ValueError("host_sample: state and priority hold one value per position (%d)" % n)
    q = _query(radius, where, None, ascending, order, seed, 0, 0, host=True)
    keeper, covers = np.full(max(n, 1), NONE, dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
    info = _abi.GsThinInfo()
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    check(_abi.load().gs_thin_host(ptr(x), ptr(y), ptr(z), n, ptr(st), ptr(pr), ctypes.byref(q), keeper.ctypes.data, covers.ctypes.data,
                                   ctypes.byref(info)))
    return keeper[:n], covers[:n], _info(info)


# ---- the editor's verbs --------------------------------------------------------------------------------------------------------------
def select_kept(r, where=(0, 0), op=_abi.GS_STATE_SET, bits=_abi.GS_SPLAT_SELECTED):
    """Applies `op` with `bits` to the kept splats of the last sample() that pass `where`; returns their number."""
    return select(r, 1, 0xFFFFFFFF, where=where, op=op, bits=bits)


def select_dropped(r, where=(0, 0), op=_abi.GS_STATE_SET, bits=_abi.GS_SPLAT_SELECTED):
    """Applies `op` with `bits` to the splats with covers 0 that pass `where` -- the dropped members of the last sample() when `where`
    is its member filter and the states have not changed since; returns their number."""
    return select(r, 0, 0, where=where, op=op, bits=bits)


def _check_tag(o, tag):
    tag = int(tag)
    if tag <= 0 or tag > 0xFF or (tag & (tag - 1)):
        raise ValueError("thin: tag 0x%x is not one bit of the state byte" % tag)
    if o.state_count(tag, tag):
        raise ValueError("thin: %d splats already carry the tag 0x%x" % (o.state_count(tag, tag), tag))
    return tag


def decimate(r, radius, where=(0, 0), priority=None, ascending=False, order="hash", seed=0, max_rounds=0, max_candidates=0, tag=DEFAULT_TAG):
    """sample(), then the dropped members are compacted away: tagged with the state bit `tag` (one no splat carries, refused otherwise,
    and none carries afterwards) and removed by compact(tag, 0).  Returns (info, ids): sample()'s info and the compaction's id map,
    ids[new index] = old index.  The kept splats and the splats that were no members stay, in their order, with their records and
    states bit for bit: an EXACT frame afterwards is a fresh context's of those records.  Needs GS_FLAG_SPLAT_STATE.  Like every
    compaction it drops the coverage, neighbour, cluster, nearest-neighbour, surface and thinning planes."""
    o = _owner(r)
    tag = _check_tag(o, tag)
    if int(where[0]) & tag:
        raise ValueError("thin: the member filter (0x%x, 0x%x) reads the tag 0x%x" % (int(where[0]), int(where[1]), tag))
    info = sample(r, radius, where, priority, ascending, order, seed, max_rounds, max_candidates)
    if not info["dropped"]:
        return info, np.arange(o.numGaussians, dtype=np.uint32)
    select_dropped(r, where=where, op=_abi.GS_STATE_SET, bits=tag)
    try:
        ids = r.compact(tag, 0)
    except Exception:
        o.state_region(_abi.GS_REGION_ALL, _abi.GS_STATE_CLEAR, tag)  # the next verb must not find the tag
        raise
    return info, ids


def decimate_to(r, target, where=(0, 0), priority=None, ascending=False, order="hash", seed=0, max_rounds=0, max_candidates=0, tag=DEFAULT_TAG,
                probes=24):
    """decimate() at a radius found by bisection on the number of KEPT members, with at most `probes` (<= 24) samples.  The kept count
    is not strictly monotone in the radius, so no optimum is promised: of the radii probed, the one whose kept count is nearest to
    `target` without exceeding it is used.  The first probe (radius 0) learns the members, the exact duplicates and the scene's extent
    from the grid it reports; the others bisect geometrically between a thousandth of that grid's cell and the whole extent.  A probe
    the work budget or the round cap refuses counts as too coarse.  Returns {"radius", "kept", "splats", "probes", "info", "ids"};
    nothing is changed and "ids" is None when no probe reaches the target (target below the members with a non-finite coordinate
    plus one)."""
    o = _owner(r)
    tag = _check_tag(o, tag)
    probes = max(2, min(int(probes), 24))
    target = int(target)
    used, best = 0, None

    def probe(radius):  # True: at most target kept; False: more; None: refused (too coarse a radius for the budget)
        nonlocal used, best
        used += 1
        try:
            i = sample(r, radius, where, priority, ascending, order, seed, max_rounds, max_candidates)
        except _abi.GsError as e:
            if e.code != _abi.GS_ERR_CAPACITY:
                raise
            return None, None
        ok = i["kept"] <= target
        if ok and (best is None or i["kept"] > best[1]["kept"]):
            best = (radius, i)
        return ok, i

    ok, i = probe(0.0)
    if i is None or not i["members"]:
        return {"radius": None, "kept": i["kept"] if i else None, "splats": o.numGaussians, "probes": used, "info": i, "ids": None}
    if not ok:
        lo = max(i["cell_edge"] * 1e-3, 1e-30)
        hi = max(i["cell_edge"] * max(i["cells"]) * 2.0, lo * 2.0)  # above the diagonal's longest side: one finite member is kept
        while used < probes and hi / lo > 1.0 + 1e-6:
            mid = math.sqrt(lo * hi)
            if probe(mid)[0] is False:
                lo = mid
            else:
                hi = mid
    if best is None:
        return {"radius": None, "kept": None, "splats": o.numGaussians, "probes": used, "info": None, "ids": None}
    info, ids = decimate(r, best[0], where, priority, ascending, order, seed, max_rounds, max_candidates, tag)
    return {"radius": best[0], "kept": info["kept"], "splats": o.numGaussians, "probes": used, "info": info, "ids": ids}


def dedupe(r, radius, where=(0, 0), max_rounds=0, tag=DEFAULT_TAG):
    """decimate() in index order without a priority: of the members within `radius` of each other the one with the lowest index
    survives (after insert.merge_ply: the resident one).  radius 0 collapses exact duplicates only.  Returns (info, ids)."""
    return decimate(r, radius, where, order="index", max_rounds=max_rounds, tag=tag)


def spread(r, radius, where=(0, 0), priority=None, seed=0, tag=DEFAULT_TAG):
    """The ids, ascending, of a sample's kept members: an evenly spaced subset (a registration's query set that the densest wall does
    not dominate, seeds for anything per region).  The scene is not changed; with GS_FLAG_SPLAT_STATE the list comes from the device
    (list_state over a tag bit that is set and cleared again), without it from the planes."""
    o = _owner(r)
    info = sample(r, radius, where, priority, seed=seed)
    if not info["kept"]:
        return np.empty(0, dtype=np.uint32)
    if not (o.flags & _abi.GS_FLAG_SPLAT_STATE):
        keeper, _ = read(r)
        return np.flatnonzero(keeper == np.arange(keeper.size, dtype=np.uint32)).astype(np.uint32)
    tag = _check_tag(o, tag)
    select_kept(r, where=where, op=_abi.GS_STATE_SET, bits=tag)
    try:
        return o.list_state(tag, tag)
    finally:
        o.state_region(_abi.GS_REGION_ALL, _abi.GS_STATE_CLEAR, tag)
