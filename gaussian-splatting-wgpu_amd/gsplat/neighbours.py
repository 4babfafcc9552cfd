"""Neighbourhoods: count the splats within a radius of each splat, select by that count (include/gsplat/gs_abi.h "neighbourhoods").

Free functions over a ``Renderer`` or a ``PipelinedRenderer`` (whose splats, state plane and count plane live with its first
member: every slot is drained, then that member is asked).  Every other selection asks about one splat at a time; these ask about a
splat in relation to the others, on the device: what would otherwise take export_splats (320 bytes per splat), a host k-d tree and
state_ids is one call that leaves a u32 per splat resident.

    neighbours.select_isolated(r, 0.05, 3)                     # floaters: fewer than 3 others within 0.05 ...
    r.hide_selected()                                          # ... hidden
    neighbours.grow_selection(r, 0.02)                         # a lasso is never exact: take what lies within 0.02 of it too

The count of a query splat i is min(limit, #{j != i : j a source, (dx dx + dy dy) + dz dz <= radius * radius}) with d = p_j - p_i,
every operation rounded once to f32 and the comparison inclusive, so a host can restate it exactly; a splat with a NaN or infinite
coordinate has no neighbours and is nobody's.  The plane describes the positions and states at the time of count(): move or
re-filter the splats and count again.  An upload, a compaction or share_splats drops it (it reads as zeros).
"""
import ctypes

import numpy as np

from . import _abi
from ._abi import check

LIMIT_NONE = _abi.GS_NEIGH_LIMIT_NONE
_SEL, _HID = _abi.GS_SPLAT_SELECTED, _abi.GS_SPLAT_HIDDEN


def _owner(r):
    """The renderer that holds the splats: a PipelinedRenderer's state owner (its slots drained first), or r itself."""
    return r._state_owner() if hasattr(r, "_state_owner") else r


def count(r, radius, limit=LIMIT_NONE, source=(0, 0), query=(0, 0), max_candidates=0):
    """gs_neigh_count: counts, for every splat that passes `query` (mask, value), the splats that pass `source` within `radius` of
    it (itself excluded), saturating at `limit`, into the count plane; every other splat gets 0.  Returns {"queried", "sources",
    "candidates", "cells", "cell_edge"}: how many splats pass the two filters, the distance tests the device's grid left to do, and
    that grid (diagnostic: no count depends on it).  max_candidates: the work budget (0: the library's default); a call that
    would exceed it raises GsError(GS_ERR_CAPACITY) and leaves the plane as it was."""
    o = _owner(r)
    q = _abi.GsNeigh()
    q.struct_size, q.radius, q.limit = ctypes.sizeof(_abi.GsNeigh), float(radius), int(limit)
    q.src_mask, q.src_value, q.qry_mask, q.qry_value = int(source[0]), int(source[1]), int(query[0]), int(query[1])
    q.reserved, q.max_candidates = 0, int(max_candidates)
    info = _abi.GsNeighInfo()
    check(o._L.gs_neigh_count(o._ctx, ctypes.byref(q), ctypes.byref(info)))
    return {"queried": int(info.queried), "sources": int(info.sources), "candidates": int(info.candidates),
            "cells": tuple(int(v) for v in info.cells), "cell_edge": float(info.cell_edge)}


def read(r):
    """gs_neigh_read: the count plane, uint32[N] in splat order (zeros before the first count())."""
    o = _owner(r)
    n = ctypes.c_uint64()
    check(o._L.gs_neigh_read(o._ctx, None, 0, ctypes.byref(n)))
    out = np.zeros(n.value, dtype=np.uint32)
    if n.value:
        check(o._L.gs_neigh_read(o._ctx, out.ctypes.data, out.size, ctypes.byref(n)))
    return out


def select(r, lo, hi, inside=True, where=(0, 0), op=_abi.GS_STATE_SET, bits=_abi.GS_SPLAT_SELECTED):
    """gs_state_neigh: applies `op` (GS_STATE_*) with `bits` to the splats that pass `where` and whose count c of the last count()
    has (lo <= c <= hi) == inside; returns how many those are.  lo > hi is the empty range."""
    o = _owner(r)
    matched = ctypes.c_uint64()
    check(o._L.gs_state_neigh(o._ctx, int(lo), int(hi), 1 if inside else 0, int(where[0]), int(where[1]), int(op), int(bits), ctypes.byref(matched)))
    return int(matched.value)


# ---- the editor's verbs ------------------------------------------------------------------------------------------------------------
def select_isolated(r, radius, k, where=(0, 0)):
    """Selects the splats passing `where` that have fewer than k others passing `where` within `radius` (floaters); returns their
    number.  k <= 0 selects nothing."""
    k = int(k)
    if k <= 0:
        return 0
    count(r, radius, limit=k, source=where, query=where)
    return select(r, 0, k - 1, where=where)


def grow_selection(r, radius):
    """Adds to the selection every visible, unselected splat within `radius` of a selected one; returns how many were added."""
    count(r, radius, limit=1, source=(_SEL, _SEL), query=(_SEL | _HID, 0))
    return select(r, 1, LIMIT_NONE, where=(_SEL | _HID, 0))


def shrink_selection(r, radius):
    """Takes out of the selection every selected splat within `radius` of a visible, unselected one (its rim); returns how many
    were taken out."""
    count(r, radius, limit=1, source=(_SEL | _HID, 0), query=(_SEL, _SEL))
    return select(r, 1, LIMIT_NONE, where=(_SEL, _SEL), op=_abi.GS_STATE_CLEAR)
