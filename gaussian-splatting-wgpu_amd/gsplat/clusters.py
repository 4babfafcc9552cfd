"""Clusters: label the splats that are connected within a radius, select by cluster (include/gsplat/gs_abi.h "clusters").

Free functions over a ``Renderer`` or a ``PipelinedRenderer`` (whose splats, state plane and cluster planes live with its first
member: every slot is drained, then that member is asked), like ``gsplat.neighbours``.  A neighbour count is a local answer: a
detached blob of floaters is dense inside and survives it.  These answer the global questions on the device -- what would
otherwise take export_splats (320 bytes per splat), a host k-d tree with connected components and state_ids:

    clusters.select_small_clusters(r, 0.05, 200); r.hide_selected()   # every island of at most 200 splats, hidden
    r.select_rect(x0, y0, x1, y1, u); clusters.select_connected(r, 0.05)   # the whole objects the rectangle touches
    clusters.select_largest_cluster(r, 0.05)                          # the main body

Two member splats i != j are linked when (dx dx + dy dy) + dz dz <= radius * radius with d = p_j - p_i, every operation rounded
once to f32 and the comparison inclusive -- the neighbourhoods' expression --; a member with a NaN or infinite coordinate is linked
to nobody.  A cluster is a connected component.  label[i] is the smallest splat index in i's cluster and size[i] its number of
members; a splat that is no member has label NONE and size 0.  Both are integers a host can restate exactly.  The planes describe
the positions and states at the time of label(): move or re-filter the splats and label again.  An upload, a compaction or
share_splats drops them (they read NONE / 0).
"""
import ctypes

import numpy as np

from . import _abi
from ._abi import check
from .neighbours import _owner

NONE = _abi.GS_CLUSTER_NONE
_SEL, _HID = _abi.GS_SPLAT_SELECTED, _abi.GS_SPLAT_HIDDEN
_VISIBLE = (_HID, 0)


def label(r, radius, members=(0, 0), max_candidates=0):
    """gs_cluster_label: labels the connected components of the splats that pass `members` (mask, value) into the label and size
    planes.  Returns {"members", "clusters", "largest", "candidates", "rounds", "cells", "cell_edge"}: how many splats pass the
    filter, how many clusters they form, the size of the largest, the distance tests of one round, the edge passes that were run,
    and the device's grid (diagnostic: no label depends on it).  max_candidates: the work budget of a round (0: the library's
    default); a call that would exceed it raises GsError(GS_ERR_CAPACITY) and leaves the planes as they were."""
    o = _owner(r)
    q = _abi.GsCluster()
    q.struct_size, q.radius, q.mask, q.value = ctypes.sizeof(_abi.GsCluster), float(radius), int(members[0]), int(members[1])
    q.max_candidates = int(max_candidates)
    info = _abi.GsClusterInfo()
    check(o._L.gs_cluster_label(o._ctx, ctypes.byref(q), ctypes.byref(info)))
    return {"members": int(info.members), "clusters": int(info.clusters), "largest": int(info.largest), "candidates": int(info.candidates),
            "rounds": int(info.rounds), "cells": tuple(int(v) for v in info.cells), "cell_edge": float(info.cell_edge)}


def read(r):
    """gs_cluster_read: (labels, sizes), uint32[N] each in splat order (NONE / 0 before the first label())."""
    o = _owner(r)
    n = ctypes.c_uint64()
    check(o._L.gs_cluster_read(o._ctx, None, None, 0, ctypes.byref(n)))
    labels, sizes = np.full(n.value, NONE, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32)
    if n.value:
        check(o._L.gs_cluster_read(o._ctx, labels.ctypes.data, sizes.ctypes.data, n.value, ctypes.byref(n)))
    return labels, sizes


def select(r, lo, hi, inside=True, where=(0, 0), op=_abi.GS_STATE_SET, bits=_abi.GS_SPLAT_SELECTED):
    """gs_state_cluster: applies `op` (GS_STATE_*) with `bits` to the splats that pass `where` and whose size s of the last label()
    has (lo <= s <= hi) == inside; returns how many those are.  A splat that was no member has size 0; lo > hi is the empty range."""
    o = _owner(r)
    matched = ctypes.c_uint64()
    check(o._L.gs_state_cluster(o._ctx, int(lo), int(hi), 1 if inside else 0, int(where[0]), int(where[1]), int(op), int(bits), ctypes.byref(matched)))
    return int(matched.value)


def select_linked(r, seeds=(_SEL, _SEL), where=(0, 0), op=_abi.GS_STATE_SET, bits=_abi.GS_SPLAT_SELECTED):
    """gs_state_cluster_linked: applies `op` with `bits` to the splats that pass `where`, were members of the last label() and whose
    cluster holds a splat that passes `seeds` as the states are now; returns how many those are."""
    o = _owner(r)
    matched = ctypes.c_uint64()
    check(o._L.gs_state_cluster_linked(o._ctx, int(seeds[0]), int(seeds[1]), int(where[0]), int(where[1]), int(op), int(bits), ctypes.byref(matched)))
    return int(matched.value)


# ---- the editor's verbs ------------------------------------------------------------------------------------------------------------
def select_small_clusters(r, radius, max_size):
    """Labels the visible splats and selects those in clusters of at most max_size members (islands); returns their number."""
    label(r, radius, members=_VISIBLE)
    return select(r, 1, max_size, where=_VISIBLE)


def select_connected(r, radius):
    """Extends the selection to the whole clusters of visible splats it touches; returns how many visible splats those clusters
    hold (the selected ones among them included)."""
    label(r, radius, members=_VISIBLE)
    return select_linked(r, seeds=(_SEL | _HID, _SEL), where=_VISIBLE)


def select_largest_cluster(r, radius):
    """Labels the visible splats and selects the largest cluster (every cluster of that size, should several share it); returns
    how many splats were selected."""
    info = label(r, radius, members=_VISIBLE)
    return select(r, info["largest"], info["largest"], where=_VISIBLE) if info["largest"] else 0
