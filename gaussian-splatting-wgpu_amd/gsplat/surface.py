"""Surface: per-splat normals and shape from the covariance of each splat's neighbourhood (include/gsplat/gs_abi.h "surface").

Free functions over a ``Renderer`` or a ``PipelinedRenderer`` (whose splats, state plane and the planes live with its first member:
every slot is drained, then that member is asked), like ``gsplat.nearest``.  A count, a label and a k-th distance are one scalar per
splat; this is the local geometry -- what would otherwise take export_splats (320 bytes per splat), a host k-d tree, a PCA per point
and state_ids:

    rad = surface.radius_for(r, 30)                                  # a radius that holds about 30 neighbours
    surface.select_planar(r, rad, 0.6)                               # everything that lies on a surface
    surface.select_facing(r, (0, 1, 0), 15.0)                        # ... the horizontal ones: floor, table tops and steps at once
    surface.select_fuzzy(r, rad, 0.15); r.hide_selected()            # floaters that are dense but have no surface
    normal, eig, count = surface.read(r)                             # oriented normals: estimate(..., toward=eye)

For a query splat i the accepted sources are the j != i with (dx dx + dy dy) + dz dz <= radius * radius, d = p_j - p_i, every
operation rounded once to f32 and the comparison inclusive -- the neighbourhoods' expression.  Each accepted difference is quantised
once, q = rint(d * 2^(16 - E)) with 2^(E-1) <= radius < 2^E, and the device adds INTEGERS: count, the three sums of q and the six of
q q, so nothing depends on the order of the visit.  The finishing is float64: mean, covariance, a fixed number of Jacobi sweeps;
eigenvalues l0 >= l1 >= l2 >= 0 in world units, the normal the eigenvector of l2 with its largest component positive (or facing
`toward`).  A query with fewer than 3 neighbours reads NaN and keeps its count; a splat that is no query reads NaN and count 0.  The
planes describe the positions and states at the time of the estimate: move or re-filter the splats and estimate again.  An upload, a
compaction or share_splats drops them.
"""
import ctypes
import math

import numpy as np

from . import _abi, nearest
from ._abi import check
from .neighbours import _owner

SUM_WORDS = _abi.GS_SURFACE_SUM_WORDS
KINDS = {"variation": _abi.GS_SURFACE_VARIATION, "planarity": _abi.GS_SURFACE_PLANARITY, "linearity": _abi.GS_SURFACE_LINEARITY,
         "sphericity": _abi.GS_SURFACE_SPHERICITY, "facing": _abi.GS_SURFACE_FACING, "facing_signed": _abi.GS_SURFACE_FACING_SIGNED,
         "count": _abi.GS_SURFACE_COUNT}


def _query(radius, source, query, toward, keep_sums, max_candidates):
    q = _abi.GsSurface()
    q.struct_size, q.radius = ctypes.sizeof(_abi.GsSurface), float(radius)
    q.flags = (_abi.GS_SURFACE_ORIENT if toward is not None else 0) | (_abi.GS_SURFACE_KEEP_SUMS if keep_sums else 0)
    q.src_mask, q.src_value, q.qry_mask, q.qry_value = int(source[0]), int(source[1]), int(query[0]), int(query[1])
    if toward is not None:
        q.toward[:] = [float(v) for v in toward]
    q.max_candidates, q.reserved = int(max_candidates), 0
    return q


def _info(info):
    return {"queried": int(info.queried), "sources": int(info.sources), "candidates": int(info.candidates), "unresolved": int(info.unresolved),
            "cells": tuple(int(v) for v in info.cells), "cell_edge": float(info.cell_edge)}


def estimate(r, radius, source=(0, 0), query=(0, 0), toward=None, keep_sums=False, max_candidates=0):
    """gs_surface_estimate: for every splat that passes `query` (mask, value), the normal, the three eigenvalues and the count of the
    splats that pass `source` within `radius` of it (itself excluded), into the planes; every other splat gets NaN / count 0.
    toward: a point (a viewpoint) the normals are turned to face.  keep_sums: keep the ten integers per splat for read_sums().
    Returns {"queried", "sources", "candidates", "unresolved", "cells", "cell_edge"}: how many splats pass the two filters, the
    distance tests the device's grid left to do, the queries that end with fewer than 3 neighbours, and that grid (diagnostic: no
    result depends on it).  max_candidates: the work budget (0: the library's default); a call that would exceed it raises
    GsError(GS_ERR_CAPACITY) and leaves the planes as they were."""
    o = _owner(r)
    q = _query(radius, source, query, toward, keep_sums, max_candidates)
    info = _abi.GsSurfaceInfo()
    check(o._L.gs_surface_estimate(o._ctx, ctypes.byref(q), ctypes.byref(info)))
    return _info(info)


def read(r):
    """gs_surface_read: (normal float32[N, 3], eig float32[N, 3], count uint32[N]) in splat order (NaN / 0 before the first estimate())."""
    o = _owner(r)
    n = ctypes.c_uint64()
    check(o._L.gs_surface_read(o._ctx, None, None, None, 0, ctypes.byref(n)))
    normal, eig = np.full((n.value, 3), np.nan, dtype=np.float32), np.full((n.value, 3), np.nan, dtype=np.float32)
    count = np.zeros(n.value, dtype=np.uint32)
    if n.value:
        check(o._L.gs_surface_read(o._ctx, normal.ctypes.data, eig.ctypes.data, count.ctypes.data, n.value, ctypes.byref(n)))
    return normal, eig, count


def read_sums(r):
    """gs_surface_read_sums: int64[N, 10] -- count, S x y z, M xx xy xz yy yz zz of the quantised differences -- of the last
    estimate(keep_sums=True); zeros for a splat that was no query.  Raises GsError when no sums are kept."""
    o = _owner(r)
    n = ctypes.c_uint64()
    check(o._L.gs_surface_read_sums(o._ctx, None, 0, ctypes.byref(n)))
    sums = np.zeros((n.value, SUM_WORDS), dtype=np.int64)
    if n.value:
        check(o._L.gs_surface_read_sums(o._ctx, sums.ctypes.data, n.value, ctypes.byref(n)))
    return sums


def select(r, kind, lo, hi, inside=True, axis=(0, 0, 0), where=(0, 0), op=_abi.GS_STATE_SET, bits=_abi.GS_SPLAT_SELECTED):
    """gs_state_surface: applies `op` (GS_STATE_*) with `bits` to the splats that pass `where` and whose feature v of the last
    estimate has (lo <= v <= hi) == inside; returns how many those are.  kind: a GS_SURFACE_* number or one of "variation" l2 / ((l0 +
    l1) + l2), "planarity" (l1 - l2) / l0, "linearity" (l0 - l1) / l0, "sphericity" l2 / l0, "facing" |n . axis|, "facing_signed"
    n . axis (axis as given, not normalised), "count".  A NaN (no query, fewer than 3 neighbours, 0 / 0) is in no range."""
    o = _owner(r)
    rg = _abi.GsSurfaceRange()
    rg.struct_size, rg.kind = ctypes.sizeof(_abi.GsSurfaceRange), int(KINDS.get(kind, kind))
    rg.lo, rg.hi, rg.inside = float(lo), float(hi), 1 if inside else 0
    rg.axis[:] = [float(v) for v in axis]
    matched = ctypes.c_uint64()
    check(o._L.gs_state_surface(o._ctx, ctypes.byref(rg), int(where[0]), int(where[1]), int(op), int(bits), ctypes.byref(matched)))
    return int(matched.value)


def host_estimate(pos, radius, state=None, source=(0, 0), query=(0, 0), toward=None):
    """gs_surface_host: the same computation over host positions (float32[n, 3]) without a renderer or a GPU, all pairs, compiled from
    the same header as the kernels.  state: uint8[n], needed with a filter other than (0, 0).  Returns (normal, eig, count, sums, info)
    as read(), read_sums() and estimate() do."""
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    n = pos.shape[0]
    st = None if state is None else np.ascontiguousarray(state, dtype=np.uint8)
    if st is not None and st.shape != (n,):
        raise ValueError("state must hold one byte per position")
    q = _query(radius, source, query, toward, False, 0)
    normal, eig = np.full((n, 3), np.nan, dtype=np.float32), np.full((n, 3), np.nan, dtype=np.float32)
    count, sums = np.zeros(n, dtype=np.uint32), np.zeros((n, SUM_WORDS), dtype=np.int64)
    info = _abi.GsSurfaceInfo()
    check(_abi.load().gs_surface_host(pos.ctypes.data, None if st is None else st.ctypes.data, n, ctypes.byref(q), normal.ctypes.data, eig.ctypes.data,
                                      count.ctypes.data, sums.ctypes.data, ctypes.byref(info)))
    return normal, eig, count, sums, _info(info)


# ---- the editor's verbs ------------------------------------------------------------------------------------------------------------
def radius_for(r, k, where=(0, 0)):
    """A radius that holds about k neighbours: nearest.distances(r, k, where), then the median over the members' finite values of the
    k-th nearest distance, in float64.  Returns 0.0 when no member has k neighbours."""
    nearest.distances(r, int(k), where=where)
    d2, _ = nearest.read(r)
    d2 = d2[np.isfinite(d2)].astype(np.float64)
    return float(np.median(np.sqrt(d2))) if d2.size else 0.0


def select_planar(r, radius, min_planarity, where=(0, 0), op=_abi.GS_STATE_SET, bits=_abi.GS_SPLAT_SELECTED):
    """Everything that lies on a surface: estimate() among the splats that pass `where`, then select("planarity", min_planarity, inf).
    Returns the number selected."""
    estimate(r, radius, source=where, query=where)
    return select(r, "planarity", min_planarity, np.inf, where=where, op=op, bits=bits)


def select_facing(r, axis, max_angle_deg, signed=False, where=(0, 0), op=_abi.GS_STATE_SET, bits=_abi.GS_SPLAT_SELECTED):
    """The splats whose normal of the last estimate() is within max_angle_deg of `axis` (either way round unless signed): the host
    normalises the axis and takes the cosine in float64, then rounds each once to float32, and select("facing" or "facing_signed", cos,
    inf).  Returns the number selected."""
    a = np.asarray(axis, dtype=np.float64).reshape(3)
    a = a / math.sqrt(float((a * a).sum()))
    cos = np.float32(math.cos(math.radians(float(max_angle_deg))))
    return select(r, "facing_signed" if signed else "facing", cos, np.inf, axis=a.astype(np.float32), where=where, op=op, bits=bits)


def select_fuzzy(r, radius, min_variation, where=(0, 0), op=_abi.GS_STATE_SET, bits=_abi.GS_SPLAT_SELECTED):
    """Dense clutter without a surface: estimate() among the splats that pass `where`, then select("variation", min_variation, inf)
    (surface variation is 0 on a plane and 1/3 for an isotropic blob).  Returns the number selected."""
    estimate(r, radius, source=where, query=where)
    return select(r, "variation", min_variation, np.inf, where=where, op=op, bits=bits)
