"""Simplify: merge the splats of each grid cell into one moment-matched splat (include/gsplat/gs_abi.h "cell merge").

Free functions over a ``Renderer`` or a ``PipelinedRenderer``, like gsplat.insert.  ``hide_unseen`` + ``compact`` only drop splats and
``packed.save`` only shrinks bytes; these make a scene SMALLER without punching holes in it, and without the export / host script /
re-upload round trip:

    info, ids = simplify.simplify(r, 0.02)                      # every 2 cm cell with two or more splats becomes one splat
    out = simplify.simplify_to(r, 5_000_000)                    # ... or: at most 5 M splats, by bisecting the cell edge

Like a compaction, a simplification renumbers the splats: a gsplat.snapshots snapshot taken before it does not restore into the new
numbering, so what must be undoable is saved first (export_splats, packed.save) and uploaded again.

A cell's eligible splats -- those that pass the filter, with a finite position, a finite covariance and a positive weight -- are
replaced by ONE splat with their weighted mean position, the covariance of the mixture (each member's own covariance plus the spread
of the centres), the weighted mean SH (world frame: no rotation) and an opacity that conserves opacity x cross-section area, capped at
0.99; the weight is opacity x the area of the two largest axes, so a flat surfel weighs by its area.  k coincident copies of a splat
merge into that splat with opacity min(0.99, k a).  Cells with fewer than min_members eligible splats, and every splat that is not
eligible, are left exactly as they are.

Everything up to the group sums is pinned bit for bit (f32 with one rounding per operation, f64 sums in ascending index) and
``host_merge`` runs the same code without a GPU; the records follow from the sums by a 3x3 f64 Jacobi, pinned up to the last places of
/, sqrt and log.  The grid is anchored at the bounds of the filter's splats, so the number of groups is NOT monotone in the edge.
"""
import ctypes
import math

import numpy as np

from . import _abi, insert
from ._abi import check
from .neighbours import _owner

NONE = _abi.GS_MERGE_NONE
DEFAULT_TAG = 0x80  # bit 7 of the state byte: the host's, free in every verb of this package


def _params(cell, mask, value, min_members, max_members, op, bits):
    p = _abi.GsMerge()
    p.struct_size, p.mask, p.value, p.cell = ctypes.sizeof(_abi.GsMerge), int(mask), int(value), float(cell)
    p.min_members, p.max_members, p.op, p.bits = int(min_members), int(max_members), int(op), int(bits)
    return p


def _info(i):
    return {"eligible": int(i.eligible), "groups": int(i.groups), "members": int(i.members), "largest": int(i.largest),
            "cells": tuple(int(v) for v in i.cells), "cell_edge": float(i.cell_edge)}


def count(r, cell, mask=0, value=0, min_members=2, max_members=0):
    """gs_cell_merge in its count-only mode: {"eligible", "groups", "members", "largest", "cells", "cell_edge"} of a merge with these
    parameters; nothing is written or marked.  The scene would shrink by members - groups splats.  A cell fuller than max_members
    (0: 65536) raises GsError(GS_ERR_CAPACITY) as the merge itself would."""
    o = _owner(r)
    p, info = _params(cell, mask, value, min_members, max_members, 0, 0), _abi.GsMergeInfo()
    check(o._L.gs_cell_merge(o._ctx, ctypes.byref(p), None, 0, None, None, ctypes.byref(info)))
    return _info(info)


def merge_cells(r, cell, mask=0, value=0, min_members=2, max_members=0, op=0, bits=0, device=False, sums=False, group_of=False, groups=None):
    """gs_cell_merge[_device]: the merged records, float32[G, 80] in group order (ascending cell key) -- a numpy array, or with
    device=True a torch tensor on the renderer's device that never crosses PCIe -- and the info of count().  With sums / group_of a
    third value, a dict: "sums" float64[G, 64] (W, S[3], M[6], H[48], members, first index, c[3], 0) and "group_of" uint32[N], the
    group of every splat or NONE.  op / bits: a GS_STATE_* operation applied to the members of merged groups after the outputs are
    complete (0: none).  The scene itself is not changed: see simplify().  The record buffer is sized by a count() of its own (bounds,
    keys, sort and runs a second time) unless `groups` gives the number a count() with the same arguments reported; too small a number
    is refused by the library before anything is written or marked."""
    o = _owner(r)
    G = count(r, cell, mask, value, min_members, max_members)["groups"] if groups is None else int(groups)
    p, info = _params(cell, mask, value, min_members, max_members, op, bits), _abi.GsMergeInfo()
    extra = {}
    s = np.zeros((G, 64), dtype=np.float64) if sums else None
    g = np.full(o.numGaussians, NONE, dtype=np.uint32) if group_of else None
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    if device:
        import torch
        dev = torch.device("cuda", o.device)
        rec = torch.empty((max(G, 1), 80), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()  # the allocator may hand out memory another stream still uses
        check(o._L.gs_cell_merge_device(o._ctx, ctypes.byref(p), rec.data_ptr(), G, ptr(s), ptr(g), ctypes.byref(info)))
        rec = rec[:G]
    else:
        rec = np.zeros((max(G, 1), 80), dtype=np.float32)
        check(o._L.gs_cell_merge(o._ctx, ctypes.byref(p), rec.ctypes.data, G, ptr(s), ptr(g), ctypes.byref(info)))
        rec = rec[:G]
    if sums:
        extra["sums"] = s
    if group_of:
        extra["group_of"] = g
    return (rec, _info(info), extra) if (sums or group_of) else (rec, _info(info))


def host_merge(records, state, cell, mask=0, value=0, min_members=2, max_members=0, op=0, bits=0, count_only=False, cap=None):
    """gs_cell_merge_host: the same computation over host records (float32[n, 80]) and an optional state plane (uint8[n], marked IN
    PLACE when op is given) -- no renderer, no GPU, the same code.  Returns (records, info, {"sums", "group_of"}); count_only: (None,
    info, {}).  cap: the record capacity to offer (default: exactly the groups)."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 80)
    n = rec.shape[0]
    if state is not None and (state.dtype != np.uint8 or not state.flags["C_CONTIGUOUS"] or state.size != n):
        raise ValueError("host_merge: the state plane must be a contiguous uint8[%d]" % n)
    L = _abi.load()
    p, info = _params(cell, mask, value, min_members, max_members, 0, 0), _abi.GsMergeInfo()
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    check(L.gs_cell_merge_host(ptr(rec), ptr(state), n, ctypes.byref(p), None, 0, None, None, ctypes.byref(info)))
    if count_only:
        return None, _info(info), {}
    G = int(info.groups)
    cap = G if cap is None else int(cap)
    out = np.zeros((max(cap, 1), 80), dtype=np.float32)
    s, g = np.zeros((max(G, 1), 64), dtype=np.float64), np.full(max(n, 1), NONE, dtype=np.uint32)
    p = _params(cell, mask, value, min_members, max_members, op, bits)
    check(L.gs_cell_merge_host(ptr(rec), ptr(state), n, ctypes.byref(p), out.ctypes.data, cap, s.ctypes.data, g.ctypes.data, ctypes.byref(info)))
    return out[:G], _info(info), {"sums": s[:G], "group_of": g[:n]}


# ---- the editor's verbs --------------------------------------------------------------------------------------------------------------
def simplify(r, cell, mask=0, value=0, tag=DEFAULT_TAG, new_state=0, min_members=2, max_members=0, groups=None):
    """Replaces the eligible splats of every cell of edge `cell` that holds min_members or more of them by their merged splat:
    merge_cells into a device buffer with the members tagged, insert.append of the records with the state byte new_state,
    compact(tag, 0).  Returns (info, ids): count()'s info, and the compaction's id map -- ids[new index] = old index for the splats
    that were kept, which keep their order; the merged splats follow in group order and read N_old + group in it.  Needs
    GS_FLAG_SPLAT_STATE; `tag` is a state bit no splat carries (refused otherwise) and none carries afterwards.  The coverage,
    neighbour, cluster and nearest-neighbour planes are dropped, as insertion and compaction document; gsplat.snapshots taken
    before the call refuse to restore into the new numbering: export what must be undoable.  groups: as for merge_cells (what a
    count() with the same arguments reported: saves the sizing pass).  If the insertion or the compaction fails (out of memory), the
    tag is cleared again before the error is raised: the members stay, unmarked, and any records already appended stay too."""
    o = _owner(r)
    tag, new_state = int(tag), int(new_state)
    if tag <= 0 or tag > 0xFF or (tag & (tag - 1)):
        raise ValueError("simplify: tag 0x%x is not one bit of the state byte" % tag)
    if new_state & tag:
        raise ValueError("simplify: new_state 0x%x carries the tag 0x%x" % (new_state, tag))
    if o.state_count(tag, tag):
        raise ValueError("simplify: %d splats already carry the tag 0x%x" % (o.state_count(tag, tag), tag))
    n_old = o.numGaussians
    rec, info = merge_cells(r, cell, mask, value, min_members, max_members, _abi.GS_STATE_SET, tag, device=True, groups=groups)
    if not info["groups"]:
        return info, np.arange(n_old, dtype=np.uint32)
    try:
        insert.append(r, rec, new_state)
        ids = r.compact(tag, 0)
    except Exception:
        _owner(r).state_region(_abi.GS_REGION_ALL, _abi.GS_STATE_CLEAR, tag)  # the next simplify must not find the tag
        raise
    return info, ids


def simplify_to(r, target, mask=0, value=0, tag=DEFAULT_TAG, new_state=0, min_members=2, max_members=0, probes=24):
    """simplify() at the smallest cell edge found, with at most `probes` (<= 24) count-only probes, whose result has at most `target`
    splats: the first probe asks for the finest grid there is (1024 cells on the widest axis) and learns the scene's extent from the
    edge it reports, the others bisect the edge geometrically between that and one cell for everything.  Returns {"edge", "splats",
    "probes", "info", "ids"}; nothing is changed and "ids" is None when no probed edge reaches the target (a cell fuller than
    max_members counts as not reaching it).  No monotonicity is promised: the grid is anchored at the bounds."""
    o = _owner(r)
    probes = max(2, min(int(probes), 24))
    n = o.numGaussians
    used = 0
    best = None

    def probe(edge):  # True: reaches the target; False: too many splats left; None: a cell is fuller than max_members
        nonlocal used, best
        used += 1
        try:
            i = count(r, edge, mask, value, min_members, max_members)
        except _abi.GsError as e:
            if e.code != _abi.GS_ERR_CAPACITY:
                raise
            return None, None
        ok = n - i["members"] + i["groups"] <= target
        if ok and (best is None or i["cell_edge"] < best[0]):
            best = (i["cell_edge"], i)
        return ok, i

    ok, i = probe(1e-30)
    if i is None or not i["eligible"]:
        return {"edge": None, "splats": n, "probes": used, "info": i, "ids": None}
    if not ok:
        lo = i["cell_edge"]
        hi = lo * 1024.0 * 1.01  # one cell holds every eligible splat
        probe(hi)
        while used < probes and hi / lo > 1.0 + 1e-6:
            mid = math.sqrt(lo * hi)
            if probe(mid)[0] is False:
                lo = mid
            else:
                hi = mid
    if best is None:
        return {"edge": None, "splats": n, "probes": used, "info": None, "ids": None}
    info, ids = simplify(r, best[0], mask, value, tag, new_state, min_members, max_members, groups=best[1]["groups"])
    return {"edge": info["cell_edge"], "splats": _owner(r).numGaussians, "probes": used, "info": info, "ids": ids}
