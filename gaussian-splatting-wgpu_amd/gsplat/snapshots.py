"""Snapshots and write-back: exact undo for resident splat edits (include/gsplat/gs_abi.h "snapshots and write-back").

Free functions over a ``Renderer`` or a ``PipelinedRenderer`` (whose splats live with its first member: every slot is drained, then
that member is asked; the other members read the owner's planes, so nothing is shared again), like ``gsplat.insert`` and
``gsplat.colours``.  Every other call on the resident splats changes them in place and none can be taken back -- the inverse of a
transform or a grade rounds again.  These are the missing inverse of export_splats:

    with snapshots.take_selected_for(r, x) as undo:        # the parts the transform names, of the selection, on the device
        r.transform(x)                                      # ... the edit ...
        undo.swap()                                         # undo: the scene is bit for bit what it was, the snapshot holds the edit
        undo.swap()                                         # redo
    rec, ids = r.export_splats(2, 2, with_ids=True)        # a per-splat edit in the host's own code ...
    snapshots.write(r, ids, my_edit(rec))                  # ... put back by index, no upload

Floats are copied as words: nothing is computed but the derived largest log-scale, so NaN payloads, -0 and infinities arrive
unchanged.  A snapshot's memory follows the parts it holds (a POSITION snapshot: 12 bytes per splat plus the index).  It names
splats by index: it stays valid across insertions, and is refused (GsError) after an upload or a compaction, and on another
renderer.  None of the calls is a frame or an upload: taps, statistics, pick, a captured frame graph and the coverage, neighbour and
cluster planes stay; the next frame shows the result.  Multi-GPU: make the same call on every rank.
"""
import ctypes

import numpy as np

from . import _abi
from ._abi import check
from .neighbours import _owner

_SEL = _abi.GS_SPLAT_SELECTED
POSITION, GEOMETRY, SH, STATE, RECORD = (_abi.GS_PART_POSITION, _abi.GS_PART_GEOMETRY, _abi.GS_PART_SH, _abi.GS_PART_STATE,
                                         _abi.GS_PART_RECORD)


def write(r, ids, records, states=None, parts=RECORD):
    """gs_write_splats[_device]: record g of float32[m, 80] `records` goes to splat ids[g] (ids None: to splat g); only the `parts`
    named are written, `states` (one byte per record) with STATE.  ids must be strictly ascending.  records: a numpy array, or a
    torch tensor on the renderer's device (then ids and states are tensors on it too, int32 / uint8; no PCIe copy).  Returns how
    many splats were written."""
    o = _owner(r)
    written = ctypes.c_uint64()
    if hasattr(records, "data_ptr"):  # device tensors
        import torch
        rec = records.contiguous()
        if rec.dtype != torch.float32 or rec.numel() % 80:
            raise ValueError("write: records must be float32[m, 80]")
        m = rec.numel() // 80
        d_ids = d_st = None
        if ids is not None:
            if not hasattr(ids, "data_ptr"):  # (a host list: its uint32 words as the int32 tensor torch can hold)
                ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint32).ravel().view(np.int32).copy())
            d_ids = ids.to(rec.device).contiguous()
            if d_ids.dtype != torch.int32 or d_ids.numel() != m:
                raise ValueError("write: ids must be int32[m]")
        if states is not None:
            if not hasattr(states, "data_ptr"):
                states = torch.from_numpy(np.ascontiguousarray(states, dtype=np.uint8).ravel().copy())
            d_st = states.to(rec.device).contiguous()
            if d_st.dtype != torch.uint8 or d_st.numel() != m:
                raise ValueError("write: states must be uint8[m]")
        torch.cuda.current_stream(rec.device).synchronize()  # the inputs must be complete: the call reads them on the context's stream
        check(o._L.gs_write_splats_device(o._ctx, d_ids.data_ptr() if d_ids is not None and m else None, m, rec.data_ptr() if m else None,
                                          d_st.data_ptr() if d_st is not None and m else None, int(parts), ctypes.byref(written)))
    else:
        rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 80)
        m = rec.shape[0]
        h_ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).ravel()
        h_st = None if states is None else np.ascontiguousarray(states, dtype=np.uint8).ravel()
        if (h_ids is not None and h_ids.size != m) or (h_st is not None and h_st.size != m):
            raise ValueError("write: ids and states must have one entry per record")
        check(o._L.gs_write_splats(o._ctx, h_ids.ctypes.data if h_ids is not None and m else None, m, rec.ctypes.data if m else None,
                                   h_st.ctypes.data if h_st is not None and m else None, int(parts), ctypes.byref(written)))
    return int(written.value)


def take(r, mask=_SEL, value=_SEL, parts=RECORD):
    """gs_snapshot_take: a device-resident copy of the `parts` of the splats with (s & mask) == value (default: the selection;
    (0, 0): every splat, also without GS_FLAG_SPLAT_STATE); returns a Snapshot."""
    o = _owner(r)
    h = ctypes.c_void_p()
    check(o._L.gs_snapshot_take(o._ctx, int(mask), int(value), int(parts), ctypes.byref(h)))
    return Snapshot(r, h)


class Snapshot:
    """What take() returns.  restore() puts the parts back and can be applied again; swap() exchanges scene and snapshot, so a
    second swap redoes the edit.  A context manager that frees on exit; a freed snapshot raises ValueError."""

    def __init__(self, r, handle):
        self._r, self._h, self._L = r, handle, _abi.load()

    def _handle(self):
        if self._h is None:
            raise ValueError("the snapshot has been freed")
        return self._h

    def _apply(self, fn, parts):
        h = self._handle()
        o = _owner(self._r)
        moved = ctypes.c_uint64()
        check(fn(o._ctx, h, int(parts), ctypes.byref(moved)))
        return int(moved.value)

    def restore(self, parts=0):
        """gs_snapshot_restore: snapshot -> scene, `parts` of what was taken (0: all of it); returns how many splats that is."""
        return self._apply(self._L.gs_snapshot_restore, parts)

    def swap(self, parts=0):
        """gs_snapshot_swap: snapshot <-> scene in one pass; returns how many splats that is."""
        return self._apply(self._L.gs_snapshot_swap, parts)

    def info(self):
        """gs_snapshot_get_info: {"count", "n_at_take", "device_bytes", "parts", "dense"} (no GPU call)."""
        i = _abi.GsSnapshotInfo()
        check(self._L.gs_snapshot_get_info(self._handle(), ctypes.byref(i)))
        return {"count": int(i.count), "n_at_take": int(i.n_at_take), "device_bytes": int(i.device_bytes), "parts": int(i.parts),
                "dense": bool(i.dense)}

    def free(self):
        """gs_snapshot_free: releases the device memory; works after the renderer was destroyed, and twice."""
        if self._h is not None:
            h, self._h = self._h, None
            check(self._L.gs_snapshot_free(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- the editor's verbs --------------------------------------------------------------------------------------------------------------
_XFORM_PARTS = ((_abi.GS_XFORM_POSITION, POSITION), (_abi.GS_XFORM_ORIENT, GEOMETRY | SH), (_abi.GS_XFORM_SIZE, GEOMETRY))
_GRADE_PARTS = ((_abi.GS_GRADE_MATRIX, SH), (_abi.GS_GRADE_OFFSET, SH), (_abi.GS_GRADE_OPACITY, GEOMETRY))


def take_selected_for(r, xform_or_grade):
    """A snapshot of the selection holding exactly the parts the flags of a GsXform or a GsGrade name: POSITION -> POSITION,
    ORIENT -> GEOMETRY | SH, SIZE -> GEOMETRY; MATRIX, OFFSET -> SH, OPACITY -> GEOMETRY.  An undo that costs what the edit touches."""
    table = _GRADE_PARTS if isinstance(xform_or_grade, _abi.GsGrade) else _XFORM_PARTS
    parts = 0
    for flag, part in table:
        if xform_or_grade.flags & flag:
            parts |= part
    return take(r, _SEL, _SEL, parts)
