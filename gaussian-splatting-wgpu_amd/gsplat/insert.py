"""Splat insertion: append records, a .ply or a copy of a selection to the resident splats (include/gsplat/gs_abi.h "splat insertion").

Free functions over a ``Renderer`` or a ``PipelinedRenderer`` (whose splats live with its first member: every slot is drained, that
member is asked, and the other members then borrow the new scene again, as after ``compact``), like ``gsplat.colours``.  Every other
call on the resident splats selects, hides, deletes, moves, recolours or saves them; these ADD some, where an upload would replace
the scene -- what would otherwise take export_splats of everything (320 bytes per splat), a host concatenation and a re-upload,
and for a scene streamed in from a .ply the only host copy of it there would ever be:

    insert.merge_ply(r, "second_capture.ply")              # the new capture arrives selected ...
    r.rotate_selected(q); r.translate_selected(t)          # ... is straightened and moved into place ...
    colours.brighten(r, 1.2); colours.saturate(r, 0.8)     # ... and graded to match the first
    r.select_box(lo, hi); insert.duplicate_selected(r, _abi.compose_xform(translate=(2, 0, 0)))   # a second copy of the chair

The old splats keep their indices, records and state bytes; the new ones take the indices first .. first + count - 1 in the order
given (a duplicate: ascending source index) and all get the one byte `state`.  Afterwards the renderer is in the state of a fresh
one given the concatenated records and state plane: like an upload or a compaction, taps and pick need a new frame, and the
coverage, neighbour-count and cluster planes read as their initial values.  count == 0 changes nothing.  A call costs O(N): it
builds the new scene beside the old one (and leaves the old one in place if anything fails on the way).  Multi-GPU: make the same
call on every rank.
"""
import ctypes

import numpy as np

from . import _abi
from ._abi import check
from .neighbours import _owner

_SEL = _abi.GS_SPLAT_SELECTED


def _grown(r, o, first, count):
    """The bookkeeping every insertion shares: numGaussians, and for a PipelinedRenderer the members that borrow the owner's
    scene share it again (an insertion counts as a re-upload for them)."""
    o.numGaussians = first + count
    if count:
        for b in getattr(r, "renderers", [o])[1:]:
            check(b._L.gs_share_splats(b._ctx, o._ctx))
            b.numGaussians = o.numGaussians
    return first, count


def append(r, records, state=0):
    """gs_append_splats[_device]: appends float32[m, 80] records (what PackedGaussians and the uploads take) -- a numpy array, or a
    torch tensor on the renderer's device (no PCIe copy) -- with the state byte `state`; returns (first, count)."""
    o = _owner(r)
    first = ctypes.c_uint64()
    if hasattr(records, "data_ptr"):  # a device tensor
        import torch
        rec = records.contiguous()
        if rec.dtype != torch.float32 or rec.numel() % 80:
            raise ValueError("append: records must be float32[m, 80]")
        m = rec.numel() // 80
        torch.cuda.current_stream(rec.device).synchronize()  # the records must be complete: the call reads them on the context's stream
        check(o._L.gs_append_splats_device(o._ctx, rec.data_ptr() if m else None, m, int(state), ctypes.byref(first)))
    else:
        rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 80)
        m = rec.shape[0]
        check(o._L.gs_append_splats(o._ctx, rec.ctypes.data if m else None, m, int(state), ctypes.byref(first)))
    return _grown(r, o, int(first.value), m)


def append_ply(r, path, state=0):
    """gs_append_ply: streams a 3DGS .ply behind the resident splats (no host copy of its records); returns (first, count)."""
    o = _owner(r)
    first, m = ctypes.c_uint64(), ctypes.c_uint64()
    check(o._L.gs_append_ply(o._ctx, str(path).encode(), int(state), ctypes.byref(first), ctypes.byref(m)))
    return _grown(r, o, int(first.value), int(m.value))


def duplicate(r, mask, value, state=0):
    """gs_duplicate_splats: appends a copy of every splat with (s & mask) == value ((0, 0): every splat, also without
    GS_FLAG_SPLAT_STATE) with the state byte `state`; returns (first, count, ids): ids[j] is the source of splat first + j."""
    o = _owner(r)
    st = _abi.GsStats()
    check(o._L.gs_get_stats(o._ctx, ctypes.byref(st)))  # N before the call: the capacity gs_duplicate_splats expects of ids
    ids = np.empty(max(int(st.num_gaussians), 1), dtype=np.uint32)
    first, m = ctypes.c_uint64(), ctypes.c_uint64()
    check(o._L.gs_duplicate_splats(o._ctx, int(mask), int(value), int(state), ctypes.byref(first), ctypes.byref(m), ids.ctypes.data))
    return _grown(r, o, int(first.value), int(m.value)) + (ids[:int(m.value)].copy(),)


# ---- the editor's verbs --------------------------------------------------------------------------------------------------------------
def merge_ply(r, path):
    """Clears the selection and appends the file SELECTED: the new capture is what translate_selected / rotate_selected /
    colours.* then act on.  Returns (first, count)."""
    _owner(r).clear_selection()
    return append_ply(r, path, _SEL)


def duplicate_selected(r, xform=None):
    """Copies the selection: the copies end up selected, the originals deselected (their other bits untouched); with `xform`
    (_abi.compose_xform) the copies are transformed too.  Returns (first, count)."""
    o = _owner(r)
    originals = o.list_state(_SEL, _SEL)
    first, count, _ = duplicate(r, _SEL, _SEL, _SEL)
    o.state_ids(originals, _abi.GS_STATE_CLEAR, _SEL)
    if xform is not None and count:
        o.transform(xform)
    return first, count
