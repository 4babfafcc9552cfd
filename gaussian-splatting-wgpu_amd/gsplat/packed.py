"""Packed scenes: save, load and append the 16-byte chunked splat format (include/gsplat/gs_abi.h "packed scenes").

The float .ply is 248 bytes per splat at SH degree 3; the packed file keeps position, rotation, log-scale and colour in four 32-bit
words per splat, quantised against the bounds of its chunk of 256 splats, plus one byte per higher SH coefficient: 16 bytes per
splat at degree 0, 61 at degree 3.  The files carry the line ``comment gsplat-packed 1`` and only files with it are read: no
interoperability with third-party files is claimed.

Free functions over a ``Renderer`` or a ``PipelinedRenderer`` (whose splats live with its first member), like ``gsplat.insert``:

    packed.save(r, "scene.packed.ply")                      # every resident splat, degree 3, along a Morton curve
    packed.save(r, "chair.packed.ply", SEL, SEL, order="index")
    packed.upload(r, "scene.packed.ply")                    # replaces the scene, decoded on the device
    packed.append(r, "chair.packed.ply", state=SEL)         # behind the resident splats, like insert.append_ply

``save`` encodes on the device and streams the file out through two pinned buffers, ``upload`` and ``append`` read it in trips of
whole chunks and decode on the device: the host never holds the scene.  ``order="morton"`` sorts the selection along a Morton curve
through its bounds first, so that the 256 splats of a chunk are neighbours and their bounds tight; ``"index"`` keeps ascending index
order.  The host-side functions (``encode``, ``decode``, ``save_records``, ``load_records``, ``logit_table``) need no GPU.
"""
import ctypes

import numpy as np

from . import _abi
from ._abi import check
from .insert import _grown
from .neighbours import _owner

ORDERS = {"index": _abi.GS_PACK_ORDER_INDEX, "morton": _abi.GS_PACK_ORDER_MORTON}


def rest_count(sh_degree):
    """K: the SH coefficients above band 0 per channel at that degree."""
    return (int(sh_degree) + 1) ** 2 - 1


# ---- resident scenes -------------------------------------------------------------------------------------------------------------------
def save(r, path, mask=0, value=0, sh_degree=3, order="morton", with_ids=False):
    """gs_export_packed: writes the resident splats with (s & mask) == value ((0, 0): every splat, also without
    GS_FLAG_SPLAT_STATE) to a packed file; returns {"count", "chunks", "file_bytes", "nonfinite"}, and with_ids (info, uint32[count]
    ids): record g of the file is splat ids[g].  nonfinite: the floats that had to be replaced by 0 because they were not finite.
    The scene is not changed."""
    o = _owner(r)
    info = _abi.GsPackInfo()
    ids = np.empty(max(int(o.numGaussians), 1), dtype=np.uint32) if with_ids else None
    check(o._L.gs_export_packed(o._ctx, str(path).encode(), int(mask), int(value), int(sh_degree), ORDERS[order], ctypes.byref(info),
                                ids.ctypes.data if with_ids else None))
    out = {"count": int(info.count), "chunks": int(info.chunks), "file_bytes": int(info.file_bytes), "nonfinite": int(info.nonfinite)}
    return (out, ids[:out["count"]].copy()) if with_ids else out


def upload(r, path):
    """gs_upload_packed: replaces the resident splats by the file's, decoded on the device (no host copy of its records); returns
    how many there are.  Like every upload, taps and pick need a new frame afterwards."""
    o = _owner(r)
    n = ctypes.c_uint64()
    check(o._L.gs_upload_packed(o._ctx, str(path).encode(), ctypes.byref(n)))
    o.numGaussians = int(n.value)
    for b in getattr(r, "renderers", [o])[1:]:
        check(b._L.gs_share_splats(b._ctx, o._ctx))
        b.numGaussians = o.numGaussians
    return o.numGaussians


def append(r, path, state=0):
    """gs_append_packed: streams a packed file behind the resident splats with the state byte `state`, like insert.append_ply;
    returns (first, count)."""
    o = _owner(r)
    first, m = ctypes.c_uint64(), ctypes.c_uint64()
    check(o._L.gs_append_packed(o._ctx, str(path).encode(), int(state), ctypes.byref(first), ctypes.byref(m)))
    return _grown(r, o, int(first.value), int(m.value))


# ---- the host codec (no GPU) -----------------------------------------------------------------------------------------------------------
def encode(records, sh_degree=3):
    """gs_pack_encode: float32[n, 80] records in the given order -> (chunks float32[ceil(n / 256), 18], vertices uint32[n, 4],
    sh uint8[n, 3 K], nonfinite)."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 80)
    n, K = rec.shape[0], rest_count(sh_degree)
    chunks = np.zeros(((n + 255) // 256, 18), np.float32)
    vertices = np.zeros((n, 4), np.uint32)
    sh = np.zeros((n, 3 * K), np.uint8)
    bad = ctypes.c_uint64()
    check(_abi.load().gs_pack_encode(rec.ctypes.data if n else None, n, int(sh_degree), chunks.ctypes.data if n else None,
                                     vertices.ctypes.data if n else None, sh.ctypes.data if n and K else None, ctypes.byref(bad)))
    return chunks, vertices, sh, int(bad.value)


def decode(chunks, vertices, sh, sh_degree=3):
    """gs_pack_decode: the inverse of encode, to float32[n, 80] records (the coefficients above sh_degree and the padding are 0)."""
    vertices = np.ascontiguousarray(vertices, dtype=np.uint32).reshape(-1, 4)
    n, K = vertices.shape[0], rest_count(sh_degree)
    chunks = np.ascontiguousarray(chunks, dtype=np.float32).reshape(-1, 18)
    sh = np.ascontiguousarray(sh, dtype=np.uint8).reshape(n, 3 * K)
    if chunks.shape[0] != (n + 255) // 256:
        raise ValueError("decode: %d chunk records for %d vertices" % (chunks.shape[0], n))
    rec = np.zeros((n, 80), np.float32)
    check(_abi.load().gs_pack_decode(chunks.ctypes.data if n else None, vertices.ctypes.data if n else None, sh.ctypes.data if n and K else None,
                                     n, int(sh_degree), rec.ctypes.data if n else None))
    return rec


def save_records(path, records, sh_degree=3):
    """gs_pack_save: float32[n, 80] records -> a packed file, in the given order."""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 80)
    check(_abi.load().gs_pack_save(str(path).encode(), rec.ctypes.data if rec.shape[0] else None, rec.shape[0], int(sh_degree)))


def load_records(path):
    """gs_pack_load: a packed file -> (records float32[n, 80], sh_degree)."""
    L = _abi.load()
    rec, n, deg = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int32()
    check(L.gs_pack_load(str(path).encode(), ctypes.byref(rec), ctypes.byref(n), ctypes.byref(deg)))
    try:
        arr = np.ctypeslib.as_array(ctypes.cast(rec, ctypes.POINTER(ctypes.c_float)), shape=(max(n.value, 1) * 80,))[: n.value * 80]
        return arr.reshape(n.value, 80).copy(), deg.value
    finally:
        L.gs_ply_free(rec)


def logit_table():
    """gs_pack_logit_table: the 256 opacity logits a decoder reads the alpha byte through, float32[256]."""
    t = np.zeros(256, np.float32)
    check(_abi.load().gs_pack_logit_table(t.ctypes.data))
    return t
