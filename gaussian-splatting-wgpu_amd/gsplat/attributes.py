"""Splat attributes: summarise, histogram, read and select resident splats by VALUE (include/gsplat/gs_abi.h "splat attributes").

Free functions over a ``Renderer`` or a ``PipelinedRenderer`` (whose splats, state plane and coverage planes live with its first
member: every slot is drained, then that member is asked).  An attribute is one f32 per resident splat -- a position coordinate,
the opacity logit, the smallest / largest / summed log-scale, the anisotropy, a base colour channel, the squared distance from a
point, the signed distance from a plane, or one of the coverage planes' numbers -- defined so that a host can restate it bit for
bit.  The calls answer on the device what would otherwise take export_splats, numpy and state_ids: 24 bytes, a histogram or 4 bytes
per match come back instead of 320 bytes per splat.

    a = attributes.attr(_abi.GS_ATTR_OPACITY_LOGIT)
    t = attributes.quantile(r, a, 0.05)                       # the logit below which the faintest 5 % lie
    attributes.select(r, a, -np.inf, t)                       # select them ...
    r.hide_selected()                                         # ... and hide them
    r.rotate_selected(q, pivot=attributes.centre(r))          # rotate the selection about its own centre
"""
import ctypes
import math

import numpy as np

from . import _abi
from ._abi import check

SELECTED = (_abi.GS_SPLAT_SELECTED, _abi.GS_SPLAT_SELECTED)
# quantile(): the value returned lies within this fraction of (max - min) of the order statistic it names (see there)
QUANTILE_RESOLUTION = 1.0 / 65536.0


def _owner(r):
    """The renderer that holds the splats: a PipelinedRenderer's state owner (its slots drained first), or r itself."""
    return r._state_owner() if hasattr(r, "_state_owner") else r


def attr(kind, p=(0, 0, 0, 0)):
    """A GsAttr: kind = _abi.GS_ATTR_*; p: the point of DIST2 (p[0..2]) or the plane of PLANE (p . (x, y, z, 1)); ignored by the
    other kinds."""
    a = _abi.GsAttr()
    a.struct_size, a.kind = ctypes.sizeof(_abi.GsAttr), int(kind)
    p = [float(v) for v in p] + [0.0] * (4 - len(p))
    a.p[:] = p[:4]
    return a


def depth_attr(uniforms):
    """PLANE with row 2 of the camera's view matrix: the value is the projection's depth pv.z of the splat's centre."""
    u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(40)
    return attr(_abi.GS_ATTR_PLANE, (u[2], u[6], u[10], u[14]))


def summary(r, a, where=(0, 0)):
    """gs_attr_summary: {"matched", "nan", "min", "max"} over the splats with (s & where[0]) == where[1]; min / max (np.float32) over
    the values that are not NaN, in the total order that puts -0 below +0; (+inf, -inf) when there is none.  There is no mean: a
    float sum depends on the order of the adds (an exact one, which does not, is moments.mean)."""
    o = _owner(r)
    out = _abi.GsAttrSummary()
    check(o._L.gs_attr_summary(o._ctx, ctypes.byref(a), int(where[0]), int(where[1]), ctypes.byref(out)))
    return {"matched": int(out.matched), "nan": int(out.nan), "min": np.float32(out.min), "max": np.float32(out.max)}


def histogram(r, a, lo, hi, bins=256, where=(0, 0)):
    """gs_attr_histogram: (counts uint64[bins], below, above, nan).  A value v of a matching splat goes to the NaN count if it is
    one, below if v < lo, above if v >= hi, else to bin min((uint32)((v - lo) * scale), bins - 1), scale = f32(bins) / (hi - lo)
    in f32.  The four add up to summary()["matched"]."""
    o = _owner(r)
    bins = int(bins)
    c = np.zeros(max(bins, 0) + 3, dtype=np.uint64)
    check(o._L.gs_attr_histogram(o._ctx, ctypes.byref(a), int(where[0]), int(where[1]), float(lo), float(hi), bins, c.ctypes.data))
    return c[:bins].copy(), int(c[bins]), int(c[bins + 1]), int(c[bins + 2])


def values(r, a, where=(0, 0), with_ids=False):
    """gs_attr_read: float32[n], the values of the matching splats in ascending index order; with_ids: (values, uint32[n] indices)."""
    o = _owner(r)
    m, v = int(where[0]), int(where[1])
    n = ctypes.c_uint64()
    check(o._L.gs_attr_read(o._ctx, ctypes.byref(a), m, v, None, 0, ctypes.byref(n), None))
    out = np.empty(n.value, dtype=np.float32)
    ids = np.empty(n.value, dtype=np.uint32) if with_ids else None
    if n.value:
        check(o._L.gs_attr_read(o._ctx, ctypes.byref(a), m, v, out.ctypes.data, out.size, ctypes.byref(n), ids.ctypes.data if with_ids else None))
    return (out, ids) if with_ids else out


def select(r, a, lo, hi, inside=True, op=_abi.GS_STATE_SET, bits=_abi.GS_SPLAT_SELECTED, where=(0, 0)):
    """gs_state_attr: applies `op` (GS_STATE_*) with `bits` to the splats that pass `where` and for which (lo <= v <= hi) == inside;
    returns how many those are.  A NaN value is in no range, so select(r, a, -inf, inf, inside=False) finds the broken splats.
    Infinite bounds are fine, lo > hi is the empty range."""
    o = _owner(r)
    matched = ctypes.c_uint64()
    check(o._L.gs_state_attr(o._ctx, ctypes.byref(a), float(lo), float(hi), 1 if inside else 0, int(where[0]), int(where[1]), int(op), int(bits),
                             ctypes.byref(matched)))
    return int(matched.value)


# ---- the editor's verbs ------------------------------------------------------------------------------------------------------------
def bounds(r, where=SELECTED):
    """(lo float32[3], hi float32[3], matched): the axis-aligned bounds of the matching splats' centres (default: the selection),
    three summaries.  Centres with a NaN coordinate are left out of that axis; no centre at all gives (+inf, -inf)."""
    s = [summary(r, attr(k), where) for k in (_abi.GS_ATTR_POS_X, _abi.GS_ATTR_POS_Y, _abi.GS_ATTR_POS_Z)]
    return (np.array([t["min"] for t in s], np.float32), np.array([t["max"] for t in s], np.float32), s[0]["matched"])


def centre(r, where=SELECTED):
    """The midpoint of bounds(), float32[3] as lo + (hi - lo) / 2 in f32: the pivot rotate_selected and scale_selected want."""
    lo, hi, matched = bounds(r, where)
    if not matched or not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("centre: no matching splat with a finite centre")
    return lo + (hi - lo) / np.float32(2)


def quantile(r, a, q, where=(0, 0)):
    """The value below which the fraction q of the matching splats' values lie, without reading them: a summary for the range, a
    256-bin histogram over it, and a second one over the bin that holds the order statistic k = floor(q (m - 1)) of the m values
    that are not NaN (numpy's method="lower").  Returns the middle of that second bin as np.float32: it lies within
    QUANTILE_RESOLUTION (max - min), i.e. 1/65536 of the range, of the k-th smallest value (plus the value's own f32 spacing when
    the range is only a few spacings wide).  Infinite values make the range infinite and are refused: filter them away first."""
    if not 0.0 <= q <= 1.0:
        raise ValueError("quantile: q must be in [0, 1]")
    s = summary(r, a, where)
    m = s["matched"] - s["nan"]
    if m == 0:
        raise ValueError("quantile: no matching splat has a value")
    lo, top = s["min"], s["max"]
    hi = np.nextafter(top, np.float32(np.inf))  # the histogram's range is half open: the largest value stays inside
    if not (np.isfinite(lo) and np.isfinite(hi) and np.isfinite(np.float32(hi - lo))):
        raise ValueError("quantile: the values are not in a finite range [%g, %g]" % (lo, top))
    if lo == top:
        return np.float32(lo)
    k = int(math.floor(q * (m - 1)))

    def locate(e0, e1, k):
        """(the bin that holds order statistic k among the 256 over [e0, e1), the bins' width), or None when k is outside the range."""
        counts, below, above, _ = histogram(r, a, e0, e1, 256, where)
        k -= below
        if k < 0 or k >= int(counts.sum()):
            return None
        b = int(np.searchsorted(np.cumsum(counts), k, side="right"))
        return b, (float(e1) - float(e0)) / 256.0

    b, w = locate(lo, hi, k)  # (every value is inside: never None)
    mid = float(lo) + (b + 0.5) * w
    # the second round: the bin, a 64th of its width wider on either side (the bin's edges in f32 are not exactly lo + b w)
    e0 = max(lo, np.float32(float(lo) + b * w - w / 64.0))
    e1 = min(hi, np.float32(float(lo) + (b + 1) * w + w / 64.0))
    if e0 < e1 and np.isfinite(np.float32(e1 - e0)):
        fine = locate(e0, e1, k)
        if fine is not None:
            mid = float(e0) + (fine[0] + 0.5) * fine[1]
    return np.float32(min(max(mid, float(lo)), float(top)))
