"""Moments: the exact mean and covariance of resident splats by VALUE (include/gsplat/gs_abi.h "moments").

Free functions over a ``Renderer`` or a ``PipelinedRenderer``, like gsplat.attributes.  The selections answer "which splats"; these
answer "where is the selection and how does it lie": the centroid as a pivot, the principal axes, an oriented box, the plane to
level a capture by.  The device adds integers and the host rounds once, so the sums do not depend on the order of anything and a
host restates them with ``fractions.Fraction``:

    S = sum(Fraction(float(v)) for v in values);  hi = float(S);  lo = float(S - Fraction(hi))

What is derived from the sums -- mean, variance, covariance -- is computed here in rational arithmetic from (hi, lo) and rounded to
float64 once, so it can be restated bit for bit as well.

    c = moments.centroid(r)                                   # of the selection, float64[3]
    r.rotate_selected(q, pivot=c)                             # one stray splat does not move this pivot (attributes.centre's does)
    moments.align_selected(r)                                 # principal axes onto x, y, z
"""
import ctypes
import math
from fractions import Fraction

import numpy as np

from . import _abi
from ._abi import check
from .attributes import SELECTED, _owner, attr, summary

_PROD = ((0, 1, 2), (1, 3, 4), (2, 4, 5))  # prod[] holds 00, 01, 02, 11, 12, 22
_XYZ = (_abi.GS_ATTR_POS_X, _abi.GS_ATTR_POS_Y, _abi.GS_ATTR_POS_Z)


def _result(out):
    pair = lambda e: (float(e.hi), float(e.lo))  # noqa: E731
    return {"matched": int(out.matched), "counted": int(out.counted), "sum": [pair(out.sum[j]) for j in range(3)],
            "prod": [[pair(out.prod[_PROD[j][k]]) for k in range(3)] for j in range(3)]}


def moments(r, attrs, where=(0, 0)):
    """gs_attr_moments of 1 .. 3 attributes (attributes.attr; the same kind may appear twice) over the splats with
    (s & where[0]) == where[1]: {"matched", "counted", "sum": [(hi, lo)] * 3, "prod": 3 x 3 symmetric table of (hi, lo)}.  counted:
    the matched splats whose values are all finite -- the others are in no sum.  sum[j] is the exact sum of attribute j's values,
    prod[j][k] of the products; hi is the float64 nearest to it (ties to even), lo the float64 nearest to what hi leaves.  Entries
    of an attribute that was not given are (0.0, 0.0)."""
    o = _owner(r)
    attrs = list(attrs)
    arr = (_abi.GsAttr * max(len(attrs), 1))(*attrs)
    out = _abi.GsAttrMoments()
    check(o._L.gs_attr_moments(o._ctx, arr, len(attrs), int(where[0]), int(where[1]), ctypes.byref(out)))
    return _result(out)


def host_moments(planes, state=None, where=(0, 0)):
    """gs_moments_host: the same record from 1 .. 3 host planes (float32[n] each) and an optional state plane (uint8[n]); no
    renderer, no GPU, the same arithmetic."""
    planes = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in planes]
    n = planes[0].size if planes else 0
    if any(p.size != n for p in planes):
        raise ValueError("host_moments: the planes differ in length")
    st = None
    if state is not None:
        st = np.ascontiguousarray(state, dtype=np.uint8).reshape(-1)
        if st.size != n:
            raise ValueError("host_moments: the state plane has %d entries for %d values" % (st.size, n))
    ptrs = (ctypes.c_void_p * max(len(planes), 1))(*[p.ctypes.data for p in planes])
    out = _abi.GsAttrMoments()
    check(_abi.load().gs_moments_host(ptrs, len(planes), n, None if st is None else st.ctypes.data, int(where[0]), int(where[1]),
                                      ctypes.byref(out)))
    return _result(out)


# ---- the rules: rational arithmetic on (hi, lo), one rounding to float64 -------------------------------------------------------------
def exact(pair):
    """Fraction(hi) + Fraction(lo): the sum as the record holds it."""
    return Fraction(pair[0]) + Fraction(pair[1])


def _counted(m, who, least=1):
    n = m["counted"]
    if n < least:
        raise ValueError("%s: %d matching splats with finite values, %d needed" % (who, n, least))
    return n


def mean_of(m, j=0):
    """RN(S_j / counted) of a moments() record."""
    return float(exact(m["sum"][j]) / _counted(m, "mean"))


def covariance_of(m, j=0, k=0):
    """RN((P_jk - S_j S_k / n) / n), n = counted: the population covariance (j == k: variance) of a moments() record."""
    n = _counted(m, "covariance")
    return float((exact(m["prod"][j][k]) - exact(m["sum"][j]) * exact(m["sum"][k]) / n) / n)


def mean(r, a, where=(0, 0)):
    """The mean of attribute a over the matching splats with a finite value: RN(S / counted), S = Fraction(hi) + Fraction(lo)."""
    return mean_of(moments(r, [a], where))


def variance(r, a, where=(0, 0)):
    """The population variance, RN((P - S^2 / n) / n) in rational arithmetic: no cancellation, never negative."""
    return covariance_of(moments(r, [a], where))


def std(r, a, where=(0, 0)):
    """math.sqrt of variance()."""
    return math.sqrt(variance(r, a, where))


def _xyz(r, where):
    return moments(r, [attr(k) for k in _XYZ], where)


def centroid(r, where=SELECTED):
    """float64[3]: the mean centre of the matching splats (default: the selection) whose three coordinates are finite.  Its
    float32 rounding is the pivot rotate_selected and scale_selected want; unlike attributes.centre, one stray splat moves it by
    1 / n of its distance only."""
    m = _xyz(r, where)
    return np.array([mean_of(m, j) for j in range(3)], dtype=np.float64)


def covariance(r, where=SELECTED):
    """float64[3, 3]: the population covariance of the matching splats' centres, from ONE device pass over (X, Y, Z); every entry
    by covariance_of's rule, symmetric by construction."""
    return _covariance(_xyz(r, where))


def _covariance(m):
    c = np.empty((3, 3), dtype=np.float64)
    for j in range(3):
        for k in range(j, 3):
            c[j, k] = c[k, j] = covariance_of(m, j, k)
    return c


def _axes(m, who):
    _counted(m, who, 3)
    w, v = np.linalg.eigh(_covariance(m))
    order = np.argsort(w)[::-1]
    w, axes = w[order], v[:, order].T.copy()
    for k in range(2):  # a sign convention: the component of largest magnitude is positive
        if axes[k, int(np.argmax(np.abs(axes[k])))] < 0:
            axes[k] = -axes[k]
    axes[2] = np.cross(axes[0], axes[1])  # right-handed
    return w, axes


def principal_axes(r, where=SELECTED):
    """(eigenvalues float64[3] in descending order, axes float64[3, 3]): the variances along the principal axes of the matching
    splats' centres and the axes as ROWS, unit length, right-handed (row 2 = row 0 x row 1).  numpy.linalg.eigh of covariance() on
    the host: the covariance is exact and restatable, the AXES ARE NOT bit-pinned -- they are what the installed LAPACK returns,
    and where two eigenvalues coincide any rotation of their plane is as good.  Fewer than 3 counted splats: ValueError."""
    return _axes(_xyz(r, where), "principal_axes")


def oriented_bounds(r, where=SELECTED):
    """The box along the principal axes that holds every matching centre: {"centre" float64[3], "axes" float32[3, 3] (rows),
    "half" float64[3], "planes": the three PLANE attributes, "lo" / "hi": float32[3]}.  Axis k's PLANE attribute is
    p = (axes[k], -(axes[k] . c)) in float32, c the centroid: its value is the signed distance from the centroid along the axis,
    and lo[k] / hi[k] are that value's exact minimum and maximum (attributes.summary), so every matching centre has
    lo[k] <= value <= hi[k] under the attribute's own f32 expression, with equality for one of them.  centre = c + sum of
    axes[k] (lo[k] + hi[k]) / 2, half[k] = (hi[k] - lo[k]) / 2.  Four device passes."""
    m = _xyz(r, where)
    _, axes = _axes(m, "oriented_bounds")
    c = np.array([mean_of(m, j) for j in range(3)], dtype=np.float64)
    axes32 = axes.astype(np.float32)
    planes, lo, hi = [], np.empty(3, np.float32), np.empty(3, np.float32)
    for k in range(3):
        d = np.float32(-float(np.dot(axes32[k].astype(np.float64), c)))
        planes.append(attr(_abi.GS_ATTR_PLANE, (axes32[k, 0], axes32[k, 1], axes32[k, 2], d)))
        s = summary(r, planes[k], where)
        lo[k], hi[k] = s["min"], s["max"]
    mid = (lo.astype(np.float64) + hi.astype(np.float64)) / 2
    return {"centre": c + mid @ axes32.astype(np.float64), "axes": axes32, "half": (hi.astype(np.float64) - lo.astype(np.float64)) / 2,
            "planes": planes, "lo": lo, "hi": hi}


def fit_plane(r, where=SELECTED):
    """(normal float64[3], offset, rms): the least-squares plane normal . p + offset = 0 through the matching centres -- the
    principal axis of least variance through the centroid -- and the root mean square distance from it, sqrt of the smallest
    eigenvalue."""
    m = _xyz(r, where)
    w, axes = _axes(m, "fit_plane")
    c = np.array([mean_of(m, j) for j in range(3)], dtype=np.float64)
    return axes[2], -float(np.dot(axes[2], c)), math.sqrt(max(float(w[2]), 0.0))


def _quaternion(R):
    """(r, x, y, z) of a rotation matrix (Shepperd's method: the largest of the four squares first)."""
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = (s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s)
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        v = [0.0, 0.0, 0.0]
        v[i], v[j], v[k] = s / 4, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
        q = ((R[k, j] - R[j, k]) / s, v[0], v[1], v[2])
    return tuple(float(x) for x in q)


def align_xform(r, where=SELECTED):
    """The GsXform (_abi.compose_xform) that rotates the principal axes of the matching centres onto x, y, z about their centroid:
    p' = A (p - c) + c, A the axes as rows."""
    m = _xyz(r, where)
    _, axes = _axes(m, "align_xform")
    c = [mean_of(m, j) for j in range(3)]
    return _abi.compose_xform(rot=_quaternion(axes), pivot=c)


def align_selected(r):
    """Applies align_xform to the selection; returns how many splats moved."""
    return _owner(r).transform(align_xform(r, SELECTED))
