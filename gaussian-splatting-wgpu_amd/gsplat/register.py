"""Registration: align a selection onto its nearest neighbours (include/gsplat/gs_abi.h "registration").

Free functions over a ``Renderer`` or a ``PipelinedRenderer``, like gsplat.nearest.  ``gsplat.insert`` puts a second capture behind
the resident one and leaves it selected; two captures of one place never share a frame, and this brings the new one onto the old
one without the export / host k-d tree / numpy / re-upload route -- the frame, the state plane and every per-splat plane stay:

    insert.merge_ply(r, "second.ply")                          # the new capture is the selection
    r.translate_selected(t); r.rotate_selected(q, pivot=c)      # a ROUGH placement by hand (or moments.align_xform)
    snap = snapshots.take(r)                                    # undo: gsplat.snapshots
    steps = register.align(r)                                   # point-to-point ICP: selected splats onto the unselected ones

WHAT ICP NEEDS FROM ITS CALLER: a rough pre-alignment.  Every step pairs each moving splat with its nearest fixed splat within
``radius`` and fits the pairs; it converges to the right pose only when most of those nearest splats are already the right ones,
that is when the moving capture lies within about the radius of where it belongs and is turned by a few degrees, not by ninety.
The alignment moves splats in place and is not its own undo: take a snapshot (``gsplat.snapshots``) first.

A step is restatable: the nearest ids are gsplat.nearest's, the 21 pair sums (pair_moments) are exact -- the device adds integers,
the host rounds once, so a host restates them with ``fractions.Fraction`` --, the centroids, the cross-covariance, the spreads and
the rms are formed from them in rational arithmetic and rounded once, and the transform is gs_transform_splats'.  Only the
rotation is what the installed LAPACK's SVD returns and is not bit-pinned, as for moments.principal_axes.
"""
import ctypes
import math
from fractions import Fraction

import numpy as np

from . import _abi, nearest
from ._abi import check
from .attributes import SELECTED
from .moments import _quaternion, exact
from .neighbours import _owner

UNSELECTED = (_abi.GS_SPLAT_SELECTED, 0)


def _dist2(max_dist):
    """max_dist rounded to f32 and squared as ONE f32 product, like a radius."""
    d = np.float32(max_dist)
    with np.errstate(all="ignore"):
        return float(d * d)


def _result(out):
    pair = lambda e: (float(e.hi), float(e.lo))  # noqa: E731
    return {"matched": int(out.matched), "paired": int(out.paired), "sum_p": [pair(out.sum_p[a]) for a in range(3)],
            "sum_q": [pair(out.sum_q[a]) for a in range(3)], "pq": [[pair(out.pq[3 * a + b]) for b in range(3)] for a in range(3)],
            "pp": [pair(out.pp[a]) for a in range(3)], "qq": [pair(out.qq[a]) for a in range(3)]}


def pair_moments(r, where=SELECTED, max_dist=math.inf, partner=None):
    """gs_pair_moments over the splats i with (s & where[0]) == where[1] and their partners j = partner[i] (uint32[N] on the host;
    None: the nearest plane of the last nearest.search on r): {"matched", "paired", "sum_p", "sum_q": [(hi, lo)] * 3, "pq": 3 x 3
    table of (hi, lo), "pp", "qq": [(hi, lo)] * 3}.  paired: the matched splats with j < N, six finite coordinates and a squared
    distance to the partner <= f32(max_dist)^2 on the positions as they are now; only they are in the sums.  sum_p[a] / sum_q[a]:
    the exact sums of p_a and q_a = (p_j)_a, pq[a][b] of p_a q_b, pp[a] / qq[a] of the squares; (hi, lo) as in moments.moments."""
    o = _owner(r)
    ids = None
    if partner is not None:
        ids = np.ascontiguousarray(partner, dtype=np.uint32).reshape(-1)
        if ids.size != o.numGaussians:
            raise ValueError("pair_moments: the partner plane has %d entries for %d splats" % (ids.size, o.numGaussians))
    out = _abi.GsPairMoments()
    check(o._L.gs_pair_moments(o._ctx, int(where[0]), int(where[1]), ids.ctypes.data if ids is not None and ids.size else None, _dist2(max_dist),
                               ctypes.byref(out)))
    return _result(out)


def host_pair_moments(pos, partner, state=None, where=(0, 0), max_dist=math.inf):
    """gs_pair_moments_host: the same record from host positions (float32[n, 3] or records [n, 80]), a partner plane (uint32[n])
    and an optional state plane (uint8[n]); no renderer, no GPU, the same arithmetic."""
    p = np.asarray(pos, dtype=np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)
    planes = [np.ascontiguousarray(p[:, a]) for a in range(3)]
    n = p.shape[0]
    ids = np.ascontiguousarray(partner, dtype=np.uint32).reshape(-1)
    if ids.size != n:
        raise ValueError("host_pair_moments: the partner plane has %d entries for %d positions" % (ids.size, n))
    st = None
    if state is not None:
        st = np.ascontiguousarray(state, dtype=np.uint8).reshape(-1)
        if st.size != n:
            raise ValueError("host_pair_moments: the state plane has %d entries for %d positions" % (st.size, n))
    out = _abi.GsPairMoments()
    ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    check(_abi.load().gs_pair_moments_host(ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), n, ptr(ids), None if st is None else ptr(st),
                                           int(where[0]), int(where[1]), _dist2(max_dist), ctypes.byref(out)))
    return _result(out)


def fit(m, scale=False):
    """The least-squares map of p onto q over the pairs of a pair_moments() record: the rotation R, scale s and translation that
    minimise sum |s R (p - pbar) + qbar - q|^2 (Kabsch; with scale=True Umeyama's s, else s = 1).

    With n = paired and the sums S as the record holds them (Fraction(hi) + Fraction(lo)), in rational arithmetic, each number
    rounded ONCE to float64 -- covariance_of's rule, so a centroid far from the origin costs no digits:
        pbar_a = S_p[a] / n,  qbar_a = S_q[a] / n,  translate_a = (S_q[a] - S_p[a]) / n
        M_ab = S_pq[a][b] - S_p[a] S_q[b] / n                     (the centred cross-covariance, not divided by n)
        spread_p = sum_a (S_pp[a] - S_p[a]^2 / n),  spread_q likewise
        ssd = sum_a (S_pp[a] + S_qq[a] - 2 S_pq[a][a])             (= sum |p - q|^2);  rms = sqrt(ssd / n) in float64
    Then U, D, Vt = numpy.linalg.svd(M), d = sign(det(Vt^T U^T)), R = Vt^T diag(1, 1, d) U^T (det R = +1, never a reflection) and
    s = (D0 + D1 + d D2) / spread_p.  R is what the installed LAPACK returns and is not bit-pinned; everything before it is.
    Returns {"rot": (r, x, y, z), "R", "scale", "pivot": pbar, "translate": qbar - pbar, "paired", "rms", "M", "spread_p",
    "spread_q", "singular"}.  Fewer than 3 pairs, or a second singular value <= 1e-12 x the first (the pairs lie on a line: the
    rotation about it is free): ValueError."""
    n = int(m["paired"])
    if n < 3:
        raise ValueError("fit: %d pairs, 3 needed" % n)
    sp, sq = [exact(v) for v in m["sum_p"]], [exact(v) for v in m["sum_q"]]
    pq = [[exact(m["pq"][a][b]) for b in range(3)] for a in range(3)]
    pp, qq = [exact(v) for v in m["pp"]], [exact(v) for v in m["qq"]]
    pbar = np.array([float(sp[a] / n) for a in range(3)], dtype=np.float64)
    translate = np.array([float((sq[a] - sp[a]) / n) for a in range(3)], dtype=np.float64)
    M = np.array([[float(pq[a][b] - sp[a] * sq[b] / n) for b in range(3)] for a in range(3)], dtype=np.float64)
    spread_p = float(sum((pp[a] - sp[a] * sp[a] / n for a in range(3)), Fraction(0)))
    spread_q = float(sum((qq[a] - sq[a] * sq[a] / n for a in range(3)), Fraction(0)))
    ssd = float(sum((pp[a] + qq[a] - 2 * pq[a][a] for a in range(3)), Fraction(0)))
    U, D, Vt = np.linalg.svd(M)
    if not D[1] > 1e-12 * D[0]:
        raise ValueError("fit: the pairs lie on a line (singular values %g, %g, %g): the rotation is not determined" % tuple(D))
    d = 1.0 if np.linalg.det(Vt.T @ U.T) > 0 else -1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    s = float((D[0] + D[1] + d * D[2]) / spread_p) if scale else 1.0
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError("fit: the scale %g is not a finite positive number" % s)
    return {"rot": _quaternion(R), "R": R, "scale": s, "pivot": pbar, "translate": translate, "paired": n, "rms": math.sqrt(ssd / n), "M": M,
            "spread_p": spread_p, "spread_q": spread_q, "singular": D}


def xform_of(f):
    """The GsXform of a fit: _abi.compose_xform(rot, translate, scale, pivot), p' = s R (p - pbar) + pbar + (qbar - pbar)."""
    return _abi.compose_xform(rot=f["rot"], translate=f["translate"], scale=f["scale"], pivot=f["pivot"])


def step(r, radius, moving=SELECTED, fixed=UNSELECTED, max_dist=None, scale=False):
    """One ICP step: nearest.search(k=1, query=moving, source=fixed) at `radius`, pair_moments over `moving` with max_dist (None:
    the radius), fit, and the fit's transform applied to `moving` in place.  Returns the fit with "search" (the search's info),
    "radius", "max_dist" and "moved" (the splats transformed); "rms" is that of the pairs BEFORE the move.  A ValueError from fit
    (too few pairs, a degenerate cloud) is raised before anything moves.  The nearest plane is left as the step's search wrote it:
    it describes the positions before the move."""
    o = _owner(r)
    info = nearest.search(o, 1, radius, source=fixed, query=moving)
    md = float(radius) if max_dist is None else float(max_dist)
    f = fit(pair_moments(o, moving, md), scale)
    f["moved"] = o.transform(xform_of(f), int(moving[0]), int(moving[1]))
    f["search"], f["radius"], f["max_dist"] = info, float(radius), md
    return f


def align(r, radius=None, moving=SELECTED, fixed=UNSELECTED, max_iters=30, tol=1e-6, trim=3.0, scale=False):
    """Point-to-point ICP: repeats step() on the splats that pass `moving` (default: the selection) against those that pass `fixed`
    (default: the unselected ones).  radius=None: eight times the median of sqrt(dist2) of nearest.distances(r, 1, where=fixed), the
    fixed capture's own spacing.  From the second step on max_dist = min(radius, trim x the previous step's rms), which drops the
    pairs that the overlap does not cover.  Stops when |rms - previous rms| <= tol x previous rms, when a fit raises ValueError (that
    step moves nothing), or after max_iters steps.  Returns the list of step records.

    The caller provides a rough pre-alignment within the radius (see the module's text); gsplat.snapshots gives the undo."""
    o = _owner(r)
    if radius is None:
        nearest.distances(o, 1, where=fixed)
        d2, _ = nearest.read(o)
        d = np.sqrt(d2[np.isfinite(d2)].astype(np.float64))
        if not d.size:
            raise ValueError("align: no fixed splat has a nearest fixed splat, give a radius")
        radius = 8.0 * float(np.median(d))
    radius = float(radius)
    steps, prev = [], None
    for _ in range(int(max_iters)):
        md = radius if prev is None else min(radius, float(trim) * prev)
        try:
            rec = step(o, radius, moving, fixed, max_dist=md, scale=scale)
        except ValueError:
            break
        steps.append(rec)
        if prev is not None and abs(rec["rms"] - prev) <= float(tol) * prev:
            break
        prev = rec["rms"]
    return steps
