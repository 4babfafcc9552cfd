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

POINT-TO-PLANE.  Captures are mostly walls, floors and table tops sampled at different places, so the tangential part of every pair
is sampling noise: the point metric creeps along surfaces and stalls at a pose biased by the sampling.  metric="plane" penalises only
the distance of a moving splat to the tangent plane of its partner:

    steps = register.align(r, metric="plane")                   # surface.estimate over the fixed splats once, then plane_step()s

pair_plane_moments gives the 29 exact sums of the normal equations, fit_plane solves them in rational arithmetic -- no SVD: every
number of a plane step is pinned --, plane_step is one step on normals the caller estimated.
"""
import ctypes
import math
from fractions import Fraction

import numpy as np

from . import _abi, moments, nearest, surface
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


def align(r, radius=None, moving=SELECTED, fixed=UNSELECTED, max_iters=30, tol=1e-6, trim=3.0, scale=False, metric="point", damping=0.0,
          normal_radius=None):
    """ICP: repeats step() (metric="point", the default) or plane_step() (metric="plane") on the splats that pass `moving` (default:
    the selection) against those that pass `fixed` (default: the unselected ones).  radius=None: eight times the median of sqrt(dist2)
    of nearest.distances(r, 1, where=fixed), the fixed capture's own spacing.  From the second step on max_dist = min(radius, trim x
    the previous step's rms), which drops the pairs that the overlap does not cover.  Stops when |rms - previous rms| <= tol x previous
    rms, when a fit raises ValueError (that step moves nothing), or after max_iters steps.  Returns the list of step records.

    metric="plane": point-to-plane.  surface.estimate(query=fixed, source=fixed) runs ONCE, at normal_radius (None:
    surface.radius_for(r, 30, where=fixed), the median distance to the 30th nearest fixed splat: a ball that holds about 30
    neighbours) -- the fixed splats do not move.  The trim uses the POINT rms of the pairs ("rms", from the d2 sum); the stop is on
    the relative change of "rms_plane".  damping: fit_plane's; scale is not fitted.

    The caller provides a rough pre-alignment within the radius (see the module's text); gsplat.snapshots gives the undo."""
    if metric not in ("point", "plane"):
        raise ValueError("align: metric %r is neither 'point' nor 'plane'" % (metric,))
    o = _owner(r)
    if radius is None:
        nearest.distances(o, 1, where=fixed)
        d2, _ = nearest.read(o)
        d = np.sqrt(d2[np.isfinite(d2)].astype(np.float64))
        if not d.size:
            raise ValueError("align: no fixed splat has a nearest fixed splat, give a radius")
        radius = 8.0 * float(np.median(d))
    radius = float(radius)
    plane = metric == "plane"
    if plane:
        nr = surface.radius_for(o, 30, where=fixed) if normal_radius is None else float(normal_radius)
        surface.estimate(o, nr, source=fixed, query=fixed)
    steps, prev, prev_stop = [], None, None
    for _ in range(int(max_iters)):
        md = radius if prev is None else min(radius, float(trim) * prev)
        try:
            rec = plane_step(o, radius, moving, fixed, max_dist=md, damping=damping) if plane else step(o, radius, moving, fixed, max_dist=md, scale=scale)
        except ValueError:
            break
        steps.append(rec)
        stop = rec["rms_plane"] if plane else rec["rms"]
        if prev_stop is not None and abs(stop - prev_stop) <= float(tol) * prev_stop:
            break
        prev, prev_stop = rec["rms"], stop
    return steps


# ---- point-to-plane ------------------------------------------------------------------------------------------------------------------
# The point metric pulls every moving splat towards ONE fixed splat; on walls, floors and table tops sampled at different places the
# tangential part of every pair is sampling noise.  The plane metric penalises only r = n . (q - p), the distance of p to the tangent
# plane of its partner; surfaces may slide over each other.  Linearised about the pivot c, moving p by a small rotation vector w and a
# translation t changes r by -(g . x), g = ((p - c) x n, n), x = (w, t): the normal equations are (sum g g^T) x = sum g r.
_TRI = [[0] * 6 for _ in range(6)]
for _a, _b, _t in ((a, b, t) for t, (a, b) in enumerate((a, b) for a in range(6) for b in range(a, 6))):
    _TRI[_a][_b] = _TRI[_b][_a] = _t


def _pivot(pivot):
    c = np.asarray(pivot, dtype=np.float32).reshape(3)
    return (ctypes.c_float * 3)(*[float(v) for v in c])


def _plane_result(out):
    pair = lambda e: (float(e.hi), float(e.lo))  # noqa: E731
    return {"matched": int(out.matched), "paired": int(out.paired), "G": [[pair(out.G[_TRI[a][b]]) for b in range(6)] for a in range(6)],
            "h": [pair(out.h[k]) for k in range(6)], "rr": pair(out.rr), "d2": pair(out.d2)}


def pair_plane_moments(r, where=SELECTED, max_dist=math.inf, pivot=(0, 0, 0), partner=None, normal=None):
    """gs_pair_plane_moments over the splats i with (s & where[0]) == where[1], their partners j = partner[i] (uint32[N] on the host;
    None: the nearest plane of the last nearest.search on r) and the partners' normals normal[j] (float32[N, 3] on the host; None: the
    normal plane of the last surface.estimate on r, NaN where none): {"matched", "paired", "G": 6 x 6 symmetric table of (hi, lo),
    "h": [(hi, lo)] * 6, "rr", "d2": (hi, lo)}.  With u = p - f32(pivot), d = q - p, r = n . d and g = (u x n, n) in f32 (gs_abi.h
    gives the operation order), paired are the matched splats with j < N, pair_moments' acceptance at f32(max_dist)^2, a finite normal
    and finite g and r; G = sum g g^T, h = sum g r, rr = sum r^2, d2 = sum |d|^2 over them, exact, (hi, lo) as in moments.moments."""
    o = _owner(r)
    ids = nrm = None
    if partner is not None:
        ids = np.ascontiguousarray(partner, dtype=np.uint32).reshape(-1)
        if ids.size != o.numGaussians:
            raise ValueError("pair_plane_moments: the partner plane has %d entries for %d splats" % (ids.size, o.numGaussians))
    if normal is not None:
        nrm = np.ascontiguousarray(normal, dtype=np.float32).reshape(-1)
        if nrm.size != 3 * o.numGaussians:
            raise ValueError("pair_plane_moments: the normal plane has %d floats for %d splats" % (nrm.size, o.numGaussians))
    out = _abi.GsPairPlaneMoments()
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    check(o._L.gs_pair_plane_moments(o._ctx, int(where[0]), int(where[1]), ptr(ids), ptr(nrm), _pivot(pivot), _dist2(max_dist), ctypes.byref(out)))
    return _plane_result(out)


def host_pair_plane_moments(pos, partner, normal, state=None, where=(0, 0), max_dist=math.inf, pivot=(0, 0, 0)):
    """gs_pair_plane_moments_host: the same record from host positions (float32[n, 3] or records [n, 80]), a partner plane
    (uint32[n]), a normal plane (float32[n, 3]) and an optional state plane (uint8[n]); no renderer, no GPU, the same arithmetic."""
    p = np.asarray(pos, dtype=np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)
    planes = [np.ascontiguousarray(p[:, a]) for a in range(3)]
    n = p.shape[0]
    ids = np.ascontiguousarray(partner, dtype=np.uint32).reshape(-1)
    if ids.size != n:
        raise ValueError("host_pair_plane_moments: the partner plane has %d entries for %d positions" % (ids.size, n))
    nrm = np.ascontiguousarray(normal, dtype=np.float32).reshape(-1)
    if nrm.size != 3 * n:
        raise ValueError("host_pair_plane_moments: the normal plane has %d floats for %d positions" % (nrm.size, n))
    st = None
    if state is not None:
        st = np.ascontiguousarray(state, dtype=np.uint8).reshape(-1)
        if st.size != n:
            raise ValueError("host_pair_plane_moments: the state plane has %d entries for %d positions" % (st.size, n))
    out = _abi.GsPairPlaneMoments()
    ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    check(_abi.load().gs_pair_plane_moments_host(ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), n, ptr(ids), ptr(nrm), None if st is None else ptr(st),
                                                 int(where[0]), int(where[1]), _pivot(pivot), _dist2(max_dist), ctypes.byref(out)))
    return _plane_result(out)


def _solve(A, b):
    """Gaussian elimination in Fraction arithmetic with the first non-zero pivot of each column; None when a column has none."""
    k = len(b)
    M = [list(A[i]) + [b[i]] for i in range(k)]
    for c in range(k):
        piv = next((i for i in range(c, k) if M[i][c] != 0), None)
        if piv is None:
            return None
        M[c], M[piv] = M[piv], M[c]
        for i in range(c + 1, k):
            if M[i][c] != 0:
                f = M[i][c] / M[c][c]
                M[i] = [x - f * y for x, y in zip(M[i], M[c])]
    x = [Fraction(0)] * k
    for c in range(k - 1, -1, -1):
        x[c] = (M[c][k] - sum((M[c][j] * x[j] for j in range(c + 1, k)), Fraction(0))) / M[c][c]
    return x


def fit_plane(m, pivot, damping=0.0, rcond=1e-6):
    """The point-to-plane step of a pair_plane_moments() record taken about `pivot`: the small rotation vector w and the translation
    t that minimise sum (r - g . x)^2, x = (w, t), to first order in w.

    With n = paired and the sums as the record holds them (Fraction(hi) + Fraction(lo)), in rational arithmetic:
        L2 = (G00 + G11 + G22) / (G33 + G44 + G55)            (L: the rms lever arm; it makes the damping unit-free)
        D  = diag(L2, L2, L2, 1, 1, 1)
        (G + damping n D) x = h                                 by Gaussian elimination, each x_k rounded ONCE to float64
        predicted = sqrt(max((rr - h . x) / n, 0))              the plane rms the normal equations predict after the move
        rms_plane = sqrt(rr / n),  rms = sqrt(d2 / n)           the residuals of the pairs BEFORE the move, in float64
    Rotation: theta = |w|, the quaternion (cos theta/2, sin(theta/2) w / theta), the identity for theta = 0, with math functions in
    float64.  "eigen": numpy.linalg.eigvalsh of D^(-1/2) (G + damping n D) D^(-1/2) / n in float64, ascending -- a diagnostic only.
    With damping == 0, a zero pivot in the elimination or a smallest eigenvalue <= rcond x the largest raises ValueError naming the
    eigenvalues: the normals span fewer than three directions (or the patches let the capture slide or turn), a direction is
    unconstrained.  rcond's default of 1e-6 is a design choice, not a measurement: a scene of three well-spread patches sits near 1e-2,
    a single plane at rounding noise.  With damping > 0 the system is always solved and unconstrained directions do not move.
    Fewer than 6 pairs: ValueError.
    Returns {"rot": (r, x, y, z), "translate", "scale": 1.0, "pivot", "paired", "rms", "rms_plane", "predicted", "eigen", "x"}, so
    xform_of works on it: p' = R (p - pivot) + pivot + t."""
    n = int(m["paired"])
    if n < 6:
        raise ValueError("fit_plane: %d pairs, 6 needed" % n)
    damping = float(damping)
    if not (damping >= 0.0 and math.isfinite(damping)):
        raise ValueError("fit_plane: damping %g is not a finite number >= 0" % damping)
    G = [[exact(m["G"][a][b]) for b in range(6)] for a in range(6)]
    h = [exact(v) for v in m["h"]]
    rr, d2 = exact(m["rr"]), exact(m["d2"])
    lever, unit = G[0][0] + G[1][1] + G[2][2], G[3][3] + G[4][4] + G[5][5]
    if unit == 0:
        raise ValueError("fit_plane: every paired normal is zero")
    L2 = lever / unit
    D = [L2 if L2 > 0 else Fraction(1)] * 3 + [Fraction(1)] * 3  # (no lever arm at all: every u x n is zero, any unit serves)
    lam = Fraction(damping) * n
    A = [[G[a][b] + (lam * D[a] if a == b else 0) for b in range(6)] for a in range(6)]
    # the diagnostic: the matrix in units where a lever arm of L counts like a translation of 1
    s = [math.sqrt(float(d)) if d > 0 else 1.0 for d in D]
    eigen = np.linalg.eigvalsh(np.array([[float(A[a][b] / n) / (s[a] * s[b]) for b in range(6)] for a in range(6)], dtype=np.float64))
    x = _solve(A, h)
    if x is None or (damping == 0.0 and not eigen[0] > float(rcond) * eigen[-1]):
        raise ValueError("fit_plane: a direction is not constrained by the pairs' normals (eigenvalues %s): give a damping"
                         % ", ".join("%g" % e for e in eigen))
    predicted = (rr - sum((h[k] * x[k] for k in range(6)), Fraction(0))) / n
    xf = np.array([float(v) for v in x], dtype=np.float64)
    w = xf[0:3]
    theta = math.sqrt(float(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]))
    if theta == 0.0:
        rot = (1.0, 0.0, 0.0, 0.0)
    else:
        k = math.sin(0.5 * theta) / theta
        rot = (math.cos(0.5 * theta), k * float(w[0]), k * float(w[1]), k * float(w[2]))
    return {"rot": rot, "translate": xf[3:6].copy(), "scale": 1.0, "pivot": np.asarray(pivot, dtype=np.float64).reshape(3).copy(), "paired": n,
            "rms": math.sqrt(float(d2 / n)), "rms_plane": math.sqrt(float(rr / n)), "predicted": math.sqrt(max(float(predicted), 0.0)),
            "eigen": eigen, "x": xf}


def plane_step(r, radius, moving=SELECTED, fixed=UNSELECTED, max_dist=None, damping=0.0, pivot=None):
    """One point-to-plane ICP step: nearest.search(k=1, query=moving, source=fixed) at `radius`, pair_plane_moments over `moving` on
    the ctx's own nearest and surface normal planes with max_dist (None: the radius) about `pivot` (None: the float32 rounding of
    moments.centroid(r, moving)), fit_plane, and the fit's transform applied to `moving` in place.

    It does NOT estimate normals: the caller runs surface.estimate(r, normal_radius, query=fixed, source=fixed) ONCE before the
    first step -- the fixed splats do not move during an alignment, so one estimate serves every step, and the moving splats' stale
    normals are never read.  Without an estimate every normal reads NaN, nothing pairs and the fit raises.

    Returns the fit with "search" (the search's info), "radius", "max_dist" and "moved" (the splats transformed); "rms" and
    "rms_plane" are those of the pairs BEFORE the move.  A ValueError from fit_plane (too few pairs, an unconstrained direction with
    damping == 0) is raised before anything moves."""
    o = _owner(r)
    info = nearest.search(o, 1, radius, source=fixed, query=moving)
    md = float(radius) if max_dist is None else float(max_dist)
    c = moments.centroid(o, moving).astype(np.float32) if pivot is None else np.asarray(pivot, dtype=np.float32).reshape(3)
    f = fit_plane(pair_plane_moments(o, moving, md, c), c, damping)
    f["moved"] = o.transform(xform_of(f), int(moving[0]), int(moving[1]))
    f["search"], f["radius"], f["max_dist"] = info, float(radius), md
    return f
