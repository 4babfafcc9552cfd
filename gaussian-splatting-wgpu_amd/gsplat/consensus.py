"""Consensus: score many plane or ball hypotheses in one pass, and find planes (include/gsplat/gs_abi.h "consensus").

Free functions over a ``Renderer`` or a ``PipelinedRenderer``, like gsplat.register.  ``moments.fit_plane`` gives the least-squares
plane through a selection that EXISTS; these find the plane -- the floor, a wall, a table top -- in an unselected, cluttered capture
by RANSAC: candidate planes through random splat triples, each scored by how many splats lie within a distance of it, the best kept.
All candidates of a call are scored in ONE streaming pass over the resident positions:

    f = consensus.find_plane(r, 0.02)                           # a pure query: {"plane", "count", "matched", "trial"} or None
    g = consensus.select_plane(r, 0.02)                         # ... and its inliers are the selection, refined by a least-squares fit
    r.hide_selected()                                           # "remove the table and keep the object"
    planes = consensus.detect_planes(r, 0.02, max_planes=4)     # floor and walls, one after the other; their union is selected
    centre, count = consensus.densest_ball(r, 0.5)              # where the main object is: a coarse seed for register.align

Everything is restatable on a host: the draws are numpy's (``default_rng(seed)``), the plane through a triple is gs_planes_through's
written-out double arithmetic, a count is an integer over the attribute's own f32 expression (host_score runs the same loop without
a GPU), the winner is the FIRST maximum.  Only ``moments.fit_plane``'s axes inside select_plane's refinement are what the installed
LAPACK returns and are not bit-pinned, as for moments.principal_axes.
"""
import ctypes
import math

import numpy as np

from . import _abi, attributes, moments
from ._abi import check
from .attributes import _owner, attr
from .register import _dist2

PLANE, DIST2 = _abi.GS_ATTR_PLANE, _abi.GS_ATTR_DIST2
_SELECTED = _abi.GS_SPLAT_SELECTED
_HOST_BITS = (0x04, 0x08, 0x10, 0x20, 0x40, 0x80)  # bits 2 to 7 of the state byte are the host's


def _table(params):
    p = np.ascontiguousarray(params, dtype=np.float32)
    if p.size % 4:
        raise ValueError("consensus: the parameters are not float32[h][4]")
    return p.reshape(-1, 4)


def score(r, kind, params, lo, hi, where=(0, 0)):
    """gs_attr_consensus: (counts uint64[h], matched).  counts[j]: the splats with (s & where[0]) == where[1] whose value under
    hypothesis j is in [lo, hi], both ends inclusive; the value is attributes.attr(kind, params[j])'s -- PLANE
    ((p0 x + p1 y) + p2 z) + p3, DIST2 the squared distance from p[0..2] -- in f32, one rounding per operation.  params:
    float32[h][4], 1 <= h <= 4096, and need not be finite: a NaN value is in no range.  lo > hi is the empty range, infinite bounds
    are fine.  matched: the splats that pass the filter.  One pass over the positions for all h hypotheses."""
    o = _owner(r)
    p = _table(params)
    counts = np.zeros(p.shape[0], dtype=np.uint64)
    matched = ctypes.c_uint64()
    check(o._L.gs_attr_consensus(o._ctx, int(kind), p.ctypes.data if p.size else None, p.shape[0], float(lo), float(hi), int(where[0]),
                                 int(where[1]), counts.ctypes.data if counts.size else None, ctypes.byref(matched)))
    return counts, int(matched.value)


def host_score(pos, kind, params, lo, hi, state=None, where=(0, 0)):
    """gs_consensus_host: the same counts from host positions (float32[n, 3] or records [n, 80]) and an optional state plane
    (uint8[n]); no renderer, no GPU, the same code."""
    q = np.asarray(pos, dtype=np.float32)
    q = q.reshape(-1, q.shape[-1] if q.ndim > 1 else 3)
    planes = [np.ascontiguousarray(q[:, a]) for a in range(3)]
    n = q.shape[0]
    st = None
    if state is not None:
        st = np.ascontiguousarray(state, dtype=np.uint8).reshape(-1)
        if st.size != n:
            raise ValueError("host_score: the state plane has %d entries for %d positions" % (st.size, n))
    p = _table(params)
    counts = np.zeros(p.shape[0], dtype=np.uint64)
    matched = ctypes.c_uint64()
    ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    check(_abi.load().gs_consensus_host(ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), n, None if st is None else ptr(st), int(where[0]),
                                        int(where[1]), int(kind), ptr(p), p.shape[0], float(lo), float(hi), ptr(counts), ctypes.byref(matched)))
    return counts, int(matched.value)


def gather(r, a, ids):
    """gs_attr_gather: float32[m], the value of attribute a (attributes.attr) of each splat of ids, in the order given; repeats are
    fine.  An id at or above the number of resident splats is refused."""
    o = _owner(r)
    i = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    out = np.empty(i.size, dtype=np.float32)
    check(o._L.gs_attr_gather(o._ctx, ctypes.byref(a), i.ctypes.data if i.size else None, i.size, out.ctypes.data if i.size else None))
    return out


def planes_through(points):
    """gs_planes_through: float32[h][4], the PLANE parameters (unit normal, offset) of the plane through each triple of points
    (float32[h][9] or [h][3][3]: a, b, c).  Double arithmetic as the header writes it out; the normal's component of largest
    magnitude (the first on a tie) is positive; a degenerate triple (a repeated point, collinear points, a non-finite coordinate)
    gives four NaNs, which score() counts as 0."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 9)
    out = np.empty((pts.shape[0], 4), dtype=np.float32)
    check(_abi.load().gs_planes_through(pts.ctypes.data if pts.size else None, pts.shape[0], out.ctypes.data if pts.size else None))
    return out


def plane_params(normal, offset):
    """float32[4]: a plane normal . p + offset = 0 given in float64 (moments.fit_plane's) as PLANE parameters under
    gs_planes_through's sign convention: negated when the normal's component of largest magnitude (the first on a tie) is negative,
    then rounded to f32."""
    m = [float(v) for v in normal]
    d = float(offset)
    big = 0
    for k in (1, 2):
        if abs(m[k]) > abs(m[big]):
            big = k
    if m[big] < 0.0:
        m, d = [-v for v in m], -d
    return np.array(m + [d], dtype=np.float32)


def _pool(o, where):
    """The ids a sampler draws from: every splat for (0, 0), else the splats that pass the filter, ascending."""
    if tuple(int(v) for v in where) == (0, 0):
        return np.arange(o.numGaussians, dtype=np.uint32)
    return o.list_state(int(where[0]), int(where[1]))


def _positions(o, ids):
    """float32[m][3]: three gathers."""
    return np.stack([gather(o, attr(k), ids) for k in (_abi.GS_ATTR_POS_X, _abi.GS_ATTR_POS_Y, _abi.GS_ATTR_POS_Z)], axis=1)


def _first_max(counts):
    j = int(np.argmax(counts)) if counts.size else 0  # (numpy's argmax returns the first maximum)
    return j, (int(counts[j]) if counts.size else 0)


def find_plane(r, distance, trials=1024, seed=0, where=(0, 0)):
    """RANSAC for the plane with the most splats within `distance` of it, among the splats that pass `where`.  A pure query: no
    state changes.  The pool is every id for (0, 0), else list_state(where); the triples are
    numpy.random.default_rng(seed).integers(0, pool.size, (trials, 3)) into it, their positions three gather() calls, the candidates
    planes_through() of them, the scores score(PLANE, params, -d, d, where) with d = float32(distance); the winner is the FIRST
    maximum.  Returns {"plane": float32[4], "count", "matched", "trial"}, or None when the best count is below 3 (or the pool is empty).
    trials: 1 .. 4096."""
    o = _owner(r)
    pool = _pool(o, where)
    if not pool.size:
        return None
    draws = np.random.default_rng(seed).integers(0, pool.size, (int(trials), 3))
    params = planes_through(_positions(o, pool[draws].reshape(-1)).reshape(int(trials), 9))
    d = np.float32(distance)
    counts, matched = score(o, PLANE, params, -d, d, where)
    j, best = _first_max(counts)
    if best < 3:
        return None
    return {"plane": params[j].copy(), "count": best, "matched": matched, "trial": j}


def _reselect(o, plane, d, where):
    """Among the splats that pass `where`: SELECTED cleared on those outside [-d, d] of the plane (a NaN value is outside), set on
    those inside; returns how many are inside."""
    a = attr(PLANE, plane)
    attributes.select(o, a, -d, d, inside=False, op=_abi.GS_STATE_CLEAR, where=where)
    return attributes.select(o, a, -d, d, inside=True, op=_abi.GS_STATE_SET, where=where)


def select_plane(r, distance, trials=1024, seed=0, where=(0, 0), refine=2):
    """find_plane, then the selection is its inliers: SELECTED is cleared on the splats that pass `where` and set on those within
    float32(distance) of the plane (attributes.select with the same attribute and range); splats outside `where` keep their bytes.
    Then up to `refine` rounds: moments.fit_plane over the selected splats among `where`, rounded to float32 by plane_params();
    score()d alone; kept, and the inliers reselected, if its count is at least the current one, else the refinement stops.  Needs
    GS_FLAG_SPLAT_STATE; a `where` that names the SELECTED bit raises ValueError.  Returns {"plane", "count", "matched", "trial",
    "refined": rounds kept}, or None (nothing changed) when find_plane found none.  count is what
    state_count(where[0] | 2, where[1] | 2) reports afterwards."""
    m, v = int(where[0]), int(where[1])
    if m & _SELECTED:
        raise ValueError("select_plane: `where` names the SELECTED bit, which the call writes")
    o = _owner(r)
    f = find_plane(o, distance, trials, seed, (m, v))
    if f is None:
        return None
    d = np.float32(distance)
    plane = f["plane"]
    count = _reselect(o, plane, d, (m, v))
    rounds = 0
    for _ in range(int(refine)):
        try:
            normal, offset, _ = moments.fit_plane(o, (m | _SELECTED, v | _SELECTED))
        except ValueError:
            break
        cand = plane_params(normal, offset)
        c, _ = score(o, PLANE, cand[None, :], -d, d, (m, v))
        if int(c[0]) < count:
            break
        plane = cand
        count = _reselect(o, plane, d, (m, v))
        rounds += 1
    return {"plane": plane, "count": count, "matched": f["matched"], "trial": f["trial"], "refined": rounds}


def detect_planes(r, distance, max_planes=8, min_inliers=None, trials=1024, seed=0, where=(0, 0), scratch_bit=0x80, refine=2):
    """Planes one after the other: select_plane (seed + k for plane k) over the splats that pass `where` and do not carry
    `scratch_bit`; each plane's inliers are marked with that bit and so are out of the next search.  Stops after max_planes, or at
    the first plane with fewer than min_inliers inliers (None: a twentieth of the splats that pass `where`, at least 3), which is
    not returned.  Then the union of the planes' inliers is the selection among `where`, the bit is cleared, and the list of
    select_plane's records is returned.  scratch_bit: one of the host's bits (0x04 .. 0x80), not named by `where`, and carried by
    no splat that passes `where` -- else ValueError."""
    m, v, sb = int(where[0]), int(where[1]), int(scratch_bit)
    if sb not in _HOST_BITS:
        raise ValueError("detect_planes: scratch_bit 0x%x is not one of the host's bits 0x04 .. 0x80" % sb)
    if m & (_SELECTED | sb):
        raise ValueError("detect_planes: `where` names the SELECTED bit or the scratch bit, which the call writes")
    o = _owner(r)
    if o.state_count(m | sb, v | sb):
        raise ValueError("detect_planes: splats that pass `where` already carry the scratch bit 0x%x" % sb)
    if min_inliers is None:
        min_inliers = max(3, o.state_count(m, v) // 20)
    d = np.float32(distance)
    rest = (m | sb, v)
    planes = []
    for k in range(int(max_planes)):
        g = select_plane(o, distance, trials, seed + k, rest, refine)
        if g is None or g["count"] < int(min_inliers):
            break
        attributes.select(o, attr(PLANE, g["plane"]), -d, d, inside=True, op=_abi.GS_STATE_SET, bits=sb, where=rest)
        planes.append(g)
    # the union: SELECTED exactly on the marked splats among `where`; then the mark goes
    o.state_region(_abi.GS_REGION_ALL, _abi.GS_STATE_CLEAR, _SELECTED, where=(m | sb, v))
    o.state_region(_abi.GS_REGION_ALL, _abi.GS_STATE_SET, _SELECTED, where=(m | sb, v | sb))
    o.state_region(_abi.GS_REGION_ALL, _abi.GS_STATE_CLEAR, sb, where=(m | sb, v | sb))
    return planes


def densest_ball(r, radius, trials=1024, seed=0, where=(0, 0)):
    """The ball of `radius` around a resident splat that holds the most splats, among those that pass `where`: the centres are the
    positions of the pool splats numpy.random.default_rng(seed).integers(0, pool.size, trials) (the pool as in find_plane), the scores
    score(DIST2, centres, -inf, r2, where) with r2 = float32(radius) squared as ONE f32 product.  Returns (centre float32[3], count) of
    the FIRST maximum, or None when the pool is empty.  A centre with a non-finite coordinate counts nothing."""
    o = _owner(r)
    pool = _pool(o, where)
    if not pool.size:
        return None
    ids = pool[np.random.default_rng(seed).integers(0, pool.size, int(trials))]
    centres = _positions(o, ids)
    params = np.concatenate([centres, np.zeros((centres.shape[0], 1), np.float32)], axis=1)
    counts, _ = score(o, DIST2, params, -math.inf, _dist2(radius), where)
    j, best = _first_max(counts)
    return centres[j].copy(), best
