"""Restatement of the surface estimate (include/gsplat/gs_abi.h "surface") in numpy: test infrastructure, imports nothing of the library.

  sums()      all pairs with the header's f32 acceptance -- d = p_j - p_i, (dx dx + dy dy) + dz dz <= radius * radius, one rounding per
              operation, self excluded by index, a non-finite coordinate has no neighbours and is nobody's --, the ONE quantisation
              q = rint(d * 2^(16 - E)) and int64 sums: count, S[3], M[6] = xx xy xz yy yz zz.  Exact, so compared bit for bit.
  model()     an INDEPENDENT float64 finishing: the covariance from exact integer arithmetic, numpy.linalg.eigh, the header's sign rule.
              Compared within derived bounds (tests/test_surface.py), never bit for bit.
  orient(), feature(), member()   the f32 rules of GS_SURFACE_ORIENT and of gs_state_surface, one rounding per written operation.
"""
import numpy as np

F = np.float32
NAN_BITS = 0x7FC00000
KINDS = ("variation", "planarity", "linearity", "sphericity", "facing", "facing_signed", "count")


def scale(radius):
    """(E, s, r2): frexp's exponent of the f32 radius, s = 2^(16 - E) as f32, r2 = radius * radius in f32."""
    r = F(radius)
    e = int(np.frexp(r)[1])
    return e, F(np.ldexp(np.float64(1.0), 16 - e)), r * r


def sums(pos, radius, src=None, qry=None):
    """(count uint32[n], sums int64[n, 10], info): info = {"queried", "sources", "unresolved"}."""
    p = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    n = p.shape[0]
    src = np.ones(n, bool) if src is None else np.asarray(src, bool)
    qry = np.ones(n, bool) if qry is None else np.asarray(qry, bool)
    _, s, r2 = scale(radius)
    fin = np.isfinite(p).all(axis=1)
    out = np.zeros((n, 10), np.int64)
    ok_src = src & fin
    with np.errstate(all="ignore"):
        for i0 in range(0, n, 128):
            i1 = min(n, i0 + 128)
            d = p[None, :, :] - p[i0:i1, None, :]  # [i, j, a] = p_j - p_i, f32
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert d2.dtype == F
            acc = (d2 <= r2) & ok_src[None, :] & (qry & fin)[i0:i1, None]
            acc[np.arange(i1 - i0), np.arange(i0, i1)] = False
            q = np.rint(np.where(acc[..., None], d, F(0)) * s)
            assert q.dtype == F
            q = q.astype(np.int64)
            out[i0:i1, 0] = acc.sum(axis=1)
            out[i0:i1, 1:4] = q.sum(axis=1)
            for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                out[i0:i1, 4 + k] = (q[..., a] * q[..., b]).sum(axis=1)
    count = out[:, 0].astype(np.uint32)
    info = {"queried": int(qry.sum()), "sources": int(src.sum()), "unresolved": int((qry & (count < 3)).sum())}
    return count, out, info


def max_abs_q(pos, radius):
    """The largest |q| over all accepted pairs (every splat a source and a query)."""
    p = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    _, s, r2 = scale(radius)
    with np.errstate(all="ignore"):
        d = p[None, :, :] - p[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        acc = (d2 <= r2) & ~np.eye(p.shape[0], dtype=bool)
        q = np.rint(np.where(acc[..., None], d, F(0)) * s)
    return int(np.abs(q).max()) if q.size else 0


def model(sums10, radius):
    """(eig float64[n, 3] descending in world units, normal float64[n, 3]) from the integer sums; NaN rows where count < 3.  The
    covariance entries are exact rationals (n M_ab - S_a S_b) / n^2 rounded once to float64."""
    e, _, _ = scale(radius)
    unscale = 2.0 ** (2 * (e - 16))
    n = sums10.shape[0]
    eig, nrm = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for i in range(n):
        w = [int(v) for v in sums10[i]]
        if w[0] < 3:
            continue
        c = np.zeros((3, 3))
        for k, (a, b) in enumerate(pairs):
            c[a, b] = c[b, a] = (w[0] * w[4 + k] - w[1 + a] * w[1 + b]) / (w[0] * w[0])
        lam, vec = np.linalg.eigh(c)
        eig[i] = np.maximum(lam[::-1], 0.0) * unscale
        v = vec[:, 0]
        big = int(np.argmax(np.abs(v)))  # the first of a tie
        nrm[i] = -v if v[big] < 0 else v
    return eig, nrm


def orient(normal, pos, toward):
    """GS_SURFACE_ORIENT on unoriented f32 normals: negated where t = (nx ex + ny ey) + nz ez < 0, e = toward - p, all f32."""
    nv = np.array(normal, dtype=F, copy=True)
    p = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e = np.asarray(toward, F)[None, :] - p
        t = (nv[:, 0] * e[:, 0] + nv[:, 1] * e[:, 1]) + nv[:, 2] * e[:, 2]
    assert t.dtype == F
    nv[t < 0] = -nv[t < 0]
    return nv


def feature(kind, normal, eig, count, axis=(0, 0, 0)):
    """The f32 value gs_state_surface compares, from the planes as gs_surface_read returns them."""
    nv, ev = np.asarray(normal, F), np.asarray(eig, F)
    l0, l1, l2 = ev[:, 0], ev[:, 1], ev[:, 2]
    a = np.asarray(axis, F)
    with np.errstate(all="ignore"):
        if kind == "variation":
            v = l2 / ((l0 + l1) + l2)
        elif kind == "planarity":
            v = (l1 - l2) / l0
        elif kind == "linearity":
            v = (l0 - l1) / l0
        elif kind == "sphericity":
            v = l2 / l0
        elif kind in ("facing", "facing_signed"):
            v = (nv[:, 0] * a[0] + nv[:, 1] * a[1]) + nv[:, 2] * a[2]
            if kind == "facing":
                v = np.abs(v)
        else:
            v = np.asarray(count).astype(F)
    assert v.dtype == F
    return v


def member(v, lo, hi, inside=True):
    """(v >= lo && v <= hi) == inside in f32: a NaN is in no range."""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        return ((v >= F(lo)) & (v <= F(hi))) == bool(inside)
