"""The plane pair moments and the point-to-plane step (gs_abi.h "registration") restated on the host: the definition the library is
held to.

THE ROW in numpy float32, in the header's operation order (numpy float32 arithmetic rounds every operation once): u = p - pivot,
d = q - p, d2 = (dx dx + dy dy) + dz dz, r = (nx dx + ny dy) + nz dz, c = (uy nz - uz ny, uz nx - ux nz, ux ny - uy nx),
g = (c, n).  A splat i that passes the filter is PAIRED when j = partner[i] < N, the six coordinates of p = p_i and q = p_j are
finite, d2 <= max_d2 (inclusive), the three components of n = normal[j] are finite and cx, cy, cz, r are finite.
THE 29 SUMS with fractions.Fraction as pairs_restate does: the terms are gathered as Python integers in units of 2^-UNIT, S =
Fraction(total, 2^UNIT), hi = float(S), lo = float(S - Fraction(hi)).  G[21] the upper triangle of sum g g^T row-major, h[6] = sum
g_k r, rr = sum r r, d2 = sum of the f32 value d2 (a d2 of +inf, which only max_d2 = +inf lets pass, counts as 2^128: what its bit
pattern splits into).
THE STEP: brute-force nearest (knn_restate) -> these sums -> gsplat.register.fit_plane (rational arithmetic, every number rounded
once) -> xform_restate.apply of register.xform_of."""
from fractions import Fraction

import numpy as np

import knn_restate
import moments_restate as mr
import pairs_restate as pr
import xform_restate as xr

F = np.float32
NONE = pr.NONE
UNIT = pr.UNIT
TRI = [(a, b) for a in range(6) for b in range(a, 6)]
# the two factors of each product quantity among f = (cx, cy, cz, nx, ny, nz, r): G, then h, then rr
FACTORS = TRI + [(k, 6) for k in range(6)] + [(6, 6)]


def rows(pos, partner, normal, pivot=(0, 0, 0)):
    """(valid, d2 float32[N], f float32[N, 7]): valid where everything but the filter and the bound holds; f = (c, n, r), 0 where not."""
    p = np.ascontiguousarray(np.asarray(pos, F)[:, :3])
    nrm = np.ascontiguousarray(np.asarray(normal, F).reshape(-1, 3))
    n = p.shape[0]
    c = np.asarray(pivot, F).reshape(3)
    j = np.asarray(partner, np.uint32).astype(np.int64)
    valid = j < n
    jj = np.where(valid, j, 0)
    q, nn = (p[jj], nrm[jj]) if n else (p, nrm)
    valid = valid & np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1) & np.isfinite(nn).all(axis=1)
    with np.errstate(all="ignore"):
        u = p - c[None, :]
        d = q - p
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        r = (nn[:, 0] * d[:, 0] + nn[:, 1] * d[:, 1]) + nn[:, 2] * d[:, 2]
        cx = u[:, 1] * nn[:, 2] - u[:, 2] * nn[:, 1]
        cy = u[:, 2] * nn[:, 0] - u[:, 0] * nn[:, 2]
        cz = u[:, 0] * nn[:, 1] - u[:, 1] * nn[:, 0]
    f = np.stack([cx, cy, cz, nn[:, 0], nn[:, 1], nn[:, 2], r], axis=1)
    assert f.dtype == F and d2.dtype == F
    valid = valid & np.isfinite(f).all(axis=1)
    return valid, np.where(valid, d2, F(0)), np.where(valid[:, None], f, F(0))


def _ints64(v):
    """A float64 array of f32-representable values (or 2^128) as (integer mantissas, exponents): v = M 2^E exactly."""
    m, e = np.frexp(v)
    M = (m * 2.0 ** 24).astype(np.int64)
    assert (M.astype(np.float64) == m * 2.0 ** 24).all()
    return [int(x) for x in M], [int(x) - 24 + UNIT for x in e]


def columns(pos, partner, normal, pivot=(0, 0, 0)):
    """(valid, d2, cols): cols[t][i] the term of quantity t (G[21], h[6], rr, d2) of splat i as a Python integer in units of
    2^-UNIT, 0 where the splat is not valid."""
    valid, d2, f = rows(pos, partner, normal, pivot)
    parts = [_ints64(f[:, k].astype(np.float64)) for k in range(7)]
    cols = []
    for a, b in FACTORS:
        (ma, ea), (mb, eb) = parts[a], parts[b]
        cols.append([(x * y) << (s + t - UNIT) for x, s, y, t in zip(ma, ea, mb, eb)])
    big = np.where(np.isinf(d2), 2.0 ** 128, d2.astype(np.float64))
    md, ed = _ints64(big)
    cols.append([x << s for x, s in zip(md, ed)])
    return valid, d2, cols


def record(cols_of, keep=None, max_d2=np.inf):
    """The dict of register.pair_plane_moments from columns(): the splats with keep (None: all), valid and d2 <= max_d2 are paired."""
    valid, d2, cols = cols_of
    n = valid.size
    keep = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    with np.errstate(all="ignore"):
        paired = keep & valid & (d2 <= F(max_d2))
    idx = [int(i) for i in np.flatnonzero(paired)]
    s = [mr.pair(Fraction(sum(c[i] for i in idx), 1 << UNIT)) for c in cols]
    G = [[None] * 6 for _ in range(6)]
    for t, (a, b) in enumerate(TRI):
        G[a][b] = G[b][a] = s[t]
    return {"matched": int(keep.sum()), "paired": len(idx), "G": G, "h": s[21:27], "rr": s[27], "d2": s[28]}


def restate(pos, partner, normal, keep=None, max_d2=np.inf, pivot=(0, 0, 0)):
    return record(columns(pos, partner, normal, pivot), keep, max_d2)


def by_fractions(pos, partner, normal, keep=None, max_d2=np.inf, pivot=(0, 0, 0)):
    """The same record term by term with Fraction(float(v)) -- slow; what pins the integer columns above."""
    valid, d2, f = rows(pos, partner, normal, pivot)
    keep = np.ones(valid.size, bool) if keep is None else np.asarray(keep, bool)
    with np.errstate(all="ignore"):
        idx = np.flatnonzero(keep & valid & (d2 <= F(max_d2)))
    cols = [[Fraction(float(v)) for v in f[idx, k]] for k in range(7)]
    tot = lambda it: mr.pair(sum(it, Fraction(0)))  # noqa: E731
    s = [tot(x * y for x, y in zip(cols[a], cols[b])) for a, b in FACTORS]
    s.append(tot(Fraction(2) ** 128 if np.isinf(v) else Fraction(float(v)) for v in d2[idx]))
    G = [[None] * 6 for _ in range(6)]
    for t, (a, b) in enumerate(TRI):
        G[a][b] = G[b][a] = s[t]
    return {"matched": int(keep.sum()), "paired": int(idx.size), "G": G, "h": s[21:27], "rr": s[27], "d2": s[28]}


def flat(m):
    """The 29 (hi, lo) in the record's order."""
    return [m["G"][a][b] for a, b in TRI] + list(m["h"]) + [m["rr"], m["d2"]]


def same(got, want):
    """Bit for bit: both counts, hi and lo of the 29 entries as uint64, and the table's symmetry."""
    if (got["matched"], got["paired"]) != (want["matched"], want["paired"]):
        return False
    both = lambda e: (mr.bits(e[0]), mr.bits(e[1]))  # noqa: E731
    if any(both(got["G"][a][b]) != both(got["G"][b][a]) for a in range(6) for b in range(a)):
        return False
    return all(mr.bits(a[0]) == mr.bits(b[0]) and mr.bits(a[1]) == mr.bits(b[1]) for a, b in zip(flat(got), flat(want)))


def as_bytes(want):
    """The 480 bytes of the record."""
    from gsplat import _abi
    rec = _abi.GsPairPlaneMoments()
    rec.matched, rec.paired = want["matched"], want["paired"]
    e = (_abi.GsExact * 29).from_buffer(rec, 16)
    for t, (hi, lo) in enumerate(flat(want)):
        e[t].hi, e[t].lo = hi, lo
    return bytes(rec)


# ---- normal planes: (n, 3) float32, seeded ------------------------------------------------------------------------------------------------
NORMALS = ("unit", "nan_third", "huge")


def normals(kind, n, seed=29):
    """unit: random unit vectors rounded to f32.  nan_third: those with NaN 0x7FC00000 in all three components of every third splat
    (an unresolved normal).  huge: un-normalised, magnitudes 2^-40 .. 2^126 -- c or r overflows to +-inf for some pairs."""
    rng = np.random.default_rng(seed + n)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if kind == "huge":
        v = v * 2.0 ** rng.integers(-40, 127, size=(n, 1))
    out = np.ascontiguousarray(v.astype(F))
    if kind == "nan_third":
        out.view(np.uint32)[1::3] = knn_restate.NAN_BITS
    return out


# ---- the step and the loop, restated -------------------------------------------------------------------------------------------------------
def centroid32(rec, mov):
    """The float32 rounding of moments.centroid over the moving splats (all finite here)."""
    return np.array([mr.mean(rec[mov, a]) for a in range(3)], dtype=np.float64).astype(F)


def step(rec, st, radius, normal, moving=(2, 2), fixed=(2, 0), max_dist=None, damping=0.0, pivot=None):
    """(records after the step, the fit, the nearest plane): brute-force nearest of the moving splats among the fixed ones within
    `radius`, the sums within max_dist (None: the radius) about pivot (None: centroid32), register.fit_plane,
    xform_restate.apply of register.xform_of on the moving splats.  A ValueError of the fit propagates."""
    from gsplat import register
    rec = np.ascontiguousarray(rec, dtype=F)
    mov, fix = pr.masks(st, moving, fixed)
    _, near, _ = knn_restate.planes(rec, 1, radius, src=fix, qry=mov)
    md = F(radius if max_dist is None else max_dist)
    c = centroid32(rec, mov) if pivot is None else np.asarray(pivot, F).reshape(3)
    with np.errstate(all="ignore"):
        m = restate(rec[:, :3], near, normal, mov, md * md, c)
    f = register.fit_plane(m, c, damping)
    out = xr.apply(rec, xr.Xform.from_struct(register.xform_of(f)), mov)
    return out, f, near


def fixed_normals(rec, st, normal_radius, fixed=(2, 0)):
    """The normal plane surface.estimate(query=fixed, source=fixed) leaves, from its host twin (bit-equal to the device's)."""
    from gsplat import surface
    return surface.host_estimate(np.ascontiguousarray(rec[:, :3]), normal_radius, np.asarray(st, np.uint8), source=fixed, query=fixed)[0]


def align(rec, st, radius, normal_radius, moving=(2, 2), fixed=(2, 0), max_iters=30, tol=1e-6, trim=3.0, damping=0.0):
    """register.align(metric="plane")'s loop on the restated step: (final records, [the fits])."""
    normal = fixed_normals(rec, st, normal_radius, fixed)
    steps, prev, prev_stop = [], None, None
    for _ in range(max_iters):
        md = float(radius) if prev is None else min(float(radius), float(trim) * prev)
        try:
            rec, f, _ = step(rec, st, radius, normal, moving, fixed, md, damping)
        except ValueError:
            break
        f["radius"], f["max_dist"] = float(radius), md
        steps.append(f)
        if prev_stop is not None and abs(f["rms_plane"] - prev_stop) <= tol * prev_stop:
            break
        prev, prev_stop = f["rms"], f["rms_plane"]
    return rec, steps
