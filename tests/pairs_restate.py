"""The pair moments and the registration step (gs_abi.h "registration") restated on the host: the definition the library is held to.

THE PAIRING RULE in numpy float32, with knn_restate's expression: a splat i that passes the filter is PAIRED when j = partner[i] < N,
the six coordinates of p = p_i and q = p_j are finite and d2 = (dx dx + dy dy) + dz dz <= max_d2, d = q - p, every operation rounded
once to f32 (numpy float32 arithmetic does that), the comparison inclusive.
THE 21 SUMS with fractions.Fraction, exactly as moments_restate.pair does: S = the sum of the real numbers, hi = float(S), lo =
float(S - Fraction(hi)).  The terms are gathered as Python integers in units of 2^-UNIT first (a finite f32 and a product of two are
integer multiples of it), so S = Fraction(total, 2^UNIT) costs one big-integer sum per quantity and not a gcd per term.
THE STEP: brute-force nearest (knn_restate) -> these pairs -> gsplat.register.fit (the same fit: its SVD is not bit-pinned, everything
before it is) -> xform_restate.apply of register.xform_of."""
from fractions import Fraction

import numpy as np

import knn_restate
import moments_restate as mr
import xform_restate as xr

F = np.float32
NONE = 0xFFFFFFFF
UNIT = 400  # 2^-149 is 2^23 2^-172 as frexp splits it, a product of two 2^46 2^-344
NAMES = ["sum_p", "sum_q", "pq", "pp", "qq"]


def d2_of(pos, partner):
    """(valid, d2): valid where j < N and all six coordinates are finite; d2 float32[N] (0 where not valid)."""
    p = np.ascontiguousarray(np.asarray(pos, F)[:, :3])
    n = p.shape[0]
    j = np.asarray(partner, np.uint32).astype(np.int64)
    valid = j < n
    q = p[np.where(valid, j, 0)]
    valid &= np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1)
    with np.errstate(all="ignore"):
        d = q - p
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == F
    return valid, np.where(valid, d2, F(0)), q


def _ints(v):
    """A finite float32 array as (integer mantissas, exponents): v = M 2^E exactly."""
    m, e = np.frexp(v.astype(np.float64))
    M = (m * 2.0 ** 24).astype(np.int64)
    assert (M.astype(np.float64) == m * 2.0 ** 24).all()
    return M, e.astype(np.int64) - 24


def columns(pos, partner):
    """(valid, d2, cols): cols[t][i] the term of quantity t (sum_p[3], sum_q[3], pq[9], pp[3], qq[3]) of splat i as a Python integer
    in units of 2^-UNIT, 0 where the splat is not valid."""
    p = np.ascontiguousarray(np.asarray(pos, F)[:, :3])
    valid, d2, q = d2_of(p, partner)
    pz, qz = np.where(valid[:, None], p, F(0)), np.where(valid[:, None], q, F(0))
    pm, pe, qm, qe = [], [], [], []
    for a in range(3):
        M, E = _ints(pz[:, a])
        pm.append([int(x) for x in M]), pe.append([int(x) + UNIT for x in E])
        M, E = _ints(qz[:, a])
        qm.append([int(x) for x in M]), qe.append([int(x) + UNIT for x in E])
    one = lambda m, e: [x << s for x, s in zip(m, e)]  # noqa: E731
    two = lambda m1, e1, m2, e2: [(x * y) << (s + t - UNIT) for x, s, y, t in zip(m1, e1, m2, e2)]  # noqa: E731
    cols = [one(pm[a], pe[a]) for a in range(3)] + [one(qm[a], qe[a]) for a in range(3)]
    cols += [two(pm[a], pe[a], qm[b], qe[b]) for a in range(3) for b in range(3)]
    cols += [two(pm[a], pe[a], pm[a], pe[a]) for a in range(3)] + [two(qm[a], qe[a], qm[a], qe[a]) for a in range(3)]
    return valid, d2, cols


def record(cols_of, keep=None, max_d2=np.inf):
    """The dict of register.pair_moments from columns(): the splats with keep (None: all), valid and d2 <= max_d2 are paired."""
    valid, d2, cols = cols_of
    n = valid.size
    keep = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    with np.errstate(all="ignore"):
        paired = keep & valid & (d2 <= F(max_d2))
    idx = [int(i) for i in np.flatnonzero(paired)]
    s = [mr.pair(Fraction(sum(c[i] for i in idx), 1 << UNIT)) for c in cols]
    return {"matched": int(keep.sum()), "paired": len(idx), "sum_p": s[0:3], "sum_q": s[3:6], "pq": [s[6 + 3 * a:9 + 3 * a] for a in range(3)],
            "pp": s[15:18], "qq": s[18:21]}


def restate(pos, partner, keep=None, max_d2=np.inf):
    return record(columns(pos, partner), keep, max_d2)


def by_fractions(pos, partner, keep=None, max_d2=np.inf):
    """The same record term by term with Fraction(float(v)) -- slow; what pins the integer columns above."""
    p = np.ascontiguousarray(np.asarray(pos, F)[:, :3])
    valid, d2, q = d2_of(p, partner)
    keep = np.ones(valid.size, bool) if keep is None else np.asarray(keep, bool)
    with np.errstate(all="ignore"):
        idx = np.flatnonzero(keep & valid & (d2 <= F(max_d2)))
    P = [[Fraction(float(v)) for v in p[idx, a]] for a in range(3)]
    Q = [[Fraction(float(v)) for v in q[idx, a]] for a in range(3)]
    tot = lambda it: mr.pair(sum(it, Fraction(0)))  # noqa: E731
    return {"matched": int(keep.sum()), "paired": int(idx.size), "sum_p": [tot(P[a]) for a in range(3)], "sum_q": [tot(Q[a]) for a in range(3)],
            "pq": [[tot(x * y for x, y in zip(P[a], Q[b])) for b in range(3)] for a in range(3)],
            "pp": [tot(x * x for x in P[a]) for a in range(3)], "qq": [tot(x * x for x in Q[a]) for a in range(3)]}


def flat(m):
    return list(m["sum_p"]) + list(m["sum_q"]) + [m["pq"][a][b] for a in range(3) for b in range(3)] + list(m["pp"]) + list(m["qq"])


def same(got, want):
    """Bit for bit: both counts, and hi and lo of the 21 entries as uint64."""
    if (got["matched"], got["paired"]) != (want["matched"], want["paired"]):
        return False
    return all(mr.bits(a[0]) == mr.bits(b[0]) and mr.bits(a[1]) == mr.bits(b[1]) for a, b in zip(flat(got), flat(want)))


def as_bytes(want):
    """The 352 bytes of the record."""
    from gsplat import _abi
    rec = _abi.GsPairMoments()
    rec.matched, rec.paired = want["matched"], want["paired"]
    e = (_abi.GsExact * 21).from_buffer(rec, 16)
    for t, (hi, lo) in enumerate(flat(want)):
        e[t].hi, e[t].lo = hi, lo
    return bytes(rec)


# ---- the scenes: (n, 3) float32 positions, seeded -----------------------------------------------------------------------------------------
def with_duplicates(pos):
    """Every tenth splat (5, 15, ...) sits exactly on its predecessor: d2 = +0.0 occurs."""
    out = np.array(pos, F, copy=True)
    out[5::10] = out[4:out.shape[0] - 1:10]
    return out


def far(n, seed=21):
    """Extent 1 at the offset 1e4: the centroid costs a float sum its digits."""
    rng = np.random.default_rng(seed)
    return with_duplicates((1.0e4 + rng.random((n, 3))).astype(F))


def spread(n, seed=22):
    """Exponents uniform in 2^-60 .. 2^60 with random signs: the products span limbs, d2 stays finite (3 x 2^122)."""
    rng = np.random.default_rng(seed)
    v = (1.0 + rng.random((n, 3))) * 2.0 ** rng.integers(-60, 60, size=(n, 3)) * rng.choice([-1.0, 1.0], size=(n, 3))
    return with_duplicates(v.astype(F))


PARTNERS = ("nearest", "none", "one", "self", "beyond", "perm")


def partner(kind, pos, seed=23):
    """uint32[n] of one partner kind."""
    n = pos.shape[0]
    rng = np.random.default_rng(seed + n)
    if kind == "nearest":
        return knn_restate.planes(pos, 1, np.inf)[1]
    if kind == "none":
        return np.full(n, NONE, np.uint32)
    if kind == "one":
        return np.full(n, n // 2, np.uint32)
    if kind == "self":
        return np.arange(n, dtype=np.uint32)
    out = rng.permutation(n).astype(np.uint32)
    if kind == "beyond":  # ids at and past N among valid ones: N itself, N + 1, 2^31, the largest below NONE, NONE
        out[0::3] = np.resize(np.array([n, n + 1, 1 << 31, NONE - 1, NONE], np.uint64), out[0::3].size).astype(np.uint32)
    return out


# ---- the step, restated --------------------------------------------------------------------------------------------------------------------
def masks(st, moving, fixed):
    st = np.asarray(st, np.uint8)
    return (st & moving[0]) == moving[1], (st & fixed[0]) == fixed[1]


def step(rec, st, radius, moving=(2, 2), fixed=(2, 0), max_dist=None, scale=False):
    """(records after the step, the fit, the nearest plane): brute-force nearest of the moving splats among the fixed ones within
    `radius`, the pairs within max_dist (None: the radius), register.fit, xform_restate.apply of register.xform_of on the moving
    splats.  A ValueError of the fit propagates."""
    from gsplat import register
    rec = np.ascontiguousarray(rec, dtype=F)
    mov, fix = masks(st, moving, fixed)
    _, near, _ = knn_restate.planes(rec, 1, radius, src=fix, qry=mov)
    md = F(radius if max_dist is None else max_dist)
    with np.errstate(all="ignore"):
        m = restate(rec[:, :3], near, mov, md * md)
    f = register.fit(m, scale)
    out = xr.apply(rec, xr.Xform.from_struct(register.xform_of(f)), mov)
    return out, f, near


def align(rec, st, radius, moving=(2, 2), fixed=(2, 0), max_iters=30, tol=1e-6, trim=3.0, scale=False):
    """register.align's loop on the restated step: (final records, [(paired, rms bits, radius, max_dist)])."""
    steps, prev = [], None
    for _ in range(max_iters):
        md = float(radius) if prev is None else min(float(radius), float(trim) * prev)
        try:
            rec, f, _ = step(rec, st, radius, moving, fixed, md, scale)
        except ValueError:
            break
        steps.append((f["paired"], mr.bits(f["rms"]), float(radius), md))
        if prev is not None and abs(f["rms"] - prev) <= tol * prev:
            break
        prev = f["rms"]
    return rec, steps
