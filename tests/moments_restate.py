"""The moments (gs_abi.h "moments") restated with fractions.Fraction, and the scenes the tests run them on.

Per quantity: S = sum of Fraction(float(v)) (or of products of two), hi = float(S) -- Python rounds a Fraction to the nearest
double, ties to even --, lo = float(S - Fraction(hi)).  A splat with a non-finite value in ANY of the planes is in no sum."""
import math
from fractions import Fraction

import numpy as np

F = np.float32
LENGTHS = (1, 3, 4, 5, 1023, 1024, 1025, 3001)
# the first and last lane, the ends of a quad, the wave and workgroup edges, the last partial quad (of 1043 = 3 mod 4)
EDGES = (0, 3, 63, 64, 255, 256, 1023, 1024, 1042)
PROD = ((0, 1, 2), (1, 3, 4), (2, 4, 5))


def pair(S):
    hi = float(S)
    return hi, float(S - Fraction(hi))


def bits(x):
    return int(np.float64(x).view(np.uint64))


def restate(planes, keep=None):
    """The record of moments.moments / host_moments for float32 planes and a boolean filter: the same dict."""
    planes = [np.asarray(p, dtype=F) for p in planes]
    n = planes[0].size
    keep = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    fin = keep.copy()
    for p in planes:
        fin &= np.isfinite(p)
    cols = [[Fraction(float(v)) for v in p[fin]] for p in planes]
    k = len(planes)
    zero = (0.0, 0.0)
    out = {"matched": int(keep.sum()), "counted": int(fin.sum()), "sum": [zero] * 3, "prod": [[zero] * 3 for _ in range(3)]}
    for j in range(k):
        out["sum"][j] = pair(sum(cols[j], Fraction(0)))
        for l in range(j, k):
            out["prod"][j][l] = out["prod"][l][j] = pair(sum((a * b for a, b in zip(cols[j], cols[l])), Fraction(0)))
    return out


def same(got, want):
    """Bit for bit: the counts, and hi and lo of every entry as uint64."""
    if (got["matched"], got["counted"]) != (want["matched"], want["counted"]):
        return False
    g = [got["sum"][j] for j in range(3)] + [got["prod"][j][l] for j in range(3) for l in range(3)]
    w = [want["sum"][j] for j in range(3)] + [want["prod"][j][l] for j in range(3) for l in range(3)]
    return all(bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1]) for a, b in zip(g, w))


def check_against_fsum(planes, keep=None, products=True):
    """The restatement against a second implementation: hi == math.fsum of the float64 values (and of the float64 products, which
    are exact) + 0.0.  Only where no product leaves float64's range downwards (a product below 2^-1074 is not a double)."""
    want = restate(planes, keep)
    planes = [np.asarray(p, dtype=F).astype(np.float64) for p in planes]
    n = planes[0].size
    fin = np.ones(n, bool) if keep is None else np.asarray(keep, bool).copy()
    for p in planes:
        fin &= np.isfinite(p)
    for j, p in enumerate(planes):
        assert bits(want["sum"][j][0]) == bits(math.fsum(p[fin]) + 0.0)
        for l in range(j, len(planes) if products else 0):
            assert bits(want["prod"][j][l][0]) == bits(math.fsum(p[fin] * planes[l][fin]) + 0.0)


# ---- the rules of gsplat.moments, restated ---------------------------------------------------------------------------------------------
def mean(values):
    v = [Fraction(float(x)) for x in np.asarray(values, F) if np.isfinite(x)]
    hi, lo = pair(sum(v, Fraction(0)))
    return float((Fraction(hi) + Fraction(lo)) / len(v))


def covariance(a, b):
    """RN((P - Sa Sb / n) / n) with P, Sa, Sb as the record holds them (hi + lo)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    fin = np.isfinite(a) & np.isfinite(b)
    fa, fb = [Fraction(float(x)) for x in a[fin]], [Fraction(float(x)) for x in b[fin]]
    held = lambda S: sum((Fraction(x) for x in pair(S)), Fraction(0))  # noqa: E731
    n = len(fa)
    P, Sa, Sb = held(sum((x * y for x, y in zip(fa, fb)), Fraction(0))), held(sum(fa, Fraction(0))), held(sum(fb, Fraction(0)))
    return float((P - Sa * Sb / n) / n)


# ---- the scenes: (n, 3) float32 positions, seeded ----------------------------------------------------------------------------------------
def third(n):
    """test_attributes._third: host bit 0x04 on every third splat, junk in bits 0, 1, 4, 5 and 6."""
    st = ((np.arange(n) * 7) & 0x73).astype(np.uint8)
    st[np.arange(n) % 3 == 0] |= 0x04
    return st


THIRD = (0x04, 0x04)
NOTHING = (0x08, 0x08)  # bit 3 is clear in third(): matches nothing
FILTERS = ((0, 0), THIRD, NOTHING)


def keep_of(where, st):
    return None if where == (0, 0) else (st & where[0]) == where[1]


def wild(n, seed=11):
    """Every coordinate a random finite f32 bit pattern; denormals, +-0, +-FLT_MAX and 2^-149 among them.  Nearly every lane
    disagrees about its limb."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 32, size=(n, 3), dtype=np.uint64).astype(np.uint32)
    w[(w & 0x7F800000) == 0x7F800000] &= np.uint32(0xBF7FFFFF)  # exponent 255 -> finite
    special = np.array([0x00000001, 0x80000001, 0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x007FFFFF, 0x00800000, 0x807FFFFF], np.uint32)
    flat = w.reshape(-1)
    at = rng.permutation(flat.size)[:min(flat.size, 3 * special.size)]
    flat[at] = np.resize(special, at.size)
    return np.ascontiguousarray(w.view(F))


def cancel(n, seed=0):
    """Repeats of (3e38, 1, -3e38, 2^-149, -1, ...): the true sums are tiny beside the terms."""
    base = np.array([3e38, 1.0, -3e38, 2.0 ** -149, -1.0, 3e38, -2.0 ** -149, -3e38, 0.5, 2.0 ** -126], F)
    out = np.empty((n, 3), F)
    for k in range(3):
        out[:, k] = np.resize(np.roll(base, k), n)
    return out


def outlier(seed=5):
    """1043 splats in [1, 2) with single values of 2^100 and 2^-140 at EDGES."""
    rng = np.random.default_rng(seed)
    out = (1.0 + rng.random((1043, 3))).astype(F)
    out[out >= 2] = F(1.5)
    for t, i in enumerate(EDGES):
        out[i, t % 3] = F(2.0 ** 100) if t % 2 == 0 else F(2.0 ** -140)
    return out


def nonfinite(seed=5):
    """outlier()'s base with NaN, +inf or -inf in ONE coordinate of the splats at EDGES, and large finite values in their other
    coordinates, which must be in no sum."""
    rng = np.random.default_rng(seed)
    out = (1.0 + rng.random((1043, 3))).astype(F)
    for t, i in enumerate(EDGES):
        out[i] = F(1e30)
        out[i, (t // 3) % 3] = (np.nan, np.inf, -np.inf)[t % 3]
    return out


def ties():
    """Sets whose sum is exactly halfway between two doubles, with what hi and lo must be (as Fractions of the set's scale)."""
    out = []
    for sign in (1, -1):
        for shift in (0, 40, -40):
            s = 2.0 ** shift * sign
            out.append(([2.0 ** 53 * s, 1.0 * s], 2.0 ** 53 * s, 1.0 * s))
            out.append(([2.0 ** 53 * s, 1.0 * s, 2.0 * s], (2.0 ** 53 + 4) * s, -1.0 * s))
    return out


def planted_plane(n=2000, seed=3, noise=1e-3):
    """n points on z = 0.3 x - 0.2 y + 1 with seeded noise along z."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-2, 2, size=(n, 2))
    z = 0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 1 + rng.normal(0, noise, n)
    return np.ascontiguousarray(np.column_stack([xy, z]).astype(F))
