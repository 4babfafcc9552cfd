"""numpy restatement of the splat attributes (include/gsplat/gs_abi.h "splat attributes"): the value of a splat, the summary with
its key order, the histogram's bin rule and the selection's membership.  TEST INFRASTRUCTURE ONLY.

Every float expression is evaluated in f32 with one rounding per operation, in the order the header fixes, so that the GPU
kernels (k_attr.hip) can be held to it bit for bit.  The CPU tests of test_attributes.py pin it to what already exists: the
upload's smax expression, state_restate's projection depth and its SPHERE membership.
"""
import numpy as np

F = np.float32
(POS_X, POS_Y, POS_Z, OPACITY_LOGIT, LOG_SCALE_MIN, LOG_SCALE_MAX, LOG_SCALE_SUM, ANISOTROPY, DC_R, DC_G, DC_B, DIST2, PLANE,
 COVER_HITS, COVER_MAX_WEIGHT, COVER_SUM, COUNT) = range(17)
SCENE_KINDS = tuple(range(COVER_HITS))
COVER_KINDS = (COVER_HITS, COVER_MAX_WEIGHT, COVER_SUM)
ZERO_SIGN_OPEN = (LOG_SCALE_MIN, LOG_SCALE_MAX, ANISOTROPY)  # fminf / fmaxf may pick either of -0 and +0


def value(kind, records, p=(0, 0, 0, 0), cov=None):
    """f32[N]: the value of every record (float32 [N, 80] as uploaded); cov: the coverage planes (sum_q, hits, max_weight) for the
    COVER_* kinds."""
    s = np.ascontiguousarray(records, dtype=F).reshape(-1, 80)
    p = [F(v) for v in p] + [F(0)] * (4 - len(p))
    with np.errstate(all="ignore"):
        if kind in (POS_X, POS_Y, POS_Z):
            return s[:, kind - POS_X].copy()
        if kind == OPACITY_LOGIT:
            return s[:, 12].copy()
        l0, l1, l2 = s[:, 4], s[:, 5], s[:, 6]
        if kind == LOG_SCALE_MAX:
            return np.fmax(l0, np.fmax(l1, l2))
        if kind == LOG_SCALE_MIN:
            return np.fmin(l0, np.fmin(l1, l2))
        if kind == LOG_SCALE_SUM:
            return (l0 + l1) + l2
        if kind == ANISOTROPY:
            return np.fmax(l0, np.fmax(l1, l2)) - np.fmin(l0, np.fmin(l1, l2))
        if kind in (DC_R, DC_G, DC_B):
            return s[:, 16 + kind - DC_R].copy()
        x, y, z = s[:, 0], s[:, 1], s[:, 2]
        if kind == DIST2:
            dx, dy, dz = x - p[0], y - p[1], z - p[2]
            return (dx * dx + dy * dy) + dz * dz
        if kind == PLANE:
            return ((p[0] * x + p[1] * y) + p[2] * z) + p[3]
        if kind == COVER_HITS:
            return cov["hits"].astype(F)  # (u32 -> f32: round to nearest even, as the device's conversion)
        if kind == COVER_MAX_WEIGHT:
            return cov["max_weight"].astype(F)
        if kind == COVER_SUM:
            q = cov["sum_q"].astype(np.uint64)
            return (q >> np.uint64(32)).astype(np.uint32).astype(F) + (q & np.uint64(0xFFFFFFFF)).astype(np.uint32).astype(F) * F(2.0 ** -32)
    raise ValueError(kind)


def keys(v):
    """The order-preserving map of the bit pattern: k = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000); unsigned order of the keys is
    -inf < ... < -0 < +0 < ... < +inf."""
    b = np.ascontiguousarray(v, dtype=F).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.uint32(k)
    b = (k ^ np.uint32(0x80000000)) if (k >> np.uint32(31)) else np.uint32(~k & np.uint32(0xFFFFFFFF))
    return np.array([b], np.uint32).view(F)[0]


def summary(v, keep=None):
    """{"matched", "nan", "min", "max"} of the values v[keep] (keep: bool[N] or None for all)."""
    v = np.ascontiguousarray(v, dtype=F)
    if keep is not None:
        v = v[keep]
    nan = np.isnan(v)
    k = keys(v[~nan])
    lo, hi = (unkey(k.min()), unkey(k.max())) if k.size else (F(np.inf), F(-np.inf))
    return {"matched": int(v.size), "nan": int(nan.sum()), "min": lo, "max": hi}


def bin_of(v, lo, hi, bins):
    """int64[N]: the slot of every value among bins + 3: [0, bins) the bins, bins below, bins + 1 above, bins + 2 NaN.  The
    conversion saturates (a NaN product, which only an infinite scale makes, is bin 0)."""
    v = np.ascontiguousarray(v, dtype=F)
    lo, hi = F(lo), F(hi)
    with np.errstate(all="ignore"):
        scale = F(bins) / (hi - lo)
        t = (v - lo) * scale
    inb = ~np.isnan(v) & ~(v < lo) & ~(v >= hi)
    b = np.zeros(v.size, np.int64)
    ok = inb & ~np.isnan(t)
    b[ok] = np.minimum(np.floor(np.minimum(t[ok], F(4294967040.0)).astype(np.float64)).astype(np.int64), bins - 1)
    out = np.where(np.isnan(v), bins + 2, np.where(v < lo, bins, np.where(v >= hi, bins + 1, b)))
    return out.astype(np.int64)


def histogram(v, lo, hi, bins, keep=None):
    """uint64[bins + 3] over v[keep]."""
    v = np.ascontiguousarray(v, dtype=F)
    if keep is not None:
        v = v[keep]
    return np.bincount(bin_of(v, lo, hi, bins), minlength=bins + 3).astype(np.uint64)


def select(v, lo, hi, inside=True):
    """bool[N]: (v >= lo && v <= hi) == inside; a NaN is in no range.  Goes through state_restate.apply_region like a region's
    membership."""
    v = np.ascontiguousarray(v, dtype=F)
    with np.errstate(all="ignore"):
        return ((v >= F(lo)) & (v <= F(hi))) == bool(inside)


def same_values(got, want, kind):
    """Bit for bit, apart from the two documented exceptions: NaN on both sides; and, for the kinds in ZERO_SIGN_OPEN, the sign of a zero."""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    if got.shape != want.shape:
        return False
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if kind in ZERO_SIGN_OPEN:
        ok |= (got == 0) & (want == 0)
    return bool(ok.all())
