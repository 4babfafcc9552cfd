"""The consensus calls (gs_abi.h "consensus") restated: the value matrix of h hypotheses over n positions in numpy f32 with one
rounding per operation, the counts as sums over it, gs_planes_through in Python floats, and the samplers of gsplat.consensus
(find_plane, select_plane, detect_planes, densest_ball) on host positions and a host state plane."""
import math

import numpy as np

F = np.float32
PLANE, DIST2 = 12, 11  # GS_ATTR_PLANE, GS_ATTR_DIST2
LENGTHS = (0, 1, 3, 4, 5, 1023, 1024, 1025, 4099)
HYPOTHESES = (1, 2, 63, 64, 65, 4096)
SELECTED = 2


def values(pos, kind, params):
    """float32[n][h]: v_j(i), attr_of_pos's expression, every operation rounded once to f32."""
    pos, p = np.asarray(pos, F).reshape(-1, 3), np.asarray(params, F).reshape(-1, 4)
    x, y, z = (pos[:, a][:, None] for a in range(3))
    with np.errstate(all="ignore"):
        if kind == DIST2:
            dx, dy, dz = x - p[None, :, 0], y - p[None, :, 1], z - p[None, :, 2]
            return (dx * dx + dy * dy) + dz * dz
        return ((p[None, :, 0] * x + p[None, :, 1] * y) + p[None, :, 2] * z) + p[None, :, 3]


def counts_of(v, lo, hi, keep=None):
    """(counts uint64[h], matched) from a value matrix: lo <= v <= hi, both inclusive, a NaN in no range."""
    n = v.shape[0]
    keep = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    with np.errstate(invalid="ignore"):
        inside = (v >= F(lo)) & (v <= F(hi))
    return (inside & keep[:, None]).sum(axis=0).astype(np.uint64), int(keep.sum())


def score(pos, kind, params, lo, hi, keep=None):
    return counts_of(values(pos, kind, params), lo, hi, keep)


def plane_through(pt):
    """gs_planes_through of one triple (nine f32 values) in Python floats, operation by operation; four f32."""
    a, b, c = ([float(F(v)) for v in pt[3 * k:3 * k + 3]] for k in range(3))
    with np.errstate(all="ignore"):
        u = [np.float64(b[k]) - np.float64(a[k]) for k in range(3)]
        w = [np.float64(c[k]) - np.float64(a[k]) for k in range(3)]
        n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
        len2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        length = np.sqrt(len2)
        if not (np.isfinite(length) and length > 0.0):
            return np.full(4, np.nan, F)
        m = [n[k] / length for k in range(3)]
        d = -((m[0] * a[0] + m[1] * a[1]) + m[2] * a[2])
        big = 0
        for k in (1, 2):
            if abs(m[k]) > abs(m[big]):
                big = k
        if m[big] < 0.0:
            m, d = [-v for v in m], -d
        return np.array(m + [d], np.float64).astype(F)


def planes_through(points):
    pts = np.asarray(points, F).reshape(-1, 9)
    return np.array([plane_through(t) for t in pts], F).reshape(-1, 4)


def same_bits(a, b):
    """float32 arrays equal bit for bit, a NaN on both sides counting as equal (gs_abi.h: a NaN's sign and payload are open)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | nan).all())


def plane_params(normal, offset):
    m, d = [float(v) for v in normal], float(offset)
    big = 0
    for k in (1, 2):
        if abs(m[k]) > abs(m[big]):
            big = k
    if m[big] < 0.0:
        m, d = [-v for v in m], -d
    return np.array(m + [d], F)


# ---- the samplers, on host positions and a host state plane; scorer(pos, kind, params, lo, hi, keep) -> (counts, matched) -------------
def keep_of(where, state, n):
    if tuple(where) == (0, 0):
        return np.ones(n, bool)
    return (np.asarray(state, np.uint8) & where[0]) == where[1]


def find_plane(pos, distance, trials=1024, seed=0, state=None, where=(0, 0), scorer=score):
    pos = np.asarray(pos, F).reshape(-1, 3)
    keep = keep_of(where, state, pos.shape[0])
    pool = np.flatnonzero(keep)
    if not pool.size:
        return None
    draws = np.random.default_rng(seed).integers(0, pool.size, (trials, 3))
    params = planes_through(pos[pool[draws].reshape(-1)].reshape(trials, 9))
    d = F(distance)
    counts, matched = scorer(pos, PLANE, params, -d, d, keep)
    j = int(np.argmax(counts))
    if int(counts[j]) < 3:
        return None
    return {"plane": params[j].copy(), "count": int(counts[j]), "matched": matched, "trial": j}


def fit_plane(pos, keep):
    """moments.fit_plane over pos[keep] through gs_moments_host (the exact sums) and the module's own rules."""
    from gsplat import moments
    pos = np.asarray(pos, F).reshape(-1, 3)
    m = moments.host_moments([np.ascontiguousarray(pos[:, a]) for a in range(3)], keep.astype(np.uint8), (1, 1))
    w, axes = moments._axes(m, "fit_plane")
    c = np.array([moments.mean_of(m, j) for j in range(3)], dtype=np.float64)
    return axes[2], -float(np.dot(axes[2], c))


def select_plane(pos, state, distance, trials=1024, seed=0, where=(0, 0), refine=2, scorer=score):
    """(record or None, the new state plane)."""
    pos, state = np.asarray(pos, F).reshape(-1, 3), np.array(state, np.uint8, copy=True)
    f = find_plane(pos, distance, trials, seed, state, where, scorer)
    if f is None:
        return None, state
    keep = keep_of(where, state, pos.shape[0])
    d = F(distance)

    def reselect(plane):
        with np.errstate(invalid="ignore"):
            v = values(pos, PLANE, plane)[:, 0]
            mask = keep & (v >= -d) & (v <= d)
        state[keep] &= np.uint8(0xFF ^ SELECTED)
        state[mask] |= np.uint8(SELECTED)
        return int(mask.sum())

    plane, rounds = f["plane"], 0
    count = reselect(plane)
    for _ in range(refine):
        sel = keep & ((state & SELECTED) != 0)
        try:
            normal, offset = fit_plane(pos, sel)
        except ValueError:
            break
        cand = plane_params(normal, offset)
        c, _ = scorer(pos, PLANE, cand[None, :], -d, d, keep)
        if int(c[0]) < count:
            break
        plane = cand
        count = reselect(plane)
        rounds += 1
    return {"plane": plane, "count": count, "matched": f["matched"], "trial": f["trial"], "refined": rounds}, state


def detect_planes(pos, state, distance, max_planes=8, min_inliers=None, trials=1024, seed=0, where=(0, 0), scratch_bit=0x80, refine=2, scorer=score):
    """(records, the new state plane)."""
    pos, state = np.asarray(pos, F).reshape(-1, 3), np.array(state, np.uint8, copy=True)
    m, v, sb = where[0], where[1], scratch_bit
    if min_inliers is None:
        min_inliers = max(3, int(keep_of(where, state, pos.shape[0]).sum()) // 20)
    d = F(distance)
    rest = (m | sb, v)
    out = []
    for k in range(max_planes):
        g, state = select_plane(pos, state, distance, trials, seed + k, rest, refine, scorer)
        if g is None or g["count"] < min_inliers:
            break
        with np.errstate(invalid="ignore"):
            val = values(pos, PLANE, g["plane"])[:, 0]
            state[keep_of(rest, state, pos.shape[0]) & (val >= -d) & (val <= d)] |= np.uint8(sb)
        out.append(g)
    state[keep_of((m | sb, v), state, pos.shape[0])] &= np.uint8(0xFF ^ SELECTED)
    marked = keep_of((m | sb, v | sb), state, pos.shape[0])
    state[marked] |= np.uint8(SELECTED)
    state[marked] &= np.uint8(0xFF ^ sb)
    return out, state


def densest_ball(pos, radius, trials=1024, seed=0, state=None, where=(0, 0), scorer=score):
    pos = np.asarray(pos, F).reshape(-1, 3)
    keep = keep_of(where, state, pos.shape[0])
    pool = np.flatnonzero(keep)
    if not pool.size:
        return None
    centres = pos[pool[np.random.default_rng(seed).integers(0, pool.size, trials)]]
    params = np.concatenate([centres, np.zeros((trials, 1), F)], axis=1)
    r = F(radius)
    with np.errstate(all="ignore"):
        r2 = F(r * r)
    counts, _ = scorer(pos, DIST2, params, -math.inf, r2, keep)
    j = int(np.argmax(counts))
    return centres[j].copy(), int(counts[j])


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------
def with_specials(pos):
    """A copy with NaN, +-inf, denormals, -0 and the largest finite value in single coordinates of the first splats and of the last
    one."""
    out = np.array(pos, F, copy=True)
    w = out.view(np.uint32)
    vals = (0x7FC00000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0xFFC0BEEF)
    n = out.shape[0]
    for k, b in enumerate(vals):
        if n:
            w[(k * 5) % n, k % 3] = b
    if n:
        w[n - 1, 1] = 0x7FC00000
    return out


def with_duplicates(pos):
    """A copy in which every tenth splat repeats its predecessor exactly."""
    out = np.array(pos, F, copy=True)
    i = np.arange(5, out.shape[0], 10)
    out[i] = out[i - 1]
    return out


def hypotheses(pos, kind, h, seed=7):
    """float32[h][4]: planes through random triples of the scene (PLANE) or centres at random splats, some nudged (DIST2); then a
    NaN, a +inf and a -inf parameter in hypotheses 1, 2, 3 where h reaches them, and a hypothesis of zeros."""
    rng = np.random.default_rng(seed)
    n = max(pos.shape[0], 1)
    base = np.asarray(pos, F).reshape(-1, 3) if pos.shape[0] else np.zeros((1, 3), F)
    fin = np.where(np.isfinite(base), base, F(0.25))
    if kind == PLANE:
        p = planes_through(fin[rng.integers(0, n, (h, 3))].reshape(h, 9))
        p[np.isnan(p)] = F(0.5)
    else:
        p = np.concatenate([fin[rng.integers(0, n, h)], rng.normal(size=(h, 1)).astype(F)], axis=1)
    p = np.ascontiguousarray(p, F)
    for j, (k, b) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf)), start=1):
        if j < h:
            p[j, k] = b
    if h > 4:
        p[4] = 0
    return p


def planted(n=4000, share=0.4, sigma=0.01, seed=1):
    """(positions float32[n][3], unit normal, offset, planted inlier mask): `share` of the points on a tilted plane with Gaussian
    noise sigma along the normal, the rest uniform in the box [-2, 2]^3."""
    rng = np.random.default_rng(seed)
    normal = np.array([0.3, -0.5, 0.81])
    normal /= np.linalg.norm(normal)
    offset = -0.4
    k = int(n * share)
    e1 = np.cross(normal, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(normal, e1)
    uv = rng.uniform(-2, 2, (k, 2))
    on = uv[:, :1] * e1 + uv[:, 1:] * e2 - offset * normal + rng.normal(0, sigma, (k, 1)) * normal
    box = rng.uniform(-2, 2, (n - k, 3))
    pos = np.concatenate([on, box]).astype(F)
    order = rng.permutation(n)
    mask = np.zeros(n, bool)
    mask[:k] = True
    return np.ascontiguousarray(pos[order]), normal, offset, mask[order]


def two_planes(n=3000, sigma=0.005, seed=2):
    """float32[n][3]: 40 % on a tilted plane, 30 % on z = -1, the rest uniform in the box; every tenth splat a duplicate, one NaN."""
    rng = np.random.default_rng(seed)
    a, _, _, _ = planted(int(n * 0.4), 1.0, sigma, seed)
    k = int(n * 0.3)
    b = np.column_stack([rng.uniform(-2, 2, (k, 2)), -1.0 + rng.normal(0, sigma, k)]).astype(F)
    c = rng.uniform(-2, 2, (n - a.shape[0] - k, 3)).astype(F)
    pos = np.concatenate([a, b, c])[rng.permutation(n)]
    pos = with_duplicates(pos)
    pos[17, 1] = np.nan
    return np.ascontiguousarray(pos, F)
