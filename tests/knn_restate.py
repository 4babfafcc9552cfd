"""The nearest-neighbour planes of include/gsplat/gs_abi.h "nearest neighbours", restated in numpy: the definition the GPU is held to.

A blockwise brute force over all pairs, like neigh_restate.counts, with exactly the header's f32 expression: d = p_j - p_i per
component, d2 = (dx dx + dy dy) + dz dz (every operation rounded once to f32: numpy float32 arithmetic does that), accepted when
d2 <= r2 with r2 = radius * radius as ONE f32 product and j != i by index.  Rejected pairs are set to +inf, then every row is sorted
along the source axis (a partition to the largest k asked for, then a sort of those: the same k smallest values): dist2 is the
k-th entry, +inf when fewer than k were accepted.  The sources run in ascending id, so argmin -- the FIRST minimum -- is the tie
rule: the smallest id at the smallest d2; NONE when the row's minimum is +inf.  A NaN or infinite coordinate makes the comparison
false (inf - inf and 0 * inf are NaN, inf * inf is inf > r2).  A splat that is no query reads NaN 0x7FC00000 / NONE.  No GPU, no grid."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
INF_BITS, NAN_BITS = 0x7F800000, 0x7FC00000


def planes_multi(pos, ks, radius, src=None, qry=None, block=512):
    """{k: (dist2 float32[N], nearest uint32[N], unresolved)} for every k of ks, from one pass over the pairs.  pos: [N, 3] (or
    records [N, 80]: the first three floats); src / qry: boolean masks, None = every splat; unresolved: the queries that read +inf."""
    p = np.ascontiguousarray(np.asarray(pos, dtype=F)[:, :3])
    n = p.shape[0]
    src = np.ones(n, bool) if src is None else np.asarray(src, bool)
    qry = np.ones(n, bool) if qry is None else np.asarray(qry, bool)
    ks = [int(k) for k in ks]
    r2 = F(radius) * F(radius)
    js = np.flatnonzero(src)
    kmax = min(max(ks), js.size)
    head = np.full((n, max(max(ks), 1)), np.inf, F)  # the k smallest accepted d2 of every row, ascending
    near = np.full(n, NONE, np.uint32)
    with np.errstate(all="ignore"):
        for i0 in range(0, n, block):
            i = np.arange(i0, min(n, i0 + block))
            if not js.size:
                break
            d = p[js][None, :, :] - p[i][:, None, :]  # p_j - p_i
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert d2.dtype == F
            ok = (d2 <= r2) & (js[None, :] != i[:, None])
            d2 = np.where(ok, d2, F(np.inf))
            first = d2.argmin(axis=1)  # the first minimum: ascending source ids
            near[i] = np.where(d2[np.arange(i.size), first] < np.inf, js[first], NONE).astype(np.uint32)
            part = np.partition(d2, kmax - 1, axis=1)[:, :kmax]
            part.sort(axis=1)
            head[i, :kmax] = part
    out = {}
    for k in ks:
        d2k = np.array(head[:, k - 1], F)
        nr = near.copy()
        d2k.view(np.uint32)[~qry] = NAN_BITS
        nr[~qry] = NONE
        out[k] = (d2k, nr, int((d2k.view(np.uint32)[qry] == INF_BITS).sum()))
    return out


def planes(pos, k, radius, src=None, qry=None, block=512):
    """(dist2 float32[N], nearest uint32[N], unresolved) of one search."""
    return planes_multi(pos, (k,), radius, src, qry, block)[int(k)]


def refine(prev, pos, k, radius, src=None, qry=None):
    """The REFINE rule as a function of the previous planes prev = (dist2, nearest): the queries are further restricted to the
    splats whose dist2 reads +inf in prev, only their two entries are written.  Returns (dist2, nearest, queried, unresolved), the
    last two of this call's queries only."""
    pd, pn = np.array(prev[0], F, copy=True), np.array(prev[1], np.uint32, copy=True)
    n = pd.shape[0]
    qry = np.ones(n, bool) if qry is None else np.asarray(qry, bool)
    gate = qry & (pd.view(np.uint32) == INF_BITS)
    d2, nr, unresolved = planes(pos, k, radius, src, gate)
    pd[gate], pn[gate] = d2[gate], nr[gate]
    return pd, pn, int(gate.sum()), unresolved


def member(d2, lo, hi, inside=True):
    """gs_state_knn's membership: (v >= lo && v <= hi) == inside on the f32 value; a NaN is in no range."""
    v = np.asarray(d2, F)
    with np.errstate(all="ignore"):
        return ((v >= F(lo)) & (v <= F(hi))) == bool(inside)


def outlier_threshold(d2, sigma):
    """select_outliers' lower bound: the float32 above float32(mean + sigma * std)^2 of sqrt(dist2) over the finite values, in
    float64 on the host (+inf when there is none)."""
    v = np.asarray(d2, F)
    d = np.sqrt(v[np.isfinite(v)].astype(np.float64))
    if not d.size:
        return F(np.inf)
    t = F(d.mean() + float(sigma) * d.std())
    with np.errstate(all="ignore"):
        return np.nextafter(t * t, F(np.inf), dtype=F)
