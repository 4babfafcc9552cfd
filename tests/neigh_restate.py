"""The neighbour count of include/gsplat/gs_abi.h "neighbourhoods", restated in numpy: the definition the GPU is held to.

A blockwise brute force over all pairs with exactly the header's f32 expression: d = p_j - p_i per component,
d2 = (dx dx + dy dy) + dz dz (every operation rounded once to f32: numpy float32 arithmetic does that), d2 <= r2 inclusive with
r2 = radius * radius as ONE f32 product, self excluded by index, the count saturated at `limit`.  A NaN or infinite coordinate makes
the comparison false (inf - inf and 0 * inf are NaN, inf * inf is inf > r2).  No GPU, no grid."""
import numpy as np

F = np.float32


def counts(pos, radius, src=None, qry=None, limit=2**32 - 1, block=512):
    """uint32[N]: for every i with qry[i], min(limit, #{j != i : src[j] and d2(i, j) <= r2}); 0 where not qry[i].  pos: [N, 3]
    (or records [N, 80]: the first three floats); src / qry: boolean masks, None = every splat."""
    p = np.ascontiguousarray(np.asarray(pos, dtype=F)[:, :3])
    n = p.shape[0]
    src = np.ones(n, bool) if src is None else np.asarray(src, bool)
    qry = np.ones(n, bool) if qry is None else np.asarray(qry, bool)
    r2 = F(radius) * F(radius)
    js = np.flatnonzero(src)
    out = np.zeros(n, np.uint64)
    with np.errstate(all="ignore"):
        for i0 in range(0, n, block):
            i = np.arange(i0, min(n, i0 + block))
            d = p[js][None, :, :] - p[i][:, None, :]  # p_j - p_i
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert d2.dtype == F
            out[i] = ((d2 <= r2) & (js[None, :] != i[:, None])).sum(axis=1)
    out[~qry] = 0
    return np.minimum(out, np.uint64(limit)).astype(np.uint32)


def member(c, lo, hi, inside=True):
    """gs_state_neigh's membership: (c >= lo && c <= hi) == inside."""
    c = np.asarray(c, np.uint32).astype(np.uint64)
    return ((c >= int(lo)) & (c <= int(hi))) == bool(inside)
