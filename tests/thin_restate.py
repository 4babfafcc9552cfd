"""Thinning restated (include/gsplat/gs_abi.h "thinning"): a numpy brute force over all pairs with the header's f32 expression, the
rank as Python integers and the sequential greedy -- and, separately written, an iteration of the header's two fixpoint rules.  No
grid, no rounds of a device, nothing of the library."""
import numpy as np

F = np.float32
NONE = 2**32 - 1
ORDER_INDEX, ASCENDING = 1, 2
M32 = 0xFFFFFFFF


def hash32(i, seed=0):
    """The header's hash of the index, mod 2^32."""
    h = (int(i) + int(seed) * 0x9E3779B9) & M32
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    h ^= h >> 16
    return h


def hash32_array(idx, seed=0):
    h = (np.asarray(idx, np.uint64) + np.uint64((int(seed) * 0x9E3779B9) & M32)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & np.uint64(M32)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def pkey(value, ascending=False):
    """P of one f32 priority value: the order-preserving key, complemented when ascending; 0 for a NaN in both directions."""
    b = int(np.asarray(value, F).reshape(1).view(np.uint32)[0])
    if (b & 0x7FFFFFFF) > 0x7F800000:
        return 0
    k = b ^ (M32 if b >> 31 else 0x80000000)
    return (~k & M32) if ascending else k


def ranks(n, priority=None, flags=0, seed=0):
    """R_i as Python integers."""
    out = []
    for i in range(n):
        p = 0 if priority is None else pkey(priority[i], bool(flags & ASCENDING))
        h = (~i & M32) if flags & ORDER_INDEX else hash32(i, seed)
        out.append((p << 32) | h)
    return out


def links(pos, radius):
    """bool[n, n]: d2(i, j) <= r2 in f32, one rounding per operation, the diagonal cleared; a non-finite splat links to nobody."""
    p = np.asarray(pos, F)
    r2 = F(radius) * F(radius)
    with np.errstate(all="ignore"):
        d = p[None, :, :] - p[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        adj = d2 <= r2
    fin = np.isfinite(p).all(axis=1)
    adj &= fin[:, None] & fin[None, :]
    np.fill_diagonal(adj, False)
    return adj


def _members(n, members):
    return np.ones(n, bool) if members is None else np.asarray(members, bool)


def sample(pos, radius, members=None, priority=None, flags=0, seed=0, adj=None):
    """(keeper, covers) uint32[n]: the members visited from the highest rank down; kept iff no member kept before is linked."""
    p = np.asarray(pos, F)
    n = p.shape[0]
    mem = _members(n, members)
    adj = links(p, radius) if adj is None else adj  # (adj: links(pos, radius), computed once by a caller with many orders)
    R = ranks(n, priority, flags, seed)
    order = sorted(np.flatnonzero(mem).tolist(), key=lambda i: (-R[i], i))
    kept = np.zeros(n, bool)
    keeper, covers = np.full(n, NONE, np.uint32), np.zeros(n, np.uint32)
    for i in order:
        near = np.flatnonzero(adj[i] & kept)
        if near.size == 0:
            kept[i] = True
            keeper[i] = i
        else:
            keeper[i] = min(near.tolist(), key=lambda j: (-R[j], j))  # the one that outranks all the others
    for i in order:
        covers[keeper[i]] += 1
    return keeper, covers


def fixpoint(pos, radius, members=None, priority=None, flags=0, seed=0, adj=None):
    """bool[n] kept, by iterating the two rules: kept iff every linked member that outranks it is dropped; dropped iff some linked
    member that outranks it is kept."""
    p = np.asarray(pos, F)
    n = p.shape[0]
    mem = _members(n, members)
    adj = (links(p, radius) if adj is None else adj) & mem[:, None] & mem[None, :]
    R = ranks(n, priority, flags, seed)
    pos_of = np.empty(n, np.int64)
    pos_of[sorted(range(n), key=lambda i: (-R[i], i))] = np.arange(n)
    above = adj & (pos_of[None, :] < pos_of[:, None])  # above[i, j]: j is linked to i and outranks it
    kept, dropped = np.zeros(n, bool), np.zeros(n, bool)
    while True:
        new_dropped = mem & (above & kept[None, :]).any(axis=1)
        new_kept = mem & ~(above & ~new_dropped[None, :]).any(axis=1) & ~new_dropped
        if np.array_equal(new_kept, kept) and np.array_equal(new_dropped, dropped):
            break
        kept, dropped = new_kept, new_dropped
    assert np.array_equal(kept | dropped, mem)
    return kept


def info_counts(keeper, covers):
    """(members, kept, dropped, largest) of two planes."""
    members = int((keeper != NONE).sum())
    kept = int((keeper == np.arange(keeper.size)).sum())
    return members, kept, members - kept, int(covers.max()) if covers.size else 0


def member(covers, lo, hi, inside=True):
    """gs_state_thin's membership: the plain expression on the plane value."""
    c = np.asarray(covers, np.uint64)
    return ((c >= lo) & (c <= hi)) == bool(inside)
