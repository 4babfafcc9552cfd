"""The clusters of include/gsplat/gs_abi.h "clusters", restated in numpy: the definition the GPU is held to.

Two members are linked when neigh_restate's distance test says so -- the test itself is not written a second time: every question
asked here ("which of these splats lie within the radius of one of those") is a call of neigh_restate.counts with a source and a
query mask and limit 1, i.e. rows of the adjacency matrix, built blockwise by that module's float32 expression.  The components
are then a plain breadth-first search: the smallest member not yet labelled is the seed of the next cluster and therefore its
label; what is reached is taken out of the remaining splats.  Members without any link (found by one call) and members with a
non-finite coordinate are singletons.  No GPU, no grid, no union-find, no scipy."""
import numpy as np

import neigh_restate as nr

F = np.float32
NONE = 2**32 - 1


def _reached(p, radius, frontier, rest):
    """The splats of `rest` (indices) within the radius of one of `frontier` (indices, disjoint from rest)."""
    sub = np.concatenate([frontier, rest])
    src = np.arange(sub.size) < frontier.size
    c = nr.counts(p[sub], radius, src, ~src, limit=1, block=max(16, 2**20 // max(1, frontier.size)))
    return rest[c[frontier.size:] == 1]


def components(pos, radius, members=None):
    """(label, size), uint32[N] each.  pos: [N, 3] (or records [N, 80]: the first three floats); members: a boolean mask, None =
    every splat.  A member gets the smallest index of its cluster and the cluster's number of members, a member with a NaN or
    infinite coordinate itself and 1, a non-member NONE and 0."""
    p = np.ascontiguousarray(np.asarray(pos, dtype=F)[:, :3])
    n = p.shape[0]
    mem = np.ones(n, bool) if members is None else np.asarray(members, bool)
    label, size = np.full(n, NONE, np.uint32), np.zeros(n, np.uint32)
    idx = np.arange(n, dtype=np.uint32)
    label[mem], size[mem] = idx[mem], 1  # singletons, until linked
    fin = mem & np.isfinite(p).all(axis=1)
    rest = np.flatnonzero(fin & (nr.counts(p, radius, fin, fin, limit=1) == 1))  # the members with a link, ascending
    while rest.size:
        seed, rest = rest[:1], rest[1:]
        comp, frontier = [seed], seed
        while frontier.size and rest.size:
            frontier = _reached(p, radius, frontier, rest)
            rest = np.setdiff1d(rest, frontier, assume_unique=True)
            comp.append(frontier)
        comp = np.concatenate(comp)
        label[comp], size[comp] = seed[0], comp.size
    return label, size


def member(size, lo, hi, inside=True):
    """gs_state_cluster's membership: (size >= lo && size <= hi) == inside, on the plane value (a non-member's 0 takes part)."""
    return nr.member(size, lo, hi, inside)


def linked(labels, seeds):
    """gs_state_cluster_linked's membership: the splats with a label whose cluster holds a splat of the boolean mask `seeds`."""
    labels = np.asarray(labels, np.uint32)
    has = labels != NONE
    return has & np.isin(labels, labels[np.asarray(seeds, bool) & has])
