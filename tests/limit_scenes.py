"""Scenes whose (gaussian, tile) instance count is known to the unit, at and beyond the limits of 32-bit binning arithmetic, for
tests/test_instance_limits.py; and a model, in exact integers, of the sums the binning kernels form over them.

Scenes are built in pixel space (row_scenes.records) on two canvases of 8-pixel tiles from two kinds of splat:

  BLANKETS  centred on the canvas, sigma 1e5 px (35 canvas diagonals), opacity 0.5.  alpha >= 1/255 on every pixel (blanket_alpha_floor
            proves it from the conic at the four canvas corners), so no binning may drop an instance that lies on the canvas.
  FILLERS   floor-size splats on the centre of one tile, alpha >= 1/255 at the centre pixel: exactly one instance each.

What a blanket counts is NOT the number of tiles of the canvas.  The reference clamps the 3-sigma rect to [0, ntx] x [0, nty] and
counts (ntx + 1)(nty + 1) instances (process_gaussians.wgsl:74-86): the aliased column ntx and the tile row nty below the canvas are
in its count and in its (key, value) list, and only the ranges ignore them.  The tight row pipeline hands out what
lies on the canvas: ntx * nty tiles and the aliased column's tile (row + 1, column 0) of all rows but the last.

              tiles     reference count of a blanket        tight count of a blanket
  2040x2040   65 025    256 * 256 = 65 536 = 2^16           65 025 + 254 = 65 279
  2048x2040   65 280    257 * 256 = 65 792                  (the row pipeline does not take 256 columns: the reference's count)

Both are asserted from the oracle's projection and from gs_tight.h compiled for the host (tools/tight_check), never assumed.
"""
import collections

import numpy as np

from row_scenes import FLOOR, params, records, tight_check
from support import HUGE, cached

TS = 8
ROWS = (2040, 2040)   # 255 x 255 tiles: the largest canvas the row pipeline takes
WIDE = (2048, 2040)   # 256 x 255 tiles: product frames fall back to the reference's binning
LIMIT = 1 << 30       # gs_frame.hip wait_one: need >= 2^30 is refused
MARK = (1 << 32) - 1  # what a saturated 32-bit sum reads
BLANKET_LOGIT = 0.0   # opacity 0.5
FILLER_LOGIT = 1.0    # opacity 0.73
SMALL = 2.0e-5        # scale_modifier of the recovery frame: a blanket becomes 2 px of sigma

Case = collections.namedtuple("Case", "name canvas blankets fillers depth index")


def kinds(case):
    """Per gaussian index: 0 a blanket, 1 a filler."""
    B, F = case.blankets, case.fillers
    if case.index == "first":
        return np.concatenate([np.zeros(B, np.int64), np.ones(F, np.int64)])
    if case.index == "last":
        return np.concatenate([np.ones(F, np.int64), np.zeros(B, np.int64)])
    n = min(B, F)  # "mixed": b0 f0 b1 f1 ..., the longer one's tail follows
    return np.concatenate([np.tile([0, 1], n), np.zeros(B - n, np.int64), np.ones(F - n, np.int64)])


def buckets(case, kind):
    """The depth bucket every gaussian is to land in (u32(min(50 depth, 999)), write_tile_ids.wgsl:31)."""
    rank = np.where(kind == 0, np.cumsum(kind == 0) - 1, np.cumsum(kind == 1) - 1)
    if case.depth == "one":
        return np.full(kind.size, 100)
    if case.depth == "two":      # the fillers in front
        return np.where(kind == 0, 100, 50)
    if case.depth == "halves":   # the fillers in front, the blankets of the first half of the indices before those of the second
        return np.where(kind == 0, np.where(rank < case.blankets // 2, 100, 150), 50)
    assert case.depth == "many"
    return np.where(kind == 0, 10 + rank % 200, 500 + rank % 300)


def build(case):
    """(splats, uniforms, kind, wanted bucket) of a case, once."""
    def make():
        W, H = case.canvas
        ntx, nty = W // TS, H // TS
        kind = kinds(case)
        P = np.empty((kind.size, 6))
        P[kind == 0] = (W / 2.0, H / 2.0, HUGE, HUGE, 0.0, BLANKET_LOGIT)
        t = np.arange(case.fillers) % (ntx * nty)
        if case.fillers:
            P[kind == 1] = params(TS * (t % ntx) + TS / 2.0, TS * (t // ntx) + TS / 2.0, FLOOR, FLOOR, 0.0, FILLER_LOGIT)
        b = buckets(case, kind)
        s, u = records(P, W, H, (b + 0.5) / 50.0, seed=len(case.name))
        return s, u, kind, b
    return cached(("limit_scene", case.name), make)


def small_uniforms(u):
    """The same camera with scale_modifier SMALL: every blanket shrinks to a few tiles, every filler stays on its tile."""
    v = np.array(u, np.float32, copy=True)
    v[39] = SMALL
    return v


def projection(oracle, case):
    """What the oracle's projection gives the binning: dict(counts, bucket, gdata), counts as int64."""
    def make():
        s, u, _, _ = build(case)
        W, H = case.canvas
        gd, cnt = oracle.preprocess(s, u, W, H, TS)
        depth = gd[:, 7].view(np.float32)
        with np.errstate(all="ignore"):
            bucket = np.minimum(np.float32(50.0) * depth, np.float32(999.0)).astype(np.uint32).astype(np.int64)  # the kernels' own f32 expression
        return {"counts": cnt.astype(np.int64), "bucket": bucket, "gdata": gd}
    return cached(("limit_projection", case.name), make)


def blanket_alpha_floor(gdata, W, H):
    """The smallest alpha, in float64, of the records `gdata` over the four corner pixels of the canvas.  The conic is positive
    definite and the centre lies on the canvas, so q = 0.5 (cx dx^2 + cz dy^2) + cy dx dy is convex and takes its maximum over the
    canvas at a corner: every pixel's alpha is at least this."""
    g = gdata.view(np.float32).reshape(-1, 16).astype(np.float64)
    gx, gy, cx, cy, cz, op = g[:, 0] * W, g[:, 1] * H, g[:, 4], g[:, 5], g[:, 6], g[:, 11]
    assert (cx > 0).all() and (cx * cz - cy * cy > 0).all() and (gx >= 0).all() and (gx <= W - 1).all() and (gy >= 0).all() and (gy <= H - 1).all()
    worst = np.full(g.shape[0], np.inf)
    for px in (0.0, W - 1.0):
        for py in (0.0, H - 1.0):
            dx, dy = gx - px, gy - py
            worst = np.minimum(worst, op * np.exp(-(0.5 * (cx * dx * dx + cz * dy * dy) + cy * dx * dy)))
    return float(worst.min())


def _tight_dump(case, u=None):
    """The slots of the case's representatives under uniforms u: (rep: their gaussian indices, slots as tools/tight_check dumps them
    with column 0 numbering `rep`).  The slots of a gaussian depend on nothing but its own record, so one blanket per distinct depth
    stands for all blankets of that depth; every filler is dumped."""
    def make():
        s, uu, kind, b = build(case)
        W, H = case.canvas
        isb = kind == 0
        bb = np.unique(b[isb])
        rep_b = np.array([np.flatnonzero(isb & (b == x))[0] for x in bb], np.int64)
        rep = np.sort(np.concatenate([rep_b, np.flatnonzero(~isb)]))
        sl, _ = tight_check.dump(s[rep], uu if u is None else u, W, H, TS)
        return rep, rep_b, bb, sl.astype(np.int64)
    return cached(("limit_tight_dump", case.name, None if u is None else u.tobytes()), make)


def tight_shapes(case, u=None):
    """(slots, items, instances) per gaussian of what the tight projection hands the row pipeline under uniforms u (None: the case's
    own), from gs_tight.h on the host."""
    rep, rep_b, bb, sl = _tight_dump(case, u)
    _, _, kind, b = build(case)
    g, tiles = sl[:, 0], sl[:, 4]
    n = rep.size
    per = np.stack([np.bincount(g, minlength=n), np.bincount(g[tiles > 0], minlength=n), np.bincount(g, weights=tiles, minlength=n).astype(np.int64)], axis=1)
    out = np.zeros((kind.size, 3), np.int64)
    out[rep] = per
    for x, i in zip(bb, rep_b):
        out[(kind == 0) & (b == x)] = per[np.searchsorted(rep, i)]
    return out


def tight_tile_counts(case):
    """Instances per tile of the case's frame in the row pipeline, exact (int64 [tiles])."""
    rep, rep_b, bb, sl = _tight_dump(case)
    _, _, kind, b = build(case)
    W, H = case.canvas
    ntx, T = W // TS, (W // TS) * (H // TS)
    mult = np.ones(rep.size, np.int64)  # how many gaussians a representative stands for
    for x, i in zip(bb, rep_b):
        mult[np.searchsorted(rep, i)] = int(((kind == 0) & (b == x)).sum())
    diff = np.zeros(T + 1, np.int64)    # an item is a run of consecutive tiles of one tile row
    it = sl[sl[:, 4] > 0]
    first = it[:, 2] * ntx + it[:, 3]
    np.add.at(diff, first, mult[it[:, 0]])
    np.add.at(diff, first + it[:, 4], -mult[it[:, 0]])
    return np.cumsum(diff)[:T]


# ---- the sums of the reference's scan (k_binning.hip) ---------------------------------------------------------------------------------
def fold(v, saturate):
    """What a 32-bit word keeps of the exact sum v: min(v, 2^32 - 1) as the kernels do it, or v mod 2^32 as a wrapping add would."""
    v = np.asarray(v, np.int64)
    return np.minimum(v, MARK) if saturate else v & MARK


def scan_model(counts, saturate=True):
    """(offsets, I) of the index-order scan: the exclusive prefix and the total, each folded to 32 bits."""
    c = np.asarray(counts, np.int64)
    incl = np.cumsum(c)
    return fold(incl - c, saturate), int(fold(incl[-1] if c.size else 0, saturate))


# ---- the sums of the gaussian-level sort, restated from the header of k_gsort.hip ------------------------------------------------------
GC = 2048          # "a chunk of 2048 consecutive gaussian INDICES"
GBINS = 1024       # buckets
DEFAULT_GRID = 1024  # GS_OPT_PERSISTENT_GRID at its default: 4 workgroups on each of the chip's 256 compute units
SITES = ("row", "base", "carried", "total")


def gsort_model(bucket, qty, grid=DEFAULT_GRID, saturate=True):
    """The (bucket, run) arithmetic of the sort over per-index (bucket, quantity; 0: not visible), every stored word folded to 32 bits.

    "The NT chunks are cut into G contiguous RUNS of ceil(NT / G) chunks"; hist: M[bucket][run] = the run's quantity of the bucket;
    rowscan: "every bucket's row of M is scanned over the runs (exclusive) -> row totals"; scatter: "every run builds its bucket
    bases once (scan of the row totals + its column of M), then walks its chunks in ascending order ... one record per gaussian at
    base[bucket] + rank; then base[bucket] advances by the chunk's own (count, quantity) of the bucket"; "Quantities are summed in 64
    bits and stored as sat32(sum)".  Returns dict: total (the reported quantity), off (per index: the quantity prefix its record
    carries; -1 invisible), runs, cpr, and `site`: which partial sum is the FIRST, in the order the kernels form them, whose exact
    value reaches 2^32 -- "row" (a populated bucket's prefix over the runs or its row total), "base" (a run's starting base of a
    bucket it holds: the scan over buckets plus the run's column), "carried" (a base after it advanced past a chunk, at a later chunk
    that holds the bucket), "record" (no base, but a record's own prefix: the base plus the in-chunk prefix of its bucket), "total"
    (nothing any record uses; the frame's total alone), or None."""
    bucket, qty = np.asarray(bucket, np.int64), np.asarray(qty, np.int64)
    n = qty.size
    NT = -(-n // GC)
    cpr = -(-NT // max(int(grid), 1))
    G = -(-NT // cpr)
    vis = qty > 0
    idx = np.arange(n)
    chunk, run = idx // GC, idx // GC // cpr
    M = np.zeros((GBINS, G), np.int64)  # exact
    np.add.at(M, (bucket[vis], run[vis]), qty[vis])
    Ms = fold(M, saturate)
    ex_row = np.cumsum(Ms, axis=1) - Ms              # 64-bit sums of the stored words
    rowtot_exact = Ms.sum(axis=1)
    row_store, rowtot = fold(ex_row, saturate), fold(rowtot_exact, saturate)
    ex_b = np.cumsum(rowtot) - rowtot                # the scan over buckets, 64 bits wide in the kernel
    base0_exact = ex_b[:, None] + row_store
    total_exact = int(rowtot.sum())
    populated = M > 0
    site = None
    if (np.cumsum(M, axis=1)[populated.any(axis=1)] > MARK).any():
        site = "row"
    elif (base0_exact[populated] > MARK).any():
        site = "base"
    base = fold(base0_exact, saturate)               # [bucket][run]: what LDS holds when the run starts
    off = np.full(n, -1, np.int64)
    carried_hit = record_hit = False
    for r in range(G):
        b_run, e_run = base[:, r].copy(), base0_exact[:, r].copy()  # what LDS holds, and the exact sum it stands for
        for c in range(r * cpr, min((r + 1) * cpr, NT)):
            sel = np.flatnonzero(vis & (chunk == c))
            if sel.size == 0:
                continue
            o = sel[np.argsort(bucket[sel], kind="stable")]  # (bucket, index) order inside the chunk
            q, bb = qty[o], bucket[o]
            assert int(q.sum()) <= MARK  # the in-chunk prefix P is exact (its saturation is out of this module's scope)
            P = np.cumsum(q) - q
            start = np.searchsorted(bb, bb, "left")
            exact = b_run[bb] + (P - P[start])
            if c > r * cpr and (e_run[np.unique(bb)] > MARK).any():
                carried_hit = True
            record_hit = record_hit or bool(((e_run[bb] + (P - P[start])) > MARK).any())
            off[o] = fold(exact, saturate)
            cq = np.bincount(bb, weights=q, minlength=GBINS).astype(np.int64)
            b_run, e_run = fold(b_run + cq, saturate), e_run + cq
    if site is None and carried_hit:
        site = "carried"
    if site is None and record_hit:
        site = "record"
    if site is None and total_exact > MARK:
        site = "total"
    return {"total": int(fold(total_exact, saturate)), "off": off, "runs": G, "cpr": cpr, "site": site}


# ---- what a truncated debug frame must still hold ------------------------------------------------------------------------------------
def emission_prefix(oracle, case, capacity):
    """The first `capacity` (key, value) pairs of the reference's emission (gaussians in index order): those a frame that does not
    fit still writes."""
    p = projection(oracle, case)
    cnt = p["counts"]
    m = int(np.searchsorted(np.cumsum(cnt), capacity, "left")) + 1
    m = min(m, cnt.size)
    c32 = cnt[:m].astype(np.uint32)
    off, tot = oracle.scan(c32)
    k, v = oracle.emit(p["gdata"][:m], off, c32, tot, case.canvas[0], TS, H=case.canvas[1])
    return k[:capacity], v[:capacity]


def model_slots(case):
    """(S, R, I) of the case's frame in the row pipeline."""
    t = tight_shapes(case)
    return tuple(int(x) for x in t.sum(axis=0))

