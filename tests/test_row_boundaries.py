"""The tight row pipeline (k_rows.hip: row sort, count, scan, expansion; fed by k_preprocess.hip and k_gsort.hip) at its hand-written
boundaries: sort tiles of 4096 slots and their 512-slot wave shares, the 1024-slot granule of the gaussian sort's chunk table, the
look-back's rounds of 8, 7- and 8-bit digits, chunks of 512 items, the scan's 4 parts and 8 loads, the expansion's sub-batches of
2048 instances and wave shares of 512, and the chunk a workgroup prefetches for its next trip.

Scenes are built in pixel space from four kinds of splat whose row items are known: DOTS (one slot, one item, one instance), BARS
(one item of L tiles), POSTS (one-tile items in consecutive tile rows) and BLANKETS (an item of ntx tiles in every row, plus the
aliased column's items).  How many of each go where sets the slots, items and instances of a sort tile, a tile row or a chunk exactly.
What a scene gives the row pipeline is computed on the CPU: tools/tight_check (gs_tight.h compiled for the host) dumps every slot,
rows_restate.model orders and cuts them the way the kernels do.

The unmarked tests assert, from that model alone, that every scene reaches the boundary its name says.  The gpu tests render every
scene on the product path with GS_FLAG_EXACT_BLEND, on the default grid and with GS_OPT_PERSISTENT_GRID 4 (3 sort, 8 count and 6
expansion workgroups, so that every workgroup takes many tiles or chunks), and assert the frame's slot, item and instance counts
with equality, the lists through gpu_checks.check_product_lists and the image bit for bit.  Nothing here has a tolerance.
"""
import numpy as np
import pytest

import rows_restate as rr
from row_scenes import (BAR_LOGIT, BLANKET_LOGIT, DEFAULT, FLOOR, LONG_CANVAS, POST_CANVAS, _rng, bar_table, bars, blankets, dots, frame_of, frames,
                        interleave, model_of, params, per_splat, post, records, scene, slots_of, tight_check)
from support import cached


# row sort, slot totals: S dots over all rows, in REVERSED depth (z falls as the index rises: the slot order is not the record order)
SLOT_TOTALS = (1, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 9 * 4096, 9 * 4096 + 1, 17 * 4096 + 1)


def slot_total_scene(S):
    def make():
        W, H, ts = DEFAULT
        rng = _rng(1, S)
        tile = rng.integers(0, 108, S)
        tile[:min(S, 9)] = 12 * np.arange(9)[:min(S, 9)] + 5  # every row is populated
        z = 1.0 + 18.0 * (S - 1 - np.arange(S)) / max(S - 1, 1)
        return scene("slots_%d" % S, W, H, ts, dots(ts, tile % 12, tile // 12, rng), z=z, S=S)
    return cached(("slot_total_scene", S), make)


# row sort, one gaussian across a boundary: a post of K slots on 16 x 320 (2 x 40 tiles of 8 pixels) after X dots, in the first of two
# interleaved depth buckets
K = 40
KI = 20  # of a post's K slots the first KI are its items (one per tile row), the other KI the aliased column's holes
STRADDLES = {"tile_minus_1": 4096 - 1, "tile": 4096, "ends_tile": 4096 - K, "last_slot_over_tile": 4096 - K + 1, "half_over_tile": 4096 - K // 2, "half_over_wave": 512 - K // 2,
             "granule_minus_1": 1024 - 1, "granule": 1024, "half_over_granule_3": 3 * 1024 - K // 2,
             # ... and with half of the post's ITEMS on either side of the boundary (at boundary - K / 2 only its holes lie beyond it)
             "items_over_tile": 4096 - KI // 2, "items_over_wave": 512 - KI // 2, "items_over_granule_3": 3 * 1024 - KI // 2}


def _two_buckets(A, B):
    P, which = interleave(A, B)
    return P, np.where(which == 0, 1.0, 1.5)  # buckets 50 and 75


def straddle_scene(name):
    def make():
        W, H, ts = POST_CANVAS
        rng = _rng(2, len(name), STRADDLES.get(name, 0))
        rt = lambda k: dots(ts, rng.integers(0, 2, k), rng.integers(0, 40, k), rng)
        pk, shape = post(W, H, ts, lambda r: r[0] == K and r[1] >= 10)
        if name == "posts_only":
            P, z = _two_buckets(np.repeat(pk, 110, axis=0), rt(50))
            return scene("straddle_" + name, W, H, ts, P, z=z, first=None, post=shape)
        if name == "long_post":
            W, H, ts = LONG_CANVAS
            rt = lambda k: dots(ts, rng.integers(0, 2, k), rng.integers(0, 255, k), rng)
            pl, shape = post(W, H, ts, lambda r: r[0] >= 200 and r[1] >= 50)
            P, z = _two_buckets(np.concatenate([rt(4000), pl, rt(150)]), rt(100))
            return scene("straddle_" + name, W, H, ts, P, z=z, first=4000, post=shape)
        X = STRADDLES[name]
        P, z = _two_buckets(np.concatenate([rt(X), pk, rt(300)]), rt(200))
        return scene("straddle_" + name, W, H, ts, P, z=z, first=X, post=shape)
    return cached(("straddle_scene", name), make)


# row sort, holes: thin diagonal splats hanging over the left edge of a 512 x 512 canvas of 8-pixel tiles (their rows whose chord
# lies left of the canvas are holes), and diagonal splats across a tile-column slab (runs outside the slab are holes)
HOLE_CANVAS = (512, 512, 8)
SLAB = (8, 24)


def hole_scene(name):
    def make():
        rng = _rng(3, len(name))
        if name in ("tail", "long_tail"):  # the frame's last, short sort tile holds nothing but the aliased holes of the last gaussian
            W, H, ts = POST_CANVAS if name == "tail" else LONG_CANVAS
            rt = lambda k: dots(ts, rng.integers(0, 2, k), rng.integers(0, H // ts, k), rng)
            pk, shape = post(W, H, ts, (lambda r: r[0] == K and r[1] == KI) if name == "tail" else (lambda r: r[0] == 510 and r[1] == 255))
            nd = 4096 - int(shape[1])  # dots before the post: its items end the first tile
            P, z = _two_buckets(rt(nd - 700), np.concatenate([rt(700), pk]))  # the post is the last record of the last bucket
            return scene("holes_" + name, W, H, ts, P, z=z, post=shape)
        W, H, ts = HOLE_CANVAS
        if name == "left_edge":
            k = 130
            gh = params(-24.0, ts * rng.integers(25, 39, k) + 4.3, 60.0, FLOOR, np.deg2rad(80.0), BAR_LOGIT)
            P = np.concatenate([gh, dots(ts, rng.integers(0, 64, 100), rng.integers(0, 64, 100), rng)])
            return scene("holes_" + name, W, H, ts, P)
        k = 300
        dg = params(rng.uniform(30.0, 230.0, k), rng.uniform(60.0, 450.0, k), 40.0, FLOOR, np.deg2rad(rng.choice([45.0, 135.0, 60.0], k)), BAR_LOGIT)
        P = np.concatenate([dg, dots(ts, rng.integers(SLAB[0], SLAB[1], 600), rng.integers(0, 64, 600), rng)])
        return scene("holes_" + name, W, H, ts, P[rng.permutation(P.shape[0])], cols=SLAB)
    return cached(("hole_scene", name), make)


# digits: 127 / 128 tile rows and columns
DIGIT_CANVASES = ((16, 1016), (16, 1024), (1016, 16), (1024, 16))


def digit_scene(W, H):
    def make():
        ts = 8
        ntx, nty = W // ts, H // ts
        rng = _rng(4, W, H)
        edge = lambda n: np.array([0, 1, n - 2, n - 1])
        if nty > ntx:
            P = [dots(ts, np.repeat([0, 1], 4), np.tile(edge(nty), 2), rng), dots(ts, rng.integers(0, 2, 700), rng.integers(0, nty, 700), rng)]
            P.append(params(ts * 1.5, H / 2.0 + 4.3, FLOOR, 3.0 * H, 0.0, BAR_LOGIT))  # a post over every row
        else:
            P = [dots(ts, np.tile(edge(ntx), 2), np.repeat([0, 1], 4), rng), dots(ts, rng.integers(0, ntx, 700), rng.integers(0, 2, 700), rng)]
            P.append(params(W - 30.3 - 8.0 * np.arange(6), ts * (np.arange(6) % 2) + 4.0, 25.0, FLOOR, 0.0, BAR_LOGIT))  # bars cut by the right edge
        P = np.concatenate(P)
        return scene("digits_%dx%d" % (W, H), W, H, ts, P[rng.permutation(P.shape[0])])
    return cached(("digit_scene", W, H), make)


# items per tile row: k items (six dots, then a bar, ...) in the row under test, in two interleaved depth buckets
K_ITEMS = (1, 511, 512, 513, 1024, 1025, 2048, 2049, 32 * 512, 32 * 512 + 1)
K_CHUNKS = (1, 1, 1, 2, 2, 3, 4, 5, 32, 33)
PATTERNS = ("row0", "last_row", "rows_2_6", "all_rows")


def _row_items(W, H, ts, row, k, rng, every=7):
    """k items of tile row `row` in record order: every `every`-th a bar of 2 .. 6 tiles, the others dots."""
    ntx = W // ts
    isbar = (np.arange(k) % every) == every - 1
    P = dots(ts, rng.integers(0, ntx, k), np.full(k, row), rng)
    if isbar.any():
        P[isbar] = bars(W, H, ts, row, rng.integers(2, 7, int(isbar.sum())), rng)
    return P


def _blanket_rows(W, H, ts):
    return cached(("blanket_rows", W, H, ts), lambda: rr.model(*slots_of(blankets(W, H, 1), W, H, ts))["row_items"])


def items_scene(k, pattern, ts=16):
    def make():
        W, H = 12 * ts, 9 * ts
        rng = _rng(5, k, PATTERNS.index(pattern), ts)
        target = np.zeros(9, np.int64)
        if pattern == "row0":
            target[0] = k
        elif pattern == "last_row":
            target[8] = k
        elif pattern == "rows_2_6":
            target[2] = target[6] = k
        else:
            target[:] = 300 + 37 * np.arange(9)
            target[4] = k
        parts = []
        if pattern == "all_rows":  # two blankets: an item of 12 tiles in every row and the aliased column's item in rows 1 .. 8
            parts.append(blankets(W, H, 2))
            fill = target - 2 * _blanket_rows(W, H, ts)[:9]
            if (fill < 0).any():  # (k = 1: the row under test holds one blanket's items only -- see the test's docstring)
                parts[0] = parts[0][:0]
                fill = target
        else:
            fill = target
        parts += [_row_items(W, H, ts, r, int(fill[r]), rng) for r in range(9) if fill[r] > 0]
        P = np.concatenate(parts)
        P = P[rng.permutation(P.shape[0])]
        z = np.where(np.arange(P.shape[0]) % 2 == 0, 1.0, 1.5)
        return scene("items_%d_%s_t%d" % (k, pattern, ts), W, H, ts, P, z=z, rows=target)
    return cached(("items_scene", k, pattern, ts), make)


# instances per chunk: a 204 x 3 tile canvas; tile row 1 holds the chunk under test, rows 0 and 2 a few dots
LB = 16  # the bars' length where the case does not set it
INSTANCES = (512, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048, 512 * LB)
PLACEMENTS = {"at_2047": 2047, "at_2048": 2048, "ends_batch": 2048 - LB, "last_over_batch": 2048 - LB + 1, "half_over_batch": 2048 - LB // 2,
              "half_over_wave_1": 512 * 2 - LB // 2, "half_over_wave_2": 2048 + 512 * 3 - LB // 2}
SHORT_CHUNKS = (1, 255, 256, 257)


def _lengths(items, instances):
    """`items` lengths (1: a dot) that add up to `instances`: bars of LB tiles, one shorter bar for the rest, dots."""
    extra = instances - items
    nb, e = divmod(extra, LB - 1)
    seq = [LB] * nb + ([e + 1] if e else [])
    assert 0 <= extra and len(seq) <= items
    return np.array(seq + [1] * (items - len(seq)), np.int64)


def _chunk_rows(W, H, ts, lengths, rng):
    ntx = W // ts
    lengths = np.asarray(lengths)
    P = dots(ts, rng.integers(0, ntx, lengths.size), np.full(lengths.size, 1), rng)
    P[lengths > 1] = bars(W, H, ts, 1, lengths[lengths > 1], rng)
    return P


def chunk_scene(kind, value, ts=8):
    def make():
        W, H = 204 * ts, 3 * ts
        rng = _rng(6, len(kind), value if isinstance(value, int) else len(value), ts)
        want = {}
        if kind == "instances":
            L = rng.permutation(_lengths(512, value))
            want = dict(chunk_inst=[value])
        elif kind == "placement":
            off = PLACEMENTS[value]
            nb, d = divmod(off, LB)  # `off` instances before the bar: nb bars and d dots, shuffled
            L = np.concatenate([rng.permutation([LB] * nb + [1] * d), [LB], np.ones(512 - nb - d - 1, np.int64)]).astype(np.int64)
            want = dict(bar_item=nb + d, bar_offset=off)
        else:
            L = np.concatenate([rng.permutation(_lengths(512, 2500)), rng.permutation(_lengths(value, value + 3 * (LB - 1) * (value > 3)))])
        P = np.concatenate([dots(ts, rng.integers(0, 204, 5), np.zeros(5), rng), _chunk_rows(W, H, ts, L, rng),
                            dots(ts, rng.integers(0, 204, 3), np.full(3, 2), rng)])
        return scene("chunk_%s_%s_t%d" % (kind, value, ts), W, H, ts, P, lengths=L, **want)
    return cached(("chunk_scene", kind, value, ts), make)


def trips_scene():
    def make():
        W, H, ts = DEFAULT
        rng = _rng(7)
        target = 2048 + 17 + 31 * np.arange(9)
        fill = target - 2 * _blanket_rows(W, H, ts)[:9]
        P = np.concatenate([blankets(W, H, 2)] + [_row_items(W, H, ts, r, int(fill[r]), rng, every=5) for r in range(9)])
        return scene("many_trips", W, H, ts, P[rng.permutation(P.shape[0])], rows=target)
    return cached("trips_scene", make)


TILE_SIZE_CASES = [("items", k, ts) for ts in (8, 32) for k in (512, 513, 2049)] + [("instances", v, ts) for ts in (8, 16, 32) for v in (2048, 2049)]


def tile_size_scene(kind, v, ts):
    return items_scene(v, "rows_2_6", ts) if kind == "items" else chunk_scene("instances", v, ts)


# ---- CPU: every scene reaches what its name says ------------------------------------------------------------------------------------
def test_the_dump_agrees_with_the_check_mode():
    """On a bicycle_like frame the slots the dump writes hold exactly the instances the committed check mode counts (its "tight
    total"), per gaussian in slot order, every item inside the canvas and the model's parts add up."""
    s, u = tight_check.bicycle_case(4000, 200, 120, 8, 3)
    slots, bucket = tight_check.dump(s, u, 200, 120, 8)
    res = tight_check.check(s, u, 200, 120, 8)
    assert int(slots[:, 4].sum()) == res["tight_total"] > 0
    g, sl = slots[:, 0].astype(np.int64), slots[:, 1].astype(np.int64)
    new = np.concatenate([[True], g[1:] != g[:-1]])
    assert (np.diff(g) >= 0).all() and (sl[new] == 0).all() and (sl[~new] == sl[np.flatnonzero(~new) - 1] + 1).all()
    it = slots[slots[:, 4] > 0].astype(np.int64)
    assert (it[:, 2] < 15).all() and (it[:, 3] + it[:, 4] <= 25).all() and (slots[:, 4] == 0).any()
    m = rr.model(slots, bucket)
    assert m["S"] == slots.shape[0] and m["R"] == it.shape[0] and m["I"] == res["tight_total"]
    assert m["tile_valid"].sum() == m["R"] == m["row_items"].sum() and m["chunk_inst"].sum() == m["I"]
    assert (m["chunk_end"] - m["chunk_begin"]).sum() == m["R"] and (m["item_offset"] < np.maximum(m["chunk_inst"][m["item_chunk"]], 1)).all()
    key = bucket.astype(np.int64)[m["order"]] * (1 << 32) + m["order"]
    assert (np.diff(key) > 0).all() and np.unique(bucket[m["order"]]).size > 10  # (bucket, index) order over many buckets


def test_the_primitives_are_what_the_scenes_assume():
    """At tile 8, 16 and 32 on a 12 x 9 tile canvas: a dot on every tile is one slot, one item, one instance; the bar table's entries
    are one slot and one item of L tiles in whatever row and at whatever shift `bars` puts them; a blanket is an item of 12 tiles in
    every row, an aliased item in rows 1 .. 8 and one hole (the last row's aliased slot)."""
    for ts in (8, 16, 32):
        W, H = 12 * ts, 9 * ts
        rng = _rng(0, ts)
        t = np.arange(108)
        sh = per_splat(dots(ts, t % 12, t // 12, rng), W, H, ts)
        assert (sh[:, :3] == 1).all() and (sh[:, 3] == t % 12).all() and (sh[:, 4] == t // 12).all()
        tab = bar_table(W, H, ts)
        assert set(range(2, 7)) <= set(tab), sorted(tab)
        L = np.array(sorted(tab) * 4)
        for row in (0, 4, 8):
            sh = per_splat(bars(W, H, ts, row, L, rng), W, H, ts)
            assert (sh[:, 0] == 1).all() and (sh[:, 1] == 1).all() and (sh[:, 2] == L).all() and (sh[:, 4] == row).all()
        m = rr.model(*slots_of(blankets(W, H, 1), W, H, ts))
        assert (m["S"], m["R"], m["I"]) == (18, 17, 9 * 12 + 8)
        assert list(m["row_items"][:9]) == [1] + [2] * 8
    tab = bar_table(1632, 24, 8)
    assert set(range(2, LB + 1)) <= set(tab), sorted(tab)


@pytest.mark.parametrize("S", SLOT_TOTALS)
def test_slot_total_scenes(S):
    m = model_of(slot_total_scene(S))
    assert (m["S"], m["R"], m["I"]) == (S, S, S)
    assert m["tile_valid"].sum() == S and m["tile_valid"].size == -(-S // 4096) and (m["tile_valid"][:-1] == 4096).all()
    assert m["tile_valid"][-1] == (S - 1) % 4096 + 1
    assert (m["row_items"][:9] > 0).all() if S >= 9 else m["row_items"].sum() == S
    if S > 1:
        assert (np.diff(m["order"]) < 0).any()  # the slot order is not the record order
    last = m["tile_valid"].size - 1
    assert rr.lookback_rounds(last) == {9 * 4096: 1, 9 * 4096 + 1: 2, 17 * 4096 + 1: 3}.get(S, 1 if last else 0)
    assert rr.grids(4) == (3, 8, 6)


@pytest.mark.parametrize("name", list(STRADDLES) + ["posts_only", "long_post"])
def test_straddle_scenes(name):
    """The post of 40 slots: on a canvas 16 pixels wide every post's rect reaches the aliased column, so a post has twice as many slots
    as tile rows.  Its slots 0 .. 19 are the items of its 20 tile rows, its slots 20 .. 39 the aliased column's slots of those rows, all
    holes (tile (row + 1, 0) is not touched from column 1).  At boundary - k / 2 (half_over_*) the boundary therefore falls between the
    post's last item and its first hole; items_over_* put the first slot at boundary - 10, so that ten of its items lie on either side.
    Its first slot is where the case puts it; the dots of the second depth bucket follow every slot of the first.
    A first slot of 4096 - k + 1 puts the post's LAST slot on 4096, the next tile's first, not on the tile's last: that position is kept
    (last_slot_over_tile) and 4096 - k, whose last slot is the tile's last, added (ends_tile)."""
    sc = straddle_scene(name)
    m = model_of(sc)
    big = np.flatnonzero(m["nslots"] > 1)
    if name == "posts_only":
        assert (m["nslots"][m["first_slot"] < 4096] == K).all() and big.size == 110 and m["S"] == 110 * K + 50
        items = int(sc["want"]["post"][1])
        assert rr.straddlers(m, 4096).size == 1 and (4096 // K) * items <= m["tile_valid"][0] <= (4096 // K) * items + 4096 % K
        return
    assert big.size == 1
    first, n = int(m["first_slot"][big[0]]), int(m["nslots"][big[0]])
    assert first == sc["want"]["first"] and n == sc["want"]["post"][0]
    assert (np.diff(m["order"]) < 0).any()
    if name == "long_post":
        assert n >= 200 and first < 4096 < first + n and rr.straddlers(m, 4096).size == 1
        return
    assert n == K and sc["want"]["post"][1] == KI
    t = m["slot_tiles"][first:first + K]
    assert (t[:KI] == 1).all() and (t[KI:] == 0).all()  # the items first, then the aliased holes
    crossed = {"tile_minus_1": 4096, "tile": None, "ends_tile": None, "last_slot_over_tile": 4096, "half_over_tile": 4096, "half_over_wave": 512, "granule_minus_1": 1024,
               "granule": None, "half_over_granule_3": 3072, "items_over_tile": 4096, "items_over_wave": 512, "items_over_granule_3": 3072}[name]
    for b in (512, 1024, 3072, 4096):
        assert (rr.straddlers(m, b).size == 1) == (b == crossed), (name, b)
    if name == "tile":
        assert first == 4096
    if name == "ends_tile":
        assert first + n == 4096
    if name == "granule":
        assert first == 1024
    if name.startswith("half_over"):
        assert first + n // 2 == crossed and first + KI == crossed
    if name.startswith("items_over"):
        assert int((m["slot_tiles"][first:crossed] > 0).sum()) == KI // 2 == int((m["slot_tiles"][crossed:first + K] > 0).sum())


HOLE_SCENES = ["left_edge", "slab", "tail", "long_tail"]


@pytest.mark.parametrize("name", HOLE_SCENES)
def test_hole_scenes(name):
    """left_edge: the first sort tile holds at least three quarters holes.  slab: a tile-column slab context, whose holes are the rows of
    a diagonal splat that run outside the slab.  tail, long_tail: a sort tile WITHOUT a valid item.  A FULL tile cannot be one (a
    gaussian whose slots are all holes takes no slots at all, a gaussian has at most 2 x 255 slots, so 4096 consecutive slots hold
    whole gaussians and with them items), but the frame's last, short tile can: a post's items come first and its aliased holes last,
    so a post that ends the slot order with its items filling tile 0 leaves tile 1 its 20 (long post: 255) holes and nothing else --
    the row sort's short tile (s_end == n) in which every slot takes the hole digit and every published count is zero."""
    m = model_of(hole_scene(name))
    holes = m["S"] - m["R"]
    if name in ("tail", "long_tail"):
        nh = KI if name == "tail" else 255
        assert list(m["tile_valid"]) == [4096, 0] and m["S"] == 4096 + nh and m["R"] == 4096
        assert m["nslots"][-1] == 2 * nh and m["first_slot"][-1] == 4096 - nh and (m["slot_tiles"][4096:] == 0).all()
        assert (np.diff(m["order"]) < 0).any()
    elif name == "left_edge":
        assert m["S"] > 4096 and m["tile_valid"][0] <= 1024 and m["tile_valid"][0] > 0
    else:
        assert m["S"] > 4096 and holes >= 1000 and m["R"] >= 1000
        assert m["item_col"].min() >= SLAB[0] and (m["item_col"] + m["item_tiles"]).max() <= SLAB[1]
        assert m["item_col"].min() == SLAB[0] and (m["item_col"] + m["item_tiles"]).max() == SLAB[1]  # runs cut at both slab edges


@pytest.mark.parametrize("W,H", DIGIT_CANVASES)
def test_digit_scenes(W, H):
    m = model_of(digit_scene(W, H))
    ntx, nty = W // 8, H // 8
    n = max(ntx, nty)
    assert rr.digits(n) == ((7, 127) if n == 127 else (8, 255))
    if nty > ntx:
        assert {0, 1, n - 2, n - 1} <= set(m["item_row"].tolist()) and m["item_row"].max() == n - 1
        assert (m["row_items"][:n] >= 1).all() and m["row_items"][n:].sum() == 0 and m["nslots"].max() >= 2 * n
    else:
        assert {0, 1, n - 2, n - 1} <= set(m["item_col"].tolist())
        end = m["item_col"] + m["item_tiles"]
        assert end.max() == n and int(((end == n) & (m["item_tiles"] > 1)).sum()) == 6  # bars that end in the last column
    assert m["S"] > m["R"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("k", K_ITEMS)
def test_items_per_row_scenes(k, pattern):
    """all_rows with k = 1: two blankets alone put 4 items into row 4, so that one case has no blanket."""
    sc = items_scene(k, pattern)
    m = model_of(sc)
    np.testing.assert_array_equal(m["row_items"][:9], sc["want"]["rows"])
    assert m["row_items"][9:].sum() == 0
    row = {"row0": 0, "last_row": 8, "rows_2_6": 2, "all_rows": 4}[pattern]
    nch = int(m["chunks_per_row"][row])
    assert m["row_items"][row] == k and nch == K_CHUNKS[K_ITEMS.index(k)]
    parts, trips = rr.scan_parts(nch)
    if nch == 5:
        assert parts == [2, 2, 1, 0]
    if nch == 33:
        assert parts == [9, 9, 9, 6] and trips == [2, 2, 2, 1]
    if nch == 32:
        assert parts == [8, 8, 8, 8] and trips == [1, 1, 1, 1]
    last = np.flatnonzero(m["chunk_row"] == row)[-1]
    assert m["chunk_end"][last] - m["chunk_begin"][last] == (k - 1) % 512 + 1
    if pattern == "rows_2_6":  # rows without chunks share their successor's chunk base
        assert list(np.flatnonzero(m["chunks_per_row"])) == [2, 6]
    assert m["I"] > m["R"] or k < 7
    assert (np.diff(m["order"]) < 0).any() or m["order"].size < 3


@pytest.mark.parametrize("kind,value", [("instances", v) for v in INSTANCES] + [("placement", p) for p in PLACEMENTS] + [("short", v) for v in SHORT_CHUNKS])
def test_chunk_scenes(kind, value):
    """One chunk of 512 items with the instances the case names; a bar of 16 whose first instance has the offset the case names (a
    first instance at 2048 - L + 1 puts the bar's LAST one on 2048, the next sub-batch's first: kept as last_over_batch, and 2048 - L,
    whose last instance is the sub-batch's last, added as ends_batch); a full chunk of more than one sub-batch before a short one."""
    sc = chunk_scene(kind, value)
    m = model_of(sc)
    L = sc["want"]["lengths"]
    in_row = m["item_row"] == 1
    np.testing.assert_array_equal(m["item_tiles"][in_row], L)  # one bucket: the row's item order is the record order
    c1 = np.flatnonzero(m["chunk_row"] == 1)
    assert m["S"] == m["R"] == L.size + 8 and m["I"] == L.sum() + 8
    if kind == "instances":
        assert c1.size == 1 and m["chunk_inst"][c1[0]] == value and L.size == 512
    elif kind == "placement":
        i = np.flatnonzero(in_row)[sc["want"]["bar_item"]]
        off = int(m["item_offset"][i])
        assert c1.size == 1 and m["item_tiles"][i] == LB and off == PLACEMENTS[value]
        sb, ws = rr.SUB_BATCH, rr.EXPAND_WAVE
        if value == "at_2047":
            assert off == sb - 1
        elif value == "at_2048":
            assert off == sb
        elif value == "ends_batch":
            assert off + LB == sb
        elif value == "last_over_batch":
            assert off + LB - 1 == sb
        elif value == "half_over_batch":
            assert off + LB // 2 == sb
        else:
            assert (off + LB // 2) % ws == 0 and (off + LB // 2) % sb != 0 and (off // sb) == (0 if value.endswith("1") else 1)
    else:
        assert c1.size == 2 and m["chunk_end"][c1[1]] - m["chunk_begin"][c1[1]] == value and m["chunk_inst"][c1[0]] > rr.SUB_BATCH


def test_many_trips_scene():
    sc = trips_scene()
    m = model_of(sc)
    np.testing.assert_array_equal(m["row_items"][:9], sc["want"]["rows"])
    nch = m["chunk_row"].size
    assert nch == 45 and (m["chunks_per_row"][:9] == 5).all()
    ends = m["chunk_end"] - m["chunk_begin"]
    assert all(0 < ends[np.flatnonzero(m["chunk_row"] == r)[-1]] < 512 for r in range(9))  # every row ends in a short chunk
    _, count_wg, expand_wg = rr.grids(4)
    assert min(rr.trips(nch, count_wg)) >= 5 and min(rr.trips(nch, expand_wg)) >= 5
    for wg in (count_wg, expand_wg):  # consecutive trips of a workgroup are chunks of different rows
        assert all(m["chunk_row"][c] != m["chunk_row"][c + wg] for c in range(nch - wg))
    assert m["S"] > m["R"]


@pytest.mark.parametrize("kind,v,ts", TILE_SIZE_CASES)
def test_tile_size_scenes(kind, v, ts):
    """The items-per-row cases (rows 2 and 6) on 12 x 9 tiles of 8 and 32 pixels; the instances-per-chunk cases on 204 x 3 tiles of 8
    (the base family's canvas), 16 and 32 pixels: one sub-block per tile at 8, four from 16 on."""
    sc = tile_size_scene(kind, v, ts)
    m = model_of(sc)
    assert sc["ts"] == ts
    if kind == "items":
        assert m["row_items"][2] == m["row_items"][6] == v and m["row_items"].sum() == 2 * v
        assert m["chunks_per_row"][2] == -(-v // 512)
    else:
        c1 = np.flatnonzero(m["chunk_row"] == 1)
        assert c1.size == 1 and m["chunk_inst"][c1[0]] == v and m["chunk_end"][c1[0]] - m["chunk_begin"][c1[0]] == 512


# ---- GPU: the frames ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("S", SLOT_TOTALS)
def test_slot_totals(oracle, S):
    frames(oracle, slot_total_scene(S))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STRADDLES) + ["posts_only", "long_post"])
def test_gaussian_across_a_boundary(oracle, name):
    frames(oracle, straddle_scene(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", HOLE_SCENES)
def test_holes(oracle, name):
    frames(oracle, hole_scene(name))


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", DIGIT_CANVASES)
def test_digits(oracle, W, H):
    frames(oracle, digit_scene(W, H))


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("k", K_ITEMS)
def test_items_per_row(oracle, k, pattern):
    frames(oracle, items_scene(k, pattern))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,value", [("instances", v) for v in INSTANCES] + [("placement", p) for p in PLACEMENTS] + [("short", v) for v in SHORT_CHUNKS])
def test_instances_per_chunk(oracle, kind, value):
    frames(oracle, chunk_scene(kind, value))


@pytest.mark.gpu
def test_many_trips(oracle):
    frames(oracle, trips_scene())


@pytest.mark.gpu
@pytest.mark.parametrize("kind,v,ts", TILE_SIZE_CASES)
def test_tile_sizes(oracle, kind, v, ts):
    frames(oracle, tile_size_scene(kind, v, ts))
