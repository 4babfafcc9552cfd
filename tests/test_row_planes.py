"""The row pipeline's hand-off behind the row sort (k_rows.hip): the sorted items as a payload plane {w0, w2} and a 16-bit span plane
(first column | (tiles - 1) << 8) inside one allocation, and the column-count table M3 with rows as wide as the canvas
(64 * ceil(ntx / 64) columns).  Only the smallest shapes at which that layout can go wrong:

  * a tile row whose first item has an odd / an even index in the sorted order, with 1, 511, 512 and 513 items (the span plane's
    2-byte elements at either alignment, the chunk edges);
  * canvases of 63, 64, 65, 127, 128, 129 and 255 tile columns (the table's stride at its boundaries), each with splats that span
    columns 0 .. ntx - 1 and that land in the aliased column (column ntx of a row is column 0 of the next);
  * a frame whose row-item slots and instances outgrow the arrays it starts with: the planes after their reallocation, at another
    row capacity and so at another span-plane offset.

Scenes and their CPU model as in test_row_boundaries.py (row_scenes, rows_restate).  Every frame is rendered on the product path with
GS_FLAG_EXACT_BLEND; asserted are the frame's slot, item and instance counts, `ranges` and the gaussian of every list entry against
the model with equality, the lists through gpu_checks.check_product_lists, and the image and its f32 tap byte for byte against the
same context with GS_OPT_TILE_CULL 0 (the reference's rect binning, which never enters k_rows.hip).  Nothing here has a tolerance.
"""
import numpy as np
import pytest

from gpu_checks import check_product_lists
from row_scenes import (BAR_LOGIT, BLANKET_LOGIT, DEFAULT, FLOOR, LONG_CANVAS, _rng, bars, blankets, dots, frame_of, model_of, params, post,
                        scene)
from support import cached, mk, oracle_frame

pytestmark = pytest.mark.gpu

ID_MASK = 0x0FFFFFFF  # gs_tight.h: GS_ID_MASK (the sub-block mask sits above it)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
ROW_ITEMS = (1, 511, 512, 513)
LEAD = {"odd": 3, "even": 4}  # items in the only tile row before the one under test: its first item's index in the sorted order
ROW_BEFORE, ROW_TESTED, ROW_AFTER = 2, 5, 7


def _row_items(W, H, ts, row, k, rng):
    """k items of tile row `row`: every seventh a bar of 2 .. 6 tiles, the others dots."""
    isbar = (np.arange(k) % 7) == 6
    P = dots(ts, rng.integers(0, W // ts, k), np.full(k, row), rng)
    if isbar.any():
        P[isbar] = bars(W, H, ts, row, rng.integers(2, 7, int(isbar.sum())), rng)
    return P


def parity_scene(k, parity):
    def make():
        W, H, ts = DEFAULT
        rng = _rng(21, k, LEAD[parity])
        P = np.concatenate([_row_items(W, H, ts, ROW_BEFORE, LEAD[parity], rng), _row_items(W, H, ts, ROW_TESTED, k, rng),
                            _row_items(W, H, ts, ROW_AFTER, 5, rng)])
        P = P[rng.permutation(P.shape[0])]
        z = np.where(np.arange(P.shape[0]) % 2 == 0, 1.0, 1.5)  # two interleaved depth buckets: the item order is not the record order
        return scene("planes_%s_%d" % (parity, k), W, H, ts, P, z=z)
    return cached(("planes_parity_scene", k, parity), make)


NTX = (63, 64, 65, 127, 128, 129, 255)
STRIDE_ROWS = 3


def stride_canvas(ntx):
    ts = 16 if ntx <= 65 else 8
    return ntx * ts, STRIDE_ROWS * ts, ts


def stride_scene(ntx):
    """Records 0 and 1 are a blanket (an item of ntx tiles in every row and the aliased column's item in every row but the first) and a
    faint splat of sigma W centred on the canvas's right edge (the same, from the side); then the four edge columns of every row, 300
    dots anywhere and six bars cut by the right edge."""
    def make():
        W, H, ts = stride_canvas(ntx)
        rng = _rng(22, ntx)
        edge = np.array([0, 1, ntx - 2, ntx - 1])
        wide = np.concatenate([blankets(W, H, 1), params(W - 3.0, H / 2.0, float(W), float(W), 0.0, BLANKET_LOGIT)])
        rest = np.concatenate([dots(ts, np.tile(edge, STRIDE_ROWS), np.repeat(np.arange(STRIDE_ROWS), 4), rng),
                               dots(ts, rng.integers(0, ntx, 300), rng.integers(0, STRIDE_ROWS, 300), rng),
                               params(W - 30.3 - 8.0 * np.arange(6), ts * (np.arange(6) % STRIDE_ROWS) + ts / 2.0, 25.0, FLOOR, 0.0, BAR_LOGIT)])
        return scene("planes_ntx_%d" % ntx, W, H, ts, np.concatenate([wide, rest[rng.permutation(rest.shape[0])]]))
    return cached(("planes_stride_scene", ntx), make)


REGROW_POSTS = 2100  # x 510 slots = 1 071 000: more than the 2^20 slots a context of a small scene starts with


def regrow_scene():
    """Posts as tall as a 2 x 255 tile canvas: 255 items and 255 aliased holes each, in two interleaved depth buckets."""
    def make():
        W, H, ts = LONG_CANVAS
        pl, shape = post(W, H, ts, lambda r: r[0] == 510 and r[1] == 255)
        P = np.repeat(pl, REGROW_POSTS, axis=0)
        z = np.where(np.arange(REGROW_POSTS) % 2 == 0, 1.0, 1.5)
        return scene("planes_regrow", W, H, ts, P, z=z, post=shape)
    return cached("planes_regrow_scene", make)


# ---- the model's lists --------------------------------------------------------------------------------------------------------------
def model_lists(m, ntx, nty):
    """(ranges, gaussian of every list entry) of the model's row-sorted items: tile (r, c) lists, in item order, the items of row r whose
    run holds c; ranges[t] is the end of tile t's list."""
    row, col, tiles, g = m["item_row"], m["item_col"], m["item_tiles"], m["item_gaussian"]
    item = np.repeat(np.arange(row.size), tiles)
    q = np.arange(item.size) - np.repeat(np.cumsum(tiles) - tiles, tiles)
    tile = row[item] * ntx + col[item] + q
    order = np.argsort(tile, kind="stable")  # (the items are in row order and, inside a row, in list order)
    return np.cumsum(np.bincount(tile, minlength=ntx * nty)).astype(np.uint32), g[item][order].astype(np.uint32)


def planes_frames(oracle, sc, grids=(0, 4), **kw):
    """The scene on the product path (per entry of `grids`: the default grid, or GS_OPT_PERSISTENT_GRID g, under which a workgroup takes
    many chunks and prefetches the next one's planes): counts, ranges and list gaussians equal to the model's, the lists checked
    against the oracle's, the image equal to the same context's with the reference's binning.  Returns the context's statistics before
    the first frame and after the last."""
    from gsplat import _abi
    s, u = frame_of(sc)
    m = model_of(sc)
    W, H, ts = sc["W"], sc["H"], sc["ts"]
    ntx, nty = W // ts, H // ts
    want_ranges, want_ids = model_lists(m, ntx, nty)
    ref = oracle_frame(oracle, "rows_" + sc["name"], s, u, W, H, ts)
    r = mk(s, W, H, ts, exact=True, **kw)
    try:
        before = r.stats()
        for grid in grids:
            if grid:
                r.set_option(_abi.GS_OPT_PERSISTENT_GRID, grid)
            r.render_uniforms(u)
            r.wait()
            st = r.stats()
            print("%s grid %d: slots %d items %d instances %d (model %d %d %d) row capacity %d" % (
                sc["name"], grid, st["num_row_slots"], st["num_row_items"], st["num_intersections"], m["S"], m["R"], m["I"], st["row_capacity"]))
            assert st["tight_binning"] == 1
            assert (st["num_row_slots"], st["num_row_items"], st["num_intersections"]) == (m["S"], m["R"], m["I"])
            np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_RANGES), want_ranges)
            np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_VALUES) & np.uint32(ID_MASK), want_ids)
            check_product_lists(r, ref, oracle, W, H, ts)
            tight = (r.read_rgba8(), r.read_buffer(_abi.GS_BUF_RGB_F32))
            r.set_option(_abi.GS_OPT_TILE_CULL, 0)
            r.render_uniforms(u)
            r.wait()
            assert r.stats()["tight_binning"] == 0
            np.testing.assert_array_equal(r.read_rgba8(), tight[0])
            np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_RGB_F32), tight[1])
            r.set_option(_abi.GS_OPT_TILE_CULL, 1)
        return before, r.stats()
    finally:
        r.destroy()


# ---- the frames ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", sorted(LEAD))
@pytest.mark.parametrize("k", ROW_ITEMS)
def test_row_at_either_span_alignment(oracle, k, parity):
    """Tile row 5 holds k items and starts at item 3 (odd) or 4 (even) of the sorted order: its span elements start at byte 6 or 8 of
    their plane, and with 513 items the row's second chunk starts at item 515 or 516."""
    sc = parity_scene(k, parity)
    m = model_of(sc)
    assert list(np.flatnonzero(m["row_items"])) == [ROW_BEFORE, ROW_TESTED, ROW_AFTER]
    assert m["row_items"][ROW_TESTED] == k and m["chunks_per_row"][ROW_TESTED] == -(-k // 512)
    first = int(m["chunk_begin"][m["chunk_row"] == ROW_TESTED][0])
    assert first == LEAD[parity] and first % 2 == (parity == "odd")
    assert m["I"] > m["R"] or k < 7  # bars among the dots
    planes_frames(oracle, sc)


@pytest.mark.parametrize("ntx", NTX)
def test_table_stride_boundaries(oracle, ntx):
    """ntx tile columns (tile 16 up to 65, tile 8 beyond), three tile rows: the table's rows are 64, 128 or 256 columns wide, and ntx
    = 64 and 128 fill them to the last column."""
    sc = stride_scene(ntx)
    m = model_of(sc)
    assert sc["W"] // sc["ts"] == ntx
    wide = np.isin(m["item_gaussian"], (0, 1))
    for g in (0, 1):  # both wide splats: every column of every row, and the aliased column's item in rows 1 and 2
        mine = m["item_gaussian"] == g
        assert int((mine & (m["item_col"] == 0) & (m["item_tiles"] == ntx)).sum()) == STRIDE_ROWS
        assert sorted(m["item_row"][mine & (m["item_tiles"] == 1)]) == [1, 2] and (m["item_col"][mine & (m["item_tiles"] == 1)] == 0).all()
    rest_col, rest_end = m["item_col"][~wide], (m["item_col"] + m["item_tiles"])[~wide]
    assert {0, 1, ntx - 2, ntx - 1} <= set(rest_col.tolist()) and rest_end.max() == ntx
    assert int(((rest_end == ntx) & (m["item_tiles"][~wide] > 1)).sum()) >= 3  # bars that end in the last column
    assert 300 <= m["R"] <= 512 * STRIDE_ROWS and (m["chunks_per_row"][:STRIDE_ROWS] == 1).all()
    planes_frames(oracle, sc)


def test_planes_after_regrowth(oracle):
    """1 071 000 slots against the 2^20 the context starts with, 535 500 instances against max_intersections = 4096: gs_wait grows the
    arena, the planes (whose span plane then starts at another offset) and the lists, and renders the frame again.  The second entry
    of `grids` renders it once more with the grown arrays."""
    sc = regrow_scene()
    m = model_of(sc)
    assert sc["want"]["post"][0] == 510 and m["S"] == 510 * REGROW_POSTS > (1 << 20) and m["R"] == m["I"] == 255 * REGROW_POSTS
    before, st = planes_frames(oracle, sc, grids=(0, 0), max_intersections=4096)
    assert before["row_capacity"] < m["S"] <= st["row_capacity"] and before["capacity"] < m["I"] <= st["capacity"]
