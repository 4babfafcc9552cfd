"""CPU restatement of the coverage planes (include/gsplat/gs_abi.h "coverage"): per-splat contribution of one frame over a set
of canvas pixels.

Built on tests/pick_restate.py, which IS the oracle's blend (test_pick.py holds its alpha and accumulated depth to the C
oracle's, bit for bit): every pixel of P is restated with max_contrib = 256, so its contributor records are ALL the (pixel,
entry) pairs the blend accepts there with their weights w = fl(alpha T); they are folded into sum_q / hits / max_weight with
numpy integer and f32 arithmetic:  sum_q += floor(w 2^32) (the f32 product w * 2^32 is exact, w <= 0.99), hits += 1,
max_weight = max(max_weight, w).
"""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
MAX_CONTRIB = 256
COVERAGE_DTYPE = np.dtype([("sum_q", np.uint64), ("hits", np.uint32), ("max_weight", np.float32)])


def region_pixels(W, H, rect=None, mask=None, cols=None, ts=None):
    """The canvas pixels (n, 2) x, y of P = rect AND mask (AND the slab `cols`), row-major."""
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, W, H)
    assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H
    if cols is not None:
        x0, x1 = max(x0, cols[0] * ts), min(x1, min(W, cols[1] * ts))
    if x0 >= x1:
        return np.zeros((0, 2), np.uint32)
    yy, xx = np.meshgrid(np.arange(y0, y1, dtype=np.uint32), np.arange(x0, x1, dtype=np.uint32), indexing="ij")
    xy = np.stack([xx.ravel(), yy.ravel()], axis=1)
    if mask is not None:
        m = np.asarray(mask)
        assert m.shape == (H, W)
        xy = xy[m[xy[:, 1], xy[:, 0]] != 0]
    return xy


def pixel_records(ref, W, H, ts, xy, cols=None):
    """pick_restate's (results, contributor records, classes) of the pixels `xy`; no pixel may accept more than 256 entries."""
    from pick_restate import restate_ref
    res, con, cls = restate_ref(ref, W, H, ts, xy, MAX_CONTRIB, cols)
    assert (res["status"] == 0).all()
    assert res["hit_count"].size == 0 or int(res["hit_count"].max()) <= MAX_CONTRIB, "a pixel accepts more entries than gs_pick reports"
    return res, con, cls


def fold(n, xy, records, W, ts, ref=None, keep=None):
    """Folds the contributor records of the pixels (those with keep[i], default all) into planes of n splats.  Returns
    (planes, classes): the class counts the tests assert on."""
    res, con, cls = records
    xy = np.asarray(xy).astype(np.int64)
    keep = np.ones(xy.shape[0], bool) if keep is None else np.asarray(keep, bool)
    res, con, xy, rta = res[keep], con[keep], xy[keep], cls["rejected_then_accepted"][keep]
    valid = con["id"] != NONE
    pix = np.repeat(np.arange(xy.shape[0]), con.shape[1]).reshape(con.shape)[valid]
    ids = con["id"][valid].astype(np.int64)
    w = con["weight"][valid].astype(F)
    assert ids.size == int(res["hit_count"].sum()) and (ids < n).all() and (w > 0).all() and (w <= F(0.99)).all()
    planes = np.zeros(n, COVERAGE_DTYPE)
    q = (w * F(4294967296.0)).astype(np.uint64)  # one exact f32 product, then floor
    assert (q < 2 ** 32).all()
    np.add.at(planes["sum_q"], ids, q)
    np.add.at(planes["hits"], ids, np.uint32(1))
    np.maximum.at(planes["max_weight"], ids, w)
    # classes
    ntx = int(np.ceil(F(W) / F(ts)))
    tile = (xy[:, 0] // ts + (xy[:, 1] // ts) * ntx)[pix]
    block = ((xy[:, 0] // 8) + (xy[:, 1] // 8) * 100003)[pix]
    it = np.unique(np.stack([ids, tile], axis=1), axis=0)
    itb = np.unique(np.stack([ids, tile, block], axis=1), axis=0)
    tiles_per_id = np.bincount(it[:, 0], minlength=n)
    _, blocks_per_pair = np.unique(itb[:, :2], axis=0, return_counts=True)
    ib = np.unique(np.stack([ids, block], axis=1), axis=0)
    classes = {
        "pixels": int(xy.shape[0]),
        "max_list": int(res["list_length"].max()) if xy.shape[0] else 0,
        "max_hits_per_pixel": int(res["hit_count"].max()) if xy.shape[0] else 0,
        "covered": int((planes["hits"] > 0).sum()),
        "multi_tile": int((tiles_per_id >= 2).sum()),
        "multi_block": int((np.bincount(ib[:, 0], minlength=n) >= 2).sum()),
        "multi_block_one_tile": int((blocks_per_pair >= 2).sum()),
        "zero_hit_pixels": int((res["hit_count"] == 0).sum()),
        "rejected_then_accepted": int(rta.sum()),
        "more_hits_than_pixels": int((planes["hits"] > xy.shape[0]).sum()),
        "listed_never_accepted": 0,
    }
    if ref is not None:  # splats in the lists of the tiles P touches that no pixel of P accepts
        vals, rng = np.asarray(ref["sorted_values"]), np.asarray(ref["ranges"]).astype(np.int64)
        listed = np.zeros(n, bool)
        for t in np.unique(xy[:, 0] // ts + (xy[:, 1] // ts) * ntx):
            listed[vals[(int(rng[t - 1]) if t > 0 else 0):int(rng[t])]] = True
        assert listed[planes["hits"] > 0].all()
        classes["listed_never_accepted"] = int((listed & (planes["hits"] == 0)).sum())
    return planes, classes


def restate(ref, n, W, H, ts, rect=None, mask=None, cols=None):
    """(planes, classes) of P = rect AND mask on the oracle frame `ref` (oracle.render(...))."""
    xy = region_pixels(W, H, rect, mask, cols, ts)
    return fold(n, xy, pixel_records(ref, W, H, ts, xy, cols), W, ts, ref)


def words(planes):
    """The planes as u32 words [n, 4] (floats compared as bits)."""
    a = np.ascontiguousarray(planes)
    return a.view(np.uint32).reshape(a.shape[0], 4)
