"""Frames whose (gaussian, tile) instance count passes 2^30 and 2^32, through every binning chain.

Every chain carries saturating 32-bit arithmetic for such frames (k_binning.hip: the scan's sat_add and the emission's capacity clamp;
k_gsort.hip: "Saturation" and its sat32 sites; k_rows.hip: row_tables, rbase, ranges and the expansion's clamp; gs_tile_range), and
gs_wait refuses them with GS_ERR_CAPACITY (gs_frame.hip wait_one: need >= 2^30).  The scenes (limit_scenes.py) are blankets that cover
the whole tile grid plus one-instance fillers, so the count is known to the unit.  Nothing here has a tolerance: every expected number
is an integer computed exactly.

THE TABLE.  A blanket counts 65 536 instances in the reference's binning of the 2040 x 2040 canvas, 65 792 on 2048 x 2040, and 65 279
in the tight row pipeline (limit_scenes.py says why it is not the number of tiles); the counts at the limits follow from that:

  reference's binning, 2040 x 2040         blankets  fillers   true I                       reported
    first_over                               16 384        0   2^30 (16 383 blankets: below)   exact
    under_mark                               65 535   64 515   2^32 - 1021                     exact, not the marker
    at_mark                                  65 535   65 535   2^32 - 1                        exact (equals the marker)
    at_2_32_total, at_2_32_row               65 535   65 536   2^32                            0xFFFFFFFF
    past_one                                 65 537        0   2^32 + 65 536                   0xFFFFFFFF
    past_halves, past_many, past_many_last   65 537    3 000   2^32 + 68 536                   0xFFFFFFFF
  reference's binning, 2048 x 2040 (what a product frame of 256 tile columns falls back to)
    wide_first_over                          16 321        0   1 073 791 232 (16 320: below)   exact
    wide_at_mark / wide_at_2_32              65 280   65 535 / 65 536   2^32 - 1 / 2^32        exact / 0xFFFFFFFF
    wide_past                                65 282    3 000   2^32 + 69 048                   0xFFFFFFFF
  row pipeline, 2040 x 2040
    t_first_over                             16 449        0   1 073 774 271 (16 448: below)   exact
    t_under_mark                             65 794        0   2^32 - 770                      exact
    t_at_mark / t_at_2_32                    65 794    769 / 770   2^32 - 1 / 2^32             exact / 0xFFFFFFFF
    t_past                                   65 795        0   2^32 + 64 509                   0xFFFFFFFF

Depth layouts (one bucket; 200 + 300 buckets; two buckets with the fillers in front; "halves": the fillers in front and the blankets
of the first and the second half of the indices in two buckets), index layouts (blankets first, last, interleaved) and the run grid
(GS_OPT_PERSISTENT_GRID default, 4, 12) move the point of saturation through the gaussian-level sort: test_every_site_is_reached
asserts, from limit_scenes.gsort_model, that the cases reach a bucket's row over the runs, the base scan over buckets, a run's carried
base and the total alone (and, on the wide canvas, a record's own prefix inside a chunk: `off`).

NOT IN SCOPE, with the arithmetic that keeps each out of a test:
  * the largest frame that is still ACCEPTED, I just under 2^30: its (key, value) arrays are 4 x 4 GB and no oracle renders it;
  * saturation INSIDE one chunk's prefix of k_gsort.hip (P / ptot and the `py[i + 1] == 0xFFFFFFFF` branch): 2048 consecutive gaussians
    of 2^32 / 2048 = 2.1 M tiles each, a canvas of 1449 x 1449 tiles (gsort_model asserts that no chunk of a case gets there);
  * saturation of the dense sort's ROW-SLOT quantity: 2^32 / 255 slots = 16.8 M splats of 255 rows;
  * in k_rows.hip, M3, tileoff and rowtot (sums inside ONE tile row): 2^32 / 256 tiles = 16.8 M blankets.  What these frames reach
    there is rbase, the frame's I, `ranges` and the expansion's capacity clamp;
  * the ticket path (gs_render_host / gs_wait_ticket) does not report overflows by design;
  * the list CONTENTS of a refused frame on the product paths.  gs_abi.h calls them truncated and not to be used, and the row
    expansion forms its destination slot in 32 bits from the saturated rbase (k_rows.hip `tstart`, "wraps are harmless"): past 2^32
    its stores stay inside the arrays (the clamp) but need not land where an unbounded list would put them.  Only the debug frame,
    whose taps are the reference's, is held to the first `capacity` pairs of the emission.

MEASURED (MI355X; every over-limit frame returned GS_ERR_CAPACITY, -8, naming the 2^30 limit; wall time of the gpu test's call):
  case             true I          reported I     debug frames   product frames, cull 0 (exact / fused)   row pipeline (exact / fused)
  first_over       1 073 741 824   1 073 741 824  0.30 s         0.13 / 0.18 s
  under_mark       4 294 966 275   4 294 966 275  0.40 s         0.13 s
  at_mark          4 294 967 295   4 294 967 295  0.33 s         0.14 s
  at_2_32_total    4 294 967 296   4 294 967 295  0.32 s         0.15 / 0.16 s
  at_2_32_row      4 294 967 296   4 294 967 295  0.32 s         0.12 s
  past_one         4 295 032 832   4 294 967 295  0.28 s         0.14 s
  past_halves      4 295 035 832   4 294 967 295  0.26 s         0.14 / 0.16 s
  past_many        4 295 035 832   4 294 967 295  0.30 s         0.13 s
  past_many_last   4 295 035 832   4 294 967 295  0.31 s         0.13 s
  wide_first_over  1 073 791 232   1 073 791 232  0.22 s         0.14 s (cull 0 and 1)
  wide_at_mark     4 294 967 295   4 294 967 295  0.33 s         0.16 s
  wide_at_2_32     4 294 967 296   4 294 967 295  0.27 s         0.15 s
  wide_past        4 295 036 344   4 294 967 295  0.27 s         0.17 / 0.19 s
  t_first_over     1 073 774 271   1 073 774 271                                                          1.02 / 0.63 s (pre-grown: 0.15 s)
  t_under_mark     4 294 966 526   4 294 966 526                                                          2.48 s
  t_at_mark        4 294 967 295   4 294 967 295                                                          2.36 s
  t_at_2_32        4 294 967 296   4 294 967 295                                                          2.32 s
  t_past           4 295 031 805   4 294 967 295                                                          2.36 / 2.23 s
  one wait over three frames: 0.27 s (reference's binning), 0.37 s (row pipeline); ring 0.24 s; graph replay 0.26 s; the batch's wait
  returned -8, its last frame (I = 592 833, row pipeline 592 155) was the oracle's, max_intersections_seen read 4 294 967 295.
Before the fixes this module brought (the commit that added it): past_one's debug frame listed 4 177 855 on-canvas entries instead of
4 177 856 -- gs_emit_kernel formed its destination slot in 32 bits, 0xFFFFFFFF + e wrapped past the capacity clamp and overwrote the
head of the list; a second gs_wait after a refusal on a ring member repeated the refusal; max_intersections_seen read the last ring
member's maximum only.
"""
import time

import numpy as np
import pytest

import limit_scenes as ls
from gpu_checks import check_product_lists, check_stages
from limit_scenes import LIMIT, MARK, ROWS, TS, WIDE, Case
from support import cached, code_of, mk, oracle_frame

REF_CASES = [
    Case("first_over", ROWS, 16384, 0, "one", "first"),
    Case("under_mark", ROWS, 65535, 64515, "many", "mixed"),
    Case("at_mark", ROWS, 65535, 65535, "two", "last"),
    Case("at_2_32_total", ROWS, 65535, 65536, "two", "first"),
    Case("at_2_32_row", ROWS, 65535, 65536, "one", "mixed"),
    Case("past_one", ROWS, 65537, 0, "one", "first"),
    Case("past_halves", ROWS, 65537, 3000, "halves", "first"),
    Case("past_many", ROWS, 65537, 3000, "many", "mixed"),
    Case("past_many_last", ROWS, 65537, 3000, "many", "last"),
    Case("wide_first_over", WIDE, 16321, 0, "one", "first"),
    Case("wide_at_mark", WIDE, 65280, 65535, "two", "last"),
    Case("wide_at_2_32", WIDE, 65280, 65536, "many", "mixed"),
    Case("wide_past", WIDE, 65282, 3000, "halves", "first"),
]
TIGHT_CASES = [
    Case("t_first_over", ROWS, 16449, 0, "one", "first"),
    Case("t_under_mark", ROWS, 65794, 0, "many", "first"),
    Case("t_at_mark", ROWS, 65794, 769, "two", "last"),
    Case("t_at_2_32", ROWS, 65794, 770, "one", "mixed"),
    Case("t_past", ROWS, 65795, 0, "halves", "first"),
]
TRUE_I = {"first_over": 1 << 30, "under_mark": (1 << 32) - 1021, "at_mark": (1 << 32) - 1, "at_2_32_total": 1 << 32, "at_2_32_row": 1 << 32,
          "past_one": (1 << 32) + 65536, "past_halves": (1 << 32) + 68536, "past_many": (1 << 32) + 68536, "past_many_last": (1 << 32) + 68536,
          "wide_first_over": 1073791232, "wide_at_mark": (1 << 32) - 1, "wide_at_2_32": 1 << 32, "wide_past": (1 << 32) + 69048,
          "t_first_over": 1073774271, "t_under_mark": (1 << 32) - 770, "t_at_mark": (1 << 32) - 1, "t_at_2_32": 1 << 32, "t_past": (1 << 32) + 64509}
REF_BLANKET = {ROWS: 256 * 256, WIDE: 257 * 256}
TIGHT_BLANKET = (510, 509, 255 * 255 + 254)  # slots, items, instances: two slots a tile row, the last row's aliased slot a hole
# the run grids of the gaussian-level sort a case is rendered with (0: the default), and the site limit_scenes.gsort_model names for each
GRIDS = {"at_2_32_total": {0: "total", 4: "total"}, "at_2_32_row": {0: "row", 12: "row"}, "past_one": {0: "row", 4: "row"},
         "past_halves": {0: "base", 4: "carried", 12: "carried"}, "past_many": {0: "base", 4: "base", 12: "base"}, "past_many_last": {0: "base"},
         "wide_at_2_32": {0: "total", 4: "total"}, "wide_past": {0: "record", 4: "record"}}
BY_NAME = {c.name: c for c in REF_CASES + TIGHT_CASES}
ids = lambda cases: [c.name for c in cases]


def grids_of(case):
    return GRIDS.get(case.name, {0: None})


def default_capacities(n):
    """gs_context.hip: max(4 N, 2^22) entries and max(2 N, 2^20) row slots (a multiple of 16)."""
    return max(4 * n, 1 << 22), (max(2 * n, 1 << 20) + 15) // 16 * 16


def tile_lists(ranges, capacity):
    """gs_tile_range, restated: tile t's list is [ranges[t - 1], min(ranges[t], capacity)), ranges[-1] = 0."""
    r = ranges.astype(np.int64)
    return np.concatenate([[0], r[:-1]]), np.minimum(r, capacity)


def assert_ranges_safe(ranges, capacity):
    start, end = tile_lists(ranges, capacity)
    assert (np.diff(ranges.astype(np.int64)) >= 0).all(), "ranges decrease"
    assert (end <= capacity).all() and (np.maximum(end - start, 0).sum() <= capacity)


# ---- CPU: every scene is what the table says -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REF_CASES + TIGHT_CASES, ids=ids(REF_CASES + TIGHT_CASES))
def test_scene_counts(oracle, case):
    """Every blanket's count is the reference's clamped rect, every filler's is 1, every gaussian is in the bucket its layout names,
    alpha >= 1/255 on every pixel of every blanket with a factor of 100 to spare, and the frame's true I -- in the reference's binning
    and, for the row pipeline's cases, from gs_tight.h on the host -- is the table's, "first past the limit" included."""
    W, H = case.canvas
    _, _, kind, b = ls.build(case)
    p = ls.projection(oracle, case)
    assert kind.size == case.blankets + case.fillers and int((kind == 0).sum()) == case.blankets
    assert (p["counts"][kind == 0] == REF_BLANKET[case.canvas]).all() and (p["counts"][kind == 1] == 1).all()
    assert (p["bucket"] == b).all()
    assert ls.blanket_alpha_floor(p["gdata"][kind == 0], W, H) >= 100.0 / 255.0
    I_ref = int(p["counts"].sum())
    assert I_ref == case.blankets * REF_BLANKET[case.canvas] + case.fillers
    if case.name.startswith("t_"):
        sh = ls.tight_shapes(case)
        assert (sh[kind == 0] == TIGHT_BLANKET).all() and (sh[kind == 1] == (1, 1, 1)).all()
        S, R, I = ls.model_slots(case)
        assert I == TRUE_I[case.name] == case.blankets * TIGHT_BLANKET[2] + case.fillers and S == 510 * case.blankets + case.fillers
        assert int(ls.tight_tile_counts(case).sum()) == I
        assert I_ref >= LIMIT  # (what the reference's binning makes of the same splats is over the limit as well)
        first_blanket = TIGHT_BLANKET[2]
    else:
        assert I_ref == TRUE_I[case.name]
        first_blanket = REF_BLANKET[case.canvas]
    I = TRUE_I[case.name]
    assert I >= LIMIT
    if "first_over" in case.name:  # the first count that is refused: one blanket less is accepted
        assert case.fillers == 0 and I - first_blanket < LIMIT <= I
    if "under_mark" in case.name:
        assert LIMIT < I < MARK
    if "at_mark" in case.name:
        assert I == MARK
    if "at_2_32" in case.name:
        assert I == MARK + 1
    if "past" in case.name:
        assert MARK + 1 < I < MARK + 1 + 2 * first_blanket  # within two blankets of 2^32


@pytest.mark.parametrize("case", REF_CASES + TIGHT_CASES, ids=ids(REF_CASES + TIGHT_CASES))
def test_recovery_frames_fit(oracle, case):
    """The same splats under scale_modifier 2e-5 are a legal frame that fits the default capacity without regrowth."""
    s, u, kind, _ = ls.build(case)
    W, H = case.canvas
    _, cnt = oracle.preprocess(s, ls.small_uniforms(u), W, H, TS)
    assert (cnt[kind == 0] >= 1).all() and (cnt[kind == 0] <= 9).all() and (cnt[kind == 1] == 1).all()
    assert int(cnt.sum()) < default_capacities(kind.size)[0]


def test_every_site_is_reached(oracle):
    """The Python-int model of the gaussian-level sort names, for every (case, run grid) the gpu tests render, the first partial sum
    that reaches 2^32; together they reach all four, under_mark and at_mark reach none, and the model's total and per-record prefixes
    are min(exact, 2^32 - 1) of the plain sums."""
    seen = set()
    for case in REF_CASES:
        p = ls.projection(oracle, case)
        for grid, site in grids_of(case).items():
            m = ls.gsort_model(p["bucket"], p["counts"], grid or ls.DEFAULT_GRID)
            assert m["total"] == min(TRUE_I[case.name], MARK)
            if grid:
                assert m["cpr"] > 1 and m["runs"] <= grid  # several chunks a run: bases are carried
            else:
                assert m["cpr"] == 1
            if case.name in GRIDS:
                assert m["site"] == site, (case.name, grid, m["site"])
                seen.add(site)
            else:
                assert m["site"] is None and TRUE_I[case.name] <= MARK
            # the records' prefixes: the exclusive prefix of the counts in (bucket, index) order, saturated
            o = np.lexsort((np.arange(p["counts"].size), p["bucket"]))
            exact = np.cumsum(p["counts"][o]) - p["counts"][o]
            assert (m["off"][o] == np.minimum(exact, MARK)).all()
    assert seen == set(ls.SITES) | {"record"}


def test_wrapping_arithmetic_would_be_noticed(oracle):
    """Teeth.  For every quantity a gpu test asserts, the same model with wrapping adds (& 0xFFFFFFFF) gives another value in at least
    one case: the reported I of the scan, of the sort and of the row pipeline, the error code that follows from it, the offsets tap,
    the records' prefixes, the row pipeline's ranges and their monotonicity, and how many entries a truncated debug frame lists."""
    differs = {k: 0 for k in ("scan I", "error code", "offsets", "sort I", "sort prefixes", "listed entries", "rows I", "rows ranges", "rows monotonic")}
    refused = lambda I: I >= LIMIT
    for case in REF_CASES:
        p = ls.projection(oracle, case)
        cap = default_capacities(p["counts"].size)[0]
        (off_s, I_s), (off_w, I_w) = ls.scan_model(p["counts"]), ls.scan_model(p["counts"], saturate=False)
        assert I_s == min(TRUE_I[case.name], MARK)
        differs["scan I"] += I_s != I_w
        differs["error code"] += refused(I_s) != refused(I_w)
        differs["offsets"] += bool((off_s != off_w).any())
        differs["listed entries"] += min(I_s, cap) != min(I_w, cap)
        for grid in grids_of(case):
            a = ls.gsort_model(p["bucket"], p["counts"], grid or ls.DEFAULT_GRID)
            w = ls.gsort_model(p["bucket"], p["counts"], grid or ls.DEFAULT_GRID, saturate=False)
            differs["sort I"] += a["total"] != w["total"]
            differs["sort prefixes"] += bool((a["off"] != w["off"]).any())
    for case in TIGHT_CASES:
        ends = np.cumsum(ls.tight_tile_counts(case))
        sat, wrap = ls.fold(ends, True), ls.fold(ends, False)
        differs["rows I"] += int(sat[-1]) != int(wrap[-1])
        differs["error code"] += refused(int(sat[-1])) != refused(int(wrap[-1]))
        differs["rows ranges"] += bool((sat != wrap).any())
        assert (np.diff(sat) >= 0).all()
        differs["rows monotonic"] += bool((np.diff(wrap) < 0).any())
    assert all(v > 0 for v in differs.values()), differs


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def _renderer(case, exact=True):
    s, u, _, _ = ls.build(case)
    W, H = case.canvas
    return mk(s, W, H, TS, exact=exact), u


def _refused(r, I, tight, name):
    """gs_wait on an over-limit frame: GS_ERR_CAPACITY naming the 2^30 limit, I reported saturated, nothing counted as truncated."""
    code, msg = code_of(r.wait)
    st = r.stats()
    print("%s: true I %d reported %d code %d (%s)" % (name, I, st["num_intersections"], code, msg.split(": ", 1)[-1]))
    assert code == -8 and "2^30" in msg, (code, msg)  # GS_ERR_CAPACITY: neither GS_ERR_TRUNCATED (-9) nor GS_ERR_DEVICE_FAULT (-7)
    assert st["num_intersections"] == min(I, MARK)
    assert st["max_intersections_seen"] == min(I, MARK)
    assert st["truncated_frames"] == 0
    assert st["tight_binning"] == tight
    return st


def _recover(oracle, r, case, u, debug, exact=True):
    """The next frame on the same context: the same splats made small, against the oracle; the wait is clean."""
    from gsplat import _abi
    s, _, _, _ = ls.build(case)
    W, H = case.canvas
    us = ls.small_uniforms(u)
    ref = oracle_frame(oracle, "limit_small_" + case.name, s, us, W, H, TS, want_illcond=True)
    r.set_option(_abi.GS_OPT_RESET_TIMING, 0)
    r.render_uniforms(us, debug=debug)
    r.wait()
    if exact:
        check_stages(r, ref, exact_image=True, debug=debug, oracle=oracle, W=W, H=H, ts=TS)
    else:
        # the fused blend is not the oracle's bit for bit: its lists are checked against the oracle, its image against the same
        # frame of a fresh fused context that never met an over-limit frame -- byte for byte, the f32 tap included
        check_product_lists(r, ref, oracle, W, H, TS)
        tight = r.stats()["tight_binning"]

        def fresh():
            f = mk(s, W, H, TS, exact=False)
            f.set_option(_abi.GS_OPT_TILE_CULL, tight)
            f.render_uniforms(us)
            f.wait()
            out = f.read_rgba8(), f.read_buffer(_abi.GS_BUF_RGB_F32)
            f.destroy()
            return out
        rgba8, rgbf = cached(("limit_fresh_fused", case.name, tight), fresh)
        np.testing.assert_array_equal(r.read_rgba8(), rgba8)
        np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_RGB_F32), rgbf)
    assert r.stats()["truncated_frames"] == 0
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("case", REF_CASES, ids=ids(REF_CASES))
def test_debug_frames(oracle, case):
    """gs_render_debug: the scan (k_binning.hip sat_add) and the index-order emission.  The counts tap is the oracle's, the offsets tap
    min(exact prefix, 2^32 - 1) word for word, the unsorted taps hold the first `capacity` pairs of the reference's emission (what a
    frame that does not fit still writes, and nothing else), the ranges are safe and end at the listed entries that lie on the
    canvas; the capacities do not move and the next debug frame is the oracle's in every tap."""
    from gsplat import _abi
    t0 = time.time()
    p = ls.projection(oracle, case)
    I = TRUE_I[case.name]
    cap, row_cap = default_capacities(p["counts"].size)
    r, u = _renderer(case)
    try:
        r.render_uniforms(u, debug=True)
        st = _refused(r, I, 0, case.name + " debug")
        assert (st["capacity"], st["row_capacity"]) == (cap, row_cap)
        np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_TILE_COUNTS), p["counts"].astype(np.uint32))
        np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_TILE_OFFSETS), ls.scan_model(p["counts"])[0].astype(np.uint32))
        ranges = r.read_buffer(_abi.GS_BUF_RANGES)
        assert_ranges_safe(ranges, cap)
        keys, vals = ls.emission_prefix(oracle, case, cap)
        T = (case.canvas[0] // TS) * (case.canvas[1] // TS)
        assert int(ranges[-1]) == int((keys // 1000 < T).sum())
        np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_KEYS_UNSORTED), keys)
        np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_VALUES_UNSORTED), vals)
        _recover(oracle, r, case, u, debug=True)
        assert (r.stats()["capacity"], r.stats()["row_capacity"]) == (cap, row_cap)
    finally:
        r.destroy()
    print("%s: %.1f s" % (case.name, time.time() - t0))


def _with_blends(cases, fused):
    """Every case with the EXACT blend, the named ones with the fused blend as well."""
    both = [(c, True) for c in cases] + [(c, False) for c in cases if c.name in fused]
    return dict(argnames="case,exact", argvalues=both, ids=["%s-%s" % (c.name, "exact" if e else "fused") for c, e in both])


@pytest.mark.gpu
@pytest.mark.parametrize(**_with_blends(REF_CASES, ("first_over", "at_2_32_total", "past_halves", "wide_past")))
def test_reference_binning_product_frames(oracle, case, exact):
    """gs_render with GS_OPT_TILE_CULL 0: the index-order emission (GS_OPT_EMIT_ORDER 1), the gaussian-level sort and the balanced
    emission (0) on every run grid of the case, and the automatic choice (2).  On the 256-column canvas the same with GS_OPT_TILE_CULL 1:
    the frame falls back to this binning by itself."""
    from gsplat import _abi
    t0 = time.time()
    I = TRUE_I[case.name]
    s, _, _, _ = ls.build(case)
    cap, row_cap = default_capacities(s.shape[0])
    r, u = _renderer(case, exact)
    try:
        culls = (0, 1) if case.canvas == WIDE else (0,)
        for cull in culls:
            r.set_option(_abi.GS_OPT_TILE_CULL, cull)
            for order, grids in ((1, (0,)), (0, tuple(grids_of(case))), (2, (0,))):
                for grid in grids:
                    r.set_option(_abi.GS_OPT_EMIT_ORDER, order)
                    r.set_option(_abi.GS_OPT_PERSISTENT_GRID, grid or ls.DEFAULT_GRID)
                    r.set_option(_abi.GS_OPT_RESET_TIMING, 0)
                    r.render_uniforms(u)
                    st = _refused(r, I, 0, "%s cull %d order %d grid %d" % (case.name, cull, order, grid))
                    assert (st["capacity"], st["row_capacity"]) == (cap, row_cap)
                    if order < 2:
                        assert st["depth_ordered"] == 1 - order
                    ranges = r.read_buffer(_abi.GS_BUF_RANGES)
                    assert_ranges_safe(ranges, cap)
                    assert 0 < int(ranges[-1]) <= cap
        r.set_option(_abi.GS_OPT_PERSISTENT_GRID, ls.DEFAULT_GRID)
        _recover(oracle, r, case, u, debug=False, exact=exact)
        assert (r.stats()["capacity"], r.stats()["row_capacity"]) == (cap, row_cap)
    finally:
        r.destroy()
    print("%s %s: %.1f s" % (case.name, "exact" if exact else "fused", time.time() - t0))


def _rows_frame(r, u, case, grid, name):
    from gsplat import _abi
    r.set_option(_abi.GS_OPT_PERSISTENT_GRID, grid or ls.DEFAULT_GRID)
    r.set_option(_abi.GS_OPT_RESET_TIMING, 0)
    r.render_uniforms(u)
    st = _refused(r, TRUE_I[case.name], 1, name)
    S, R, _ = ls.model_slots(case)
    assert (st["num_row_slots"], st["num_row_items"]) == (S, R)
    ranges = r.read_buffer(_abi.GS_BUF_RANGES)
    assert_ranges_safe(ranges, st["capacity"])
    np.testing.assert_array_equal(ranges, ls.fold(np.cumsum(ls.tight_tile_counts(case)), True).astype(np.uint32))
    return st


@pytest.mark.gpu
@pytest.mark.parametrize(**_with_blends(TIGHT_CASES, ("t_first_over", "t_past")))
def test_row_pipeline_frames(oracle, case, exact):
    """gs_render with GS_OPT_TILE_CULL 1 on 255 x 255 tiles.  The first frame overflows the row-item arena as well (510 slots a blanket
    against 2^20): gs_wait grows the arena for the slots and the lists for the instances that fitted, renders again and refuses.  The
    frames after it meet arrays that hold every slot: only the instance count is over the limit, and nothing grows.  Slots, items and I
    are the model's, and `ranges` is min(exact inclusive prefix of the tile counts, 2^32 - 1) word for word."""
    from gsplat import _abi
    t0 = time.time()
    S, _, _ = ls.model_slots(case)
    cap, row_cap = default_capacities(case.blankets + case.fillers)
    assert S > row_cap
    r, u = _renderer(case, exact)
    try:
        st = _rows_frame(r, u, case, 0, case.name + " rows, arena overflow")
        assert st["row_capacity"] >= S and cap <= st["capacity"] < LIMIT
        for grid in (0, 4):
            st2 = _rows_frame(r, u, case, grid, "%s rows grid %d" % (case.name, grid))
            assert (st2["capacity"], st2["row_capacity"]) == (st["capacity"], st["row_capacity"])
        r.set_option(_abi.GS_OPT_PERSISTENT_GRID, ls.DEFAULT_GRID)
        _recover(oracle, r, case, u, debug=False, exact=exact)
        assert (r.stats()["capacity"], r.stats()["row_capacity"]) == (st["capacity"], st["row_capacity"])
    finally:
        r.destroy()
    print("%s %s: %.1f s" % (case.name, "exact" if exact else "fused", time.time() - t0))


@pytest.mark.gpu
def test_row_pipeline_with_a_pregrown_arena(oracle):
    """The arena grown by a LEGAL frame first: the same splats with the horizontal focal length at 1e-7 are one tile wide and 255 rows
    tall -- the same 510 slots a blanket (the rect is the whole grid either way), 255 instances instead of 65 279.  The over-limit
    frame that follows overflows nothing but the instance limit, is refused at the first attempt, and no capacity moves."""
    from gsplat import _abi
    case = BY_NAME["t_first_over"]
    r, u = _renderer(case)
    thin = np.array(u, np.float32, copy=True)
    thin[37] *= np.float32(1e-7)
    sh = ls.tight_shapes(case, thin)
    assert (sh == (510, 255, 255)).all()
    try:
        r.render_uniforms(thin)
        r.wait()
        st = r.stats()
        assert st["tight_binning"] == 1 and (st["num_row_slots"], st["num_row_items"], st["num_intersections"]) == tuple(int(x) for x in sh.sum(axis=0))
        assert st["row_capacity"] >= ls.model_slots(case)[0] and st["capacity"] >= st["num_intersections"]
        frames = st["frames"]
        st2 = _rows_frame(r, u, case, 0, "t_first_over rows, arena pre-grown")
        assert (st2["capacity"], st2["row_capacity"]) == (st["capacity"], st["row_capacity"])
        assert st2["frames"] == frames + 1  # refused at the first attempt: nothing was rendered twice
        _recover(oracle, r, case, u, debug=False)
    finally:
        r.destroy()


def _three_frames(oracle, r, case, u, I_over):
    """[fits, over the limit, fits] without a wait in between, then ONE gs_wait: it fails with GS_ERR_CAPACITY (the batch's largest I is
    what it refuses; no frame is counted as truncated and nothing grows), the last frame is complete, and the next waits are clean."""
    from gsplat import _abi
    s, _, _, _ = ls.build(case)
    W, H = case.canvas
    us = ls.small_uniforms(u)
    ref = oracle_frame(oracle, "limit_small_" + case.name, s, us, W, H, TS, want_illcond=True)
    r.set_option(_abi.GS_OPT_RESET_TIMING, 0)
    before = r.stats() if r.numFrames else None  # (None: nothing rendered yet, the capacities are the defaults)
    for v in (us, u, us):
        r.render_uniforms(v)
    code, msg = code_of(r.wait)
    assert code == -8 and "2^30" in msg, (code, msg)
    st = r.stats()
    print("%s: batch of three, code %d, last I %d, largest seen %d" % (case.name, code, st["num_intersections"], st["max_intersections_seen"]))
    assert st["max_intersections_seen"] == min(I_over, MARK)
    assert st["truncated_frames"] == 0
    want = (before["capacity"], before["row_capacity"]) if before is not None else default_capacities(s.shape[0])
    assert (st["capacity"], st["row_capacity"]) == want
    check_stages(r, ref, exact_image=True, debug=False, oracle=oracle, W=W, H=H, ts=TS)  # the LAST frame, also in its lists
    r.wait()  # reported once
    r.render_uniforms(us)
    r.wait()
    check_stages(r, ref, exact_image=True, debug=False, oracle=oracle, W=W, H=H, ts=TS)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("chain", ["reference", "rows"])
def test_one_wait_over_three_frames(oracle, chain):
    """GS_OPT_FRAMES_IN_FLIGHT 1: all three frames on one context.  rows: a first over-limit frame, waited for alone, grows the arena,
    so that the batch's over-limit frame reports its whole I."""
    from gsplat import _abi
    case = BY_NAME["past_halves" if chain == "reference" else "t_past"]
    r, u = _renderer(case)
    try:
        r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
        r.set_option(_abi.GS_OPT_TILE_CULL, 0 if chain == "reference" else 1)
        if chain == "rows":
            _rows_frame(r, u, case, 0, "t_past rows, before the batch")
        st = _three_frames(oracle, r, case, u, TRUE_I[case.name])
        assert st["frames_in_flight"] == 1 and st["tight_binning"] == (chain == "rows")
    finally:
        r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ring", "graph"])
def test_ring_and_graph_replay(oracle, mode):
    """The same three frames through the default ring of three (one member each: the error is the middle member's, the statistics
    still name the largest I of the batch), and replayed from a captured frame graph on one context (GS_OPT_FRAME_GRAPH 1, frames in
    flight 1: a first small frame is captured, the over-limit frame is a replay with other uniforms)."""
    from gsplat import _abi
    case = BY_NAME["past_halves"]
    r, u = _renderer(case)
    try:
        r.set_option(_abi.GS_OPT_TILE_CULL, 0)
        if mode == "graph":
            r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
            r.set_option(_abi.GS_OPT_FRAME_GRAPH, 1)
            r.set_option(_abi.GS_OPT_EMIT_ORDER, 0)  # (the emission order is part of a capture's identity: fixed, so that every frame replays)
            r.render_uniforms(ls.small_uniforms(u))
            r.wait()
            g0 = r.stats()["graph_frames"]
            assert g0 == 1
        st = _three_frames(oracle, r, case, u, TRUE_I[case.name])
        if mode == "graph":
            assert st["graph_frames"] == g0 + 3 and st["frames_in_flight"] == 1
        else:
            assert st["frames_in_flight"] == 3
    finally:
        r.destroy()
