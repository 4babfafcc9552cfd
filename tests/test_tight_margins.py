"""The tight binning (csrc/gs_tight.h) at the margins of its conservative geometry.

gs_tight.h makes an instance disappear before the blend sees it, and each of its tests is conservative only by an explicit margin:
+0.01 on ln(255 op), 1e-5 of the terms on the chord's discriminant, the strip's slack, the inflation of xmax / ymax, eR around the
extreme point's dy, and Dlo > 0.25 D before the ellipse is trusted at all.  The margin scene (support.tight_margin_scene, built in
pixel space like the blend culls' scenes) aims at each of them, in labelled families:

  * contour: the opacity set so that ln(255 op) = qmin + delta over one 8x8 block, delta = +-10^U(-7,-2) max(1, qmin), on blocks the
    contour touches at a pixel and on which a tile hangs;
  * extreme_x / extreme_y: the ellipse's rightmost / leftmost (topmost / bottommost) point within 1e-3 .. 0.3 px of a strip
    boundary row (the first or last pixel row of a tile) and of a column's first or last pixel centre;
  * cancellation: thin diagonal splats swept across Dlo > 0.25 D, landed like the contour family within 10^U(-7,-4.5), and a part
    placed by its tip where the extents' extreme point and the chords' ellipse part (the `dyR +- eR` branches: support._tip_centres);
  * opacity_floor: ln(255 op) in [-0.02, 0.02], tiny splats centred on corner pixels of tiles and sub-blocks and half a pixel off;
  * alias: rects that reach column ntx, whose aliased instance IS tile (ty + 1, 0) at the far left.

The unmarked tests PROVE, with the oracle's lists, oracle.instance_masks and f64 geometry, that the scene reaches these margins (the
counts are conditions on the seeded scene, not measurements of the code under test).  tests/test_tight_host.py runs the header's host
emulation on the scene and shows that it has teeth; the GPU tests below run the kernels on it.  profiles/tight_margins.txt holds the
figures.
"""
import numpy as np
import pytest

from support import (F, SLAB_COLS, TIGHT_FAMILIES, block_qmin_pixels, cached, facing_corner, gdata_f32, mk, tight_geometry, tight_ref,
                     tight_scene)

NAME = "tight_margins"
TILES = (8, 16, 32)
C255 = np.float32(1.0 / 255.0)


def _fam(t, name):
    return t["family"] == TIGHT_FAMILIES.index(name)


def _geometry(oracle):
    """f64 (gx, gy, cx, cy, cz, L) of the scene's records as the oracle projects them."""
    t = tight_scene(oracle, NAME)
    return cached(("tight_geometry", NAME), lambda: tight_geometry(tight_ref(oracle, NAME, 8)["gdata"], t["W"], t["H"]))


def _landed(oracle):
    """Per splat whose opacity was landed on a block: (splat, block x, block y, qmin of the block's pixels in f64, v = (ln(255 op) -
    qmin) / max(1, qmin): v >= 0 <=> the block holds a pixel with alpha >= 1/255 in exact arithmetic)."""
    def make():
        t = tight_scene(oracle, NAME)
        gx, gy, cx, cy, cz, L = _geometry(oracle)
        idx = np.nonzero(t["block"][:, 0] >= 0)[0]
        qm = block_qmin_pixels(gx[idx], gy[idx], cx[idx], cy[idx], cz[idx], t["W"], t["H"])
        bx, by = t["block"][idx, 0], t["block"][idx, 1]
        q = qm[np.arange(idx.size), by, bx]
        return idx, bx, by, q, (L[idx] - q) / np.maximum(1.0, q)
    return cached(("tight_landed", NAME), make)


def _both_sides(v, d):
    return int(((v < 0) & (v >= -d)).sum()), int(((v >= 0) & (v <= d)).sum())


def _ref_masks(oracle, ts):
    ref = tight_ref(oracle, NAME, ts)
    t = tight_scene(oracle, NAME)
    return cached(("tight_masks", NAME, ts), lambda: oracle.instance_masks(ref["gdata"], ref["sorted_keys"], ref["sorted_values"], t["W"], t["H"], ts))


def _passing_pixels_f32(oracle, g, tx, ty, ts):
    """How many in-canvas pixels of tile (tx, ty) pass `power <= 0 && alpha >= 1/255` for record g, in f32 with the oracle's
    expression tree (gs_oracle.c gso_instance_masks; the same restatement as test_blend_culls.replay_blocks)."""
    from oracle import np_oracle as npo
    t = tight_scene(oracle, NAME)
    W, H = t["W"], t["H"]
    rec = gdata_f32(tight_ref(oracle, NAME, 8)["gdata"])[g]
    ly, lx = np.meshgrid(np.arange(ts), np.arange(ts), indexing="ij")
    px, py = (tx * ts + lx).ravel(), (ty * ts + ly).ravel()
    inside = (px < W) & (py < H)
    with np.errstate(all="ignore"):
        dx = rec[0] * F(W) - px.astype(F)
        dy = rec[1] * F(H) - py.astype(F)
        power = F(-0.5) * (rec[4] * dx * dx + rec[6] * dy * dy) - rec[5] * dx * dy
        alpha = npo.wmin(F(0.99), rec[11] * npo.expf(power))
    return int((inside & (power <= 0) & (alpha >= C255)).sum())


def tight_mode_f32(g, W, H):
    """tight_setup's mode decision restated in numpy f32 (for counting the modes of a family only): 0 = opacity below 1/255, 2 =
    the reference's whole rect (cx cz - cy^2 lost to cancellation, or a conic that is not positive definite), 1 = the ellipse."""
    cx, cy, cz, op = g[:, 4], g[:, 5], g[:, 6], g[:, 11]
    with np.errstate(all="ignore"):
        cxz, cyy = cx * cz, cy * cy
        D = cxz - cyy
        Dlo = D - F(1.1e-5) * (cxz + cyy) - F(4.0e-7) * (cxz + cyy)
        lim = np.log(op.astype(np.float64) * 255.0) + 0.01
    pd = (cx > 0) & (cz > 0) & (D > 0)
    return np.where(lim < 0, 0, np.where(pd & (Dlo > F(0.25) * D), 1, 2))


# minimum counts: about three quarters of what the seeded construction delivers (profiles/tight_margins.txt has the delivered figures)
NEED = {("contour", 1e-2): 190, ("contour", 1e-3): 150, ("contour", 1e-4): 110, ("contour", 1e-5): 70,
        ("cancellation", 1e-4): 130, ("cancellation", 1e-5): 100, ("alias", 1e-2): 22, "partial_blocks": 75, "f32_disagrees": 130,
        ("single_bit", 16): 3900, ("single_bit", 32): 1100, ("single_pixel", 8): 310, ("single_pixel", 16): 200, ("single_pixel", 32): 120,
        "far_instances": 3200, "far_splats": 78, "mode1": 315, "mode2": 78, "mode0": 28, "floor_mode1": 46, "floor_inside_margin": 14,
        ("extreme_x", 0.3): 47, ("extreme_x", 1e-2): 16, ("extreme_y", 0.3): 30, ("extreme_y", 1e-2): 9,
        ("alias_nonzero", 8): 165, ("alias_zero", 8): 6300, ("alias_nonzero", 16): 130, ("alias_zero", 16): 3000,
        ("alias_nonzero", 32): 95, ("alias_zero", 32): 1250}


# ---- the scene reaches its margins (oracle only: CPU suite) ---------------------------------------------------------------------------
def test_tight_scene_places_what_it_draws(oracle):
    t = tight_scene(oracle, NAME)
    assert t["W"] <= 512 and t["H"] <= 128 and t["splats"].shape[0] <= 1500
    assert t["W"] % 32 and t["H"] % 32 and t["W"] % 8 and t["H"] % 8  # partial tiles and partial blocks at the right and bottom edges
    for name, (drawn, kept) in t["drawn"].items():
        assert kept >= 0.9 * drawn, (name, drawn, kept)
    assert (tight_ref(oracle, NAME, 8)["tile_counts"] > 0).all()  # none culled: the geometry below is every record's


def test_tight_scene_contour_reaches_both_sides(oracle):
    t = tight_scene(oracle, NAME)
    gx, gy = _geometry(oracle)[:2]
    idx, bx, by, q, v = _landed(oracle)
    assert ((q > 0.2) & (q < 5.5)).all()
    fam = t["family"][idx]
    for name, needs in (("contour", ((1e-2, NEED["contour", 1e-2]), (1e-3, NEED["contour", 1e-3]), (1e-4, NEED["contour", 1e-4]), (1e-5, NEED["contour", 1e-5]))),
                        ("cancellation", ((1e-4, NEED["cancellation", 1e-4]), (1e-5, NEED["cancellation", 1e-5]))),
                        ("alias", ((1e-2, NEED["alias", 1e-2]),))):
        f = fam == TIGHT_FAMILIES.index(name)
        for d, need in needs:
            below, above = _both_sides(v[f], d)
            assert below >= need and above >= need, (name, d, below, above)
    # half of the contour family's blocks are their tile's corner block on the side facing the centre (at 32, so at 16 too) ...
    f = fam == TIGHT_FAMILIES.index("contour")
    corner = facing_corner(gx[idx], gy[idx], t["W"], t["H"])[np.arange(idx.size), by, bx]
    assert corner[f].mean() >= 0.5, corner[f].mean()
    # ... and partial blocks at the right and bottom edges are among the targets
    assert ((bx == t["W"] // 8) | (by == t["H"] // 8)).sum() >= NEED["partial_blocks"]
    # the oracle's f32 decision on the target block follows the exact one where the margin is wide, and need not where it is within
    # the rounding of `power` (which is what the +0.01 is for)
    m = oracle.instance_masks(tight_ref(oracle, NAME, 8)["gdata"], ((by * -(-t["W"] // 8) + bx) * 1000).astype(np.uint32), idx.astype(np.uint32),
                              t["W"], t["H"], 8)
    wide = np.abs(v) > 1e-3
    assert ((m[wide] != 0) == (v[wide] >= 0)).all()
    assert ((m != 0) != (v >= 0)).sum() >= NEED["f32_disagrees"]


def test_tight_scene_has_hanging_tiles(oracle):
    t = tight_scene(oracle, NAME)
    for ts in (16, 32):  # reference instances whose exact mask has a single bit: one 8x8 block decides the instance
        m = _ref_masks(oracle, ts)
        single = (m != 0) & ((m & (m - 1)) == 0)
        assert single.sum() >= NEED["single_bit", ts], (ts, int(single.sum()))
    idx, bx, by, q, v = _landed(oracle)
    near = np.nonzero(np.abs(v) <= 1e-3)[0]
    for ts in (8, 16, 32):  # ... and tiles in which a single pixel passes (f32, the oracle's expression)
        n1 = sum(_passing_pixels_f32(oracle, idx[k], 8 * bx[k] // ts, 8 * by[k] // ts, ts) == 1 for k in near)
        assert n1 >= NEED["single_pixel", ts], (ts, n1)


def test_tight_scene_reaches_far(oracle):
    """Contributing pixels more than 256 px from their splat's centre, where the terms of q reach 1e5 and the f32 rounding of
    `power` is no longer small against 0.01."""
    t = tight_scene(oracle, NAME)
    ref, m = tight_ref(oracle, NAME, 8), _ref_masks(oracle, 8)
    gx, gy = _geometry(oracle)[:2]
    ntx = -(-t["W"] // 8)
    tile = (ref["sorted_keys"] // 1000).astype(np.int64)
    g = ref["sorted_values"]
    tx, ty = tile % ntx, tile // ntx
    dx = np.maximum(np.maximum(8.0 * tx - gx[g], gx[g] - (8.0 * tx + 7.0)), 0.0)  # distance from the centre to the tile's nearest pixel
    dy = np.maximum(np.maximum(8.0 * ty - gy[g], gy[g] - (8.0 * ty + 7.0)), 0.0)
    far = (m != 0) & (np.hypot(dx, dy) > 256.0)
    assert far.sum() >= NEED["far_instances"], int(far.sum())
    assert np.unique(g[far]).size >= NEED["far_splats"]


def test_tight_scene_switches_modes(oracle):
    t = tight_scene(oracle, NAME)
    mode = tight_mode_f32(gdata_f32(tight_ref(oracle, NAME, 8)["gdata"]), t["W"], t["H"])
    c = mode[_fam(t, "cancellation")]
    assert (c == 1).sum() >= NEED["mode1"] and (c == 2).sum() >= NEED["mode2"], np.bincount(c)
    o = mode[_fam(t, "opacity_floor")]
    L = _geometry(oracle)[5][_fam(t, "opacity_floor")]
    assert (np.abs(L) <= 0.021).all()
    assert (o == 0).sum() >= NEED["mode0"] and (o == 1).sum() >= NEED["floor_mode1"], np.bincount(o)
    assert ((L < 0) & (L > -0.01)).sum() >= NEED["floor_inside_margin"]  # alpha < 1/255 everywhere, but kept by the +0.01


def test_tight_scene_extreme_points_on_boundaries(oracle):
    """The f64 extreme points of E = {q <= ln(255 op)} lie within 0.3 px (and, for a part, within 1e-2 px) of a strip boundary row /
    of the first or last pixel row of a tile, on both sides of it."""
    t = tight_scene(oracle, NAME)
    gx, gy, cx, cy, cz, L = _geometry(oracle)
    D = cx * cz - cy * cy
    for name in ("extreme_x", "extreme_y"):
        f = _fam(t, name)
        with np.errstate(invalid="ignore"):  # (other families hold opacities below 1/255)
            ey = (np.sqrt(2.0 * L * cz / D) * -cy / cz if name == "extreme_x" else np.sqrt(2.0 * L * cx / D))[f]
        best = np.full(int(f.sum()), np.inf)
        for sg in (-1.0, 1.0):  # either extreme point: the row nearest to it among the boundary rows
            y = gy[f] - sg * ey
            r = np.round(y / 8.0) * 8.0
            cand = [r] if name == "extreme_x" else [r, r - 1.0]
            for c in cand:
                d = y - c
                best = np.where(np.abs(d) < np.abs(best), d, best)
        assert (np.abs(best) <= 0.3001).all(), (name, np.abs(best).max())
        for d, need in ((0.3, NEED[name, 0.3]), (1e-2, NEED[name, 1e-2])):
            below, above = _both_sides(best, d)
            assert below >= need and above >= need, (name, d, below, above)


def test_tight_scene_has_aliased_instances(oracle):
    """Aliased reference instances (rect column ntx of row ty = tile (ty + 1, 0)) with non-zero and with zero exact masks."""
    t = tight_scene(oracle, NAME)
    for ts in TILES:
        ref = tight_ref(oracle, NAME, ts)
        ntx, nty = oracle.num_tiles(t["W"], t["H"], ts)
        gd = ref["gdata"]
        al = np.nonzero(gd[:, 14] == ntx + 1)[0]
        assert (t["family"][al] == TIGHT_FAMILIES.index("alias")).sum() >= 80
        g = np.concatenate([np.full(int(gd[i, 15] - gd[i, 13]), i) for i in al])
        row = np.concatenate([np.arange(gd[i, 13], gd[i, 15]) for i in al])
        m = oracle.instance_masks(gd, ((row + 1) * ntx * 1000).astype(np.uint32), g.astype(np.uint32), t["W"], t["H"], ts)
        inside = row + 1 < nty
        assert (m[inside] != 0).sum() >= NEED["alias_nonzero", ts] and (m[inside] == 0).sum() >= NEED["alias_zero", ts], (
            ts, int((m[inside] != 0).sum()), int((m[inside] == 0).sum()))
        assert (~inside).sum() >= 80 and not m[~inside].any()  # the aliased instance of the last row names a tile past the grid




# ---- the kernels on the same scene (GPU) ------------------------------------------------------------------------------------------------
def _frame(r, u):
    from gsplat import _abi
    r.render_uniforms(u)
    r.wait()
    return {"keys": r.read_buffer(_abi.GS_BUF_KEYS), "values": r.read_buffer(_abi.GS_BUF_VALUES), "masks": r.read_buffer(_abi.GS_BUF_BLOCK_MASKS),
            "rgbf": r.read_buffer(_abi.GS_BUF_RGB_F32, np.float32).copy(), "rgba8": r.read_rgba8(), "stats": r.stats()}


def _same_image(a, b, cell):
    np.testing.assert_array_equal(a["rgbf"].view(np.uint32), b["rgbf"].view(np.uint32), err_msg=str(cell))
    np.testing.assert_array_equal(a["rgba8"], b["rgba8"], err_msg=str(cell))


@pytest.mark.gpu
@pytest.mark.parametrize("slab", [False, True], ids=["canvas", "slab"])
@pytest.mark.parametrize("ts", TILES)
def test_tight_kernels_at_their_margins(oracle, ts, slab):
    """EXACT: the tight frame's lists are an ordered subset of the oracle's whose dropped instances have all-zero masks, the block
    masks cover the contributing blocks, the image equals the oracle's bit for bit, and the tight path really ran; with
    GS_OPT_TILE_CULL 0 the lists are the oracle's and the image is the tight frame's.  Fused: the tight frame equals the rect frame
    byte for byte (the fused-versus-oracle envelope of thin far-reaching splats is not this test's subject)."""
    from gsplat import _abi
    from gpu_checks import check_stages
    t = tight_scene(oracle, NAME)
    s, u, W, H = t["splats"], t["uniforms"], t["W"], t["H"]
    cols = SLAB_COLS[ts] if slab else None
    ref = tight_ref(oracle, NAME, ts, cols)
    for exact in (True, False):
        r = mk(s, W, H, ts, exact=exact, cols=cols)
        cell = (ts, cols, exact)
        r.set_option(_abi.GS_OPT_TILE_CULL, 1)
        tight = _frame(r, u)
        assert tight["stats"]["tight_binning"] == 1, cell
        assert 0 < tight["stats"]["num_intersections"] < ref["num_intersections"], cell
        print("instances", cell, "tight", tight["stats"]["num_intersections"], "reference", ref["num_intersections"])
        if exact:
            check_stages(r, ref, exact_image=True, debug=False, oracle=oracle, W=W, H=H)
        r.set_option(_abi.GS_OPT_TILE_CULL, 0)
        rect = _frame(r, u)
        assert rect["stats"]["tight_binning"] == 0, cell
        if exact:
            check_stages(r, ref, exact_image=True, debug=False, oracle=oracle, W=W, H=H)  # the lists equal the oracle's
        _same_image(tight, rect, cell)
        r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("ts", TILES)
def test_slab_instances_are_the_whole_canvas(oracle, ts):
    """gs_tight.h: "whole-canvas and slab frames agree instance for instance".  The whole canvas's (key, value, block mask) list
    restricted to the slab's tile columns (an aliased instance carries the key of tile (ty + 1, 0): it belongs to the owner of
    column 0, as with the oracle's cols=) is the slab's list."""
    t = tight_scene(oracle, NAME)
    s, u, W, H = t["splats"], t["uniforms"], t["W"], t["H"]
    ntx = oracle.num_tiles(W, H, ts)[0]
    c0, c1 = SLAB_COLS[ts]
    frames = []
    for cols in (None, (c0, c1)):
        r = mk(s, W, H, ts, exact=True, cols=cols)
        frames.append(_frame(r, u))
        assert frames[-1]["stats"]["tight_binning"] == 1
        r.destroy()
    whole, part = frames
    col = (whole["keys"] // 1000) % ntx
    own = (col >= c0) & (col < c1)
    assert 0 < own.sum() < own.size
    for k in ("keys", "values", "masks"):
        np.testing.assert_array_equal(whole[k][own], part[k], err_msg=k)


@pytest.mark.gpu
def test_splat_state_context_bins_the_same(oracle):
    """The GS_FLAG_SPLAT_STATE instantiation of the projection with an all-zero plane: the same lists as the unflagged context's."""
    t = tight_scene(oracle, NAME)
    s, u, W, H = t["splats"], t["uniforms"], t["W"], t["H"]
    frames = []
    for state in (False, True):
        r = mk(s, W, H, 16, exact=True, state=state)
        if state:
            r.write_state(np.zeros(s.shape[0], np.uint8))
        frames.append(_frame(r, u))
        assert frames[-1]["stats"]["tight_binning"] == 1
        r.destroy()
    for k in ("keys", "values", "masks"):
        np.testing.assert_array_equal(frames[0][k], frames[1][k], err_msg=k)
    _same_image(frames[0], frames[1], "state")
