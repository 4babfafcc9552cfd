"""The blend's two parking culls at their margins, in every blend kernel.

An entry is parked (evaluated for a block's pixels) only if (1) its alpha >= 1/255 ellipse reaches the bounding box of the block's
LIVE pixels (`block_qmin` against ln(255 op) + 0.01, with 1e-5 of the terms' magnitude on q) and (2) Tmax (1 - alpha_lo) over
that box is not below 0.0000999 (alpha_lo = 0.99 min(0.99, op exp(-qmax))).  Both are meant to skip only work that cannot change a
pixel.  The scenes (tests/support.py) are built in pixel space (identity view and projection, focal W/2, H/2, centres in pixels, one depth
bucket so that the list order is the splat order) and aim at the margins of the two decisions:

  * transmittance_edge_scene: T brought to just above the final threshold (1.0039e-4) by huge, near-uniform splats, then a sweep
    of entries whose T (1 - alpha) lands at 1e-4 (1 +- delta), and entries at the 0.99 clamp;
  * live_box_scene: most pixels of a block finished, one corner / one row / one column / two opposite corners left live, then
    thin (eigenvalue ratio >= 1e3), rotated splats whose alpha = 1/255 contour passes just inside or just outside the live box;
  * degenerate_conic_scene: extreme scales and anisotropy at 45 degrees (conics that are not positive definite in f32, tiny cx or
    cz).

Every scene PROVES that it reaches its margins (unmarked tests, they run in the CPU suite): `replay_blocks` replays the oracle's
EXACT blend per 8x8 block in f32 and records, per (block, entry), the live set, its box, Tmax, the f64 minimum of q over the box
against ln(255 op) and Tmax (1 - alpha_min).  The GPU tests then render each scene with the culls on and off
(GS_OPT_BLEND_ABLATION bit 2) in every blend kernel, binning and mode, against each other and against the oracle.
"""
import numpy as np
import pytest

from support import F, SCENES, SLAB_COLS, box_qmin_f64, gdata_f32, margin_ref, margin_scene

C255 = np.float32(1.0 / 255.0)


# ---- the replay --------------------------------------------------------------------------------------------------------------
def replay_blocks(ref, W, H, ts, cols=None):
    """Replays the oracle's EXACT blend (gs_oracle.c gso_blend, the kernels' EXACT expression tree) per tile in f32 and returns,
    per (8x8 block, list entry) whose block still has a live pixel before the entry, one row of:
      block, entry, nlive, Tmax, m_box = qmin(live box) - ln(255 op)  (f64; <= 0: the entry reaches alpha >= 1/255 in the box),
      m_pix = min over the live PIXELS of q - ln(255 op), r_T = Tmax (1 - alpha_min) / 1e-4 - 1 (f64, alpha over the live box),
      pd (the kernels' f32 positive-definiteness test), min(cx, cz), box area / live pixels.
    Also returns the replayed f32 image (it must equal the oracle's bit for bit) and the per-pixel T before each entry is not
    kept.  The per-entry live set is tighter than the kernels' per-batch one."""
    from oracle import np_oracle as npo
    ntx = int(np.ceil(F(W) / F(ts)))
    nty = int(np.ceil(F(H) / F(ts)))
    c0, c1 = cols if cols is not None else (0, ntx)
    g = gdata_f32(ref["gdata"])
    vals, rng = ref["sorted_values"], ref["ranges"]
    img = np.zeros((H, W, 3), np.float32)
    rows = []
    fin = F(1.0) - C255
    for ty in range(nty):
        for tx in range(c0, c1):
            tile = tx + ty * ntx
            start = int(rng[tile - 1]) if tile > 0 else 0
            end = int(rng[tile])
            ly, lx = np.meshgrid(np.arange(ts), np.arange(ts), indexing="ij")
            gx, gy = (tx * ts + lx).ravel(), (ty * ts + ly).ravel()
            inside = (gx < W) & (gy < H)
            blk = ((ly // 8) * (ts // 8) + lx // 8).ravel()
            pxf, pyf = gx.astype(F), gy.astype(F)
            T = np.ones(gx.size, F)
            acc = np.zeros((gx.size, 3), F)
            if end > start:
                rec = g[vals[start:end]]
                gxp = rec[:, 0] * F(W)
                gyp = rec[:, 1] * F(H)
                cx, cy, cz = rec[:, 4], rec[:, 5], rec[:, 6]
                op = rec[:, 11]
                with np.errstate(all="ignore"):
                    dx = gxp[:, None] - pxf[None, :]
                    dy = gyp[:, None] - pyf[None, :]
                    t1 = cx[:, None] * dx * dx
                    t2 = cz[:, None] * dy * dy
                    t3 = cy[:, None] * dx * dy
                    power = F(-0.5) * (t1 + t2) - t3
                    alpha = npo.wmin(F(0.99), op[:, None] * npo.expf(power))
                    pd = (cx > 0) & (cz > 0) & (cx * cz - cy * cy > 0)
                    lim0 = np.log(255.0 * op.astype(np.float64))
                    qpix = -power.astype(np.float64)
                for e in range(end - start):
                    live = inside & ~(T * fin < F(0.0001))
                    with np.errstate(all="ignore"):
                        for b in np.unique(blk[live]):
                            lb = live & (blk == b)
                            bx = gx[lb].astype(np.float64)
                            by = gy[lb].astype(np.float64)
                            x0, x1, y0, y1 = bx.min(), bx.max(), by.min(), by.max()
                            Tm = float(T[lb].max())
                            cxd, cyd, czd = float(cx[e]), float(cy[e]), float(cz[e])
                            ex, ey = float(gxp[e]), float(gyp[e])
                            if pd[e] and np.isfinite([cxd, cyd, czd, ex, ey]).all():
                                mb = box_qmin_f64(cxd, cyd, czd, ex - x1, ex - x0, ey - y1, ey - y0) - lim0[e]
                                cs = [(ex - a) for a in (x0, x1)], [(ey - a) for a in (y0, y1)]
                                qmax = max(0.5 * (cxd * a * a + czd * c * c) + cyd * a * c for a in cs[0] for c in cs[1])
                                amin = min(0.99, float(op[e]) * np.exp(-qmax))
                                rT = Tm * (1.0 - amin) / 1e-4 - 1.0
                            else:
                                mb, rT = np.nan, np.nan
                            mp = float((qpix[e, lb] - lim0[e]).min()) if pd[e] else np.nan
                            area = (x1 - x0 + 1) * (y1 - y0 + 1) / lb.sum()
                            rows.append((tile * 64 + b, start + e, int(lb.sum()), Tm, mb, mp, rT, bool(pd[e]),
                                         float(min(cxd, czd)), area))
                    a = alpha[e]
                    test = T * (F(1.0) - a)
                    cond = ((power[e] <= 0) & (a >= C255) & (test >= F(0.0001))).astype(F)
                    for ch in range(3):
                        acc[:, ch] = acc[:, ch] + cond * rec[e, 8 + ch] * a * T
                    T = cond * test + (F(1.0) - cond) * T
            img[gy[inside], gx[inside]] = acc[inside]
    dt = np.dtype([("block", np.int64), ("entry", np.int64), ("nlive", np.int64), ("Tmax", np.float64), ("m_box", np.float64),
                   ("m_pix", np.float64), ("r_T", np.float64), ("pd", bool), ("cmin", np.float64), ("sparse", np.float64)])
    return np.array(rows, dtype=dt), img


_CACHE = {}


def _replay(oracle, name):
    key = (name, "replay")
    if key not in _CACHE:
        s, u, W, H = margin_scene(oracle, name)
        ref = margin_ref(oracle, name, 8)
        rows, img = replay_blocks(ref, W, H, 8)
        np.testing.assert_array_equal(img.view(np.uint32), ref["rgbf"].view(np.uint32))  # the replay IS the oracle's blend
        _CACHE[key] = rows
    return _CACHE[key]


def _both_sides(v, d):
    """(pairs with v in [-d, 0), pairs with v in [0, d])"""
    return int(((v < 0) & (v >= -d)).sum()), int(((v >= 0) & (v <= d)).sum())


# ---- the scenes reach their margins (oracle only: CPU suite) ------------------------------------------------------------------
def test_transmittance_edge_scene_reaches_its_margins(oracle):
    rows = _replay(oracle, "transmittance_edge")
    rT = rows["r_T"]
    # the kernels cull when Tmax (1 - 0.99 alpha_lo) < 0.999e-4: entries at 1e-4 (1 +- delta) for every delta down to 3e-4,
    # on both sides of the exact decision T (1 - alpha) >= 1e-4
    for d, need in ((3e-2, 500), (3e-3, 300), (1e-3, 150), (3e-4, 60)):
        below, above = _both_sides(rT, d)
        assert below >= need and above >= need, (d, below, above)
    # Tmax is not most pixels' own T: most (block, entry) pairs have several live pixels
    assert (rows["nlive"] > 1).sum() > 0.5 * rows.size
    # the 0.99 clamp: entries with alpha 0.99 over blocks that are still live
    g = gdata_f32(margin_ref(oracle, "transmittance_edge", 8)["gdata"])
    ent = margin_ref(oracle, "transmittance_edge", 8)["sorted_values"][rows["entry"]]
    assert (g[ent, 11] >= 0.99).sum() >= 100


def test_live_box_scene_reaches_its_margins(oracle):
    rows = _replay(oracle, "live_box")
    mb, mp = rows["m_box"], rows["m_pix"]
    # min over the live box of q against ln(255 op): just inside (must park) and just outside (may skip) the alpha = 1/255 contour
    for d, need in ((1e-2, 150), (3e-3, 100), (1e-3, 60), (3e-4, 15)):
        below, above = _both_sides(mb, d)
        assert below >= need and above >= need, (d, below, above)
    # ... with the contour's inside on a live PIXEL (an entry there with alpha in [1/255, 1.01/255): a cull that drops it changes a bit)
    assert _both_sides(mp, 1e-2)[0] >= 100 and _both_sides(mp, 1e-3)[0] >= 40
    # every live set: one pixel, a row or column, two opposite corners (the box much larger than the live set), partial blocks
    near = np.abs(mb) <= 1e-2
    assert (near & (rows["nlive"] == 1)).sum() >= 30
    assert (near & (rows["nlive"] >= 3) & (rows["sparse"] == 1.0)).sum() >= 30
    assert (near & (rows["nlive"] == 2) & (rows["sparse"] >= 4.0)).sum() >= 10
    s, u, W, H = margin_scene(oracle, "live_box")
    ntx = int(np.ceil(W / 8))
    blk = rows["block"] // 64
    edge = ((blk % ntx) == ntx - 1) | ((blk // ntx) == int(np.ceil(H / 8)) - 1)
    assert (near & edge).sum() >= 10
    # the opacities just above 1/255, where lim = ln(255 op) is near 0
    g = gdata_f32(margin_ref(oracle, "live_box", 8)["gdata"])
    op = g[margin_ref(oracle, "live_box", 8)["sorted_values"][rows["entry"]], 11]
    assert (near & (op < 0.0045)).sum() >= 20


def test_degenerate_conic_scene_reaches_its_margins(oracle):
    rows = _replay(oracle, "degenerate_conic")
    ref = margin_ref(oracle, "degenerate_conic", 8)
    g = gdata_f32(ref["gdata"])
    fin = np.isfinite(g[:, :12]).all(axis=1)
    ent = ref["sorted_values"][rows["entry"]]
    # valid (finite) records whose conic fails the kernels' f32 test cx cz - cy^2 > 0 (an indefinite conic: a covariance
    # determinant that cancelled to a negative number), reaching live blocks: such an entry must be kept
    assert (~rows["pd"] & fin[ent]).sum() >= 20
    # tiny cx or cz (rcp huge in block_qmin) on live blocks
    assert (rows["pd"] & (rows["cmin"] < 1e-6)).sum() >= 500


# ---- the matrix (GPU) ---------------------------------------------------------------------------------------------------------
KERNELS = [(16, 0), (32, 0), (16, 8), (32, 8), (8, 0)]  # (tile, GS_OPT_BLEND_ABLATION): the quad kernel at 16 / 32, the workgroup-
                                                          # per-tile kernel at 16 / 32, gs_blend_kernel<8>


def _frame(r, u, debug=False):
    from gsplat import _abi
    r.render_uniforms(u, debug=debug)
    r.wait()
    return (r.read_buffer(_abi.GS_BUF_RGB_F32, np.float32).copy(), r.read_rgba8(), r.stats())


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS, ids=["quad16", "quad32", "wg16", "wg32", "tile8"])
@pytest.mark.parametrize("name", list(SCENES))
def test_blend_culls_at_their_margins(oracle, name, kernel):
    """Every blend kernel, both binnings (gs_render tight = MASKED walkers; GS_OPT_TILE_CULL 0 and gs_render_debug = the reference's
    lists), EXACT and fused, the whole canvas and one tile-column slab: the frame with the culls (ablation bit 2 clear) equals the
    frame without them bit for bit, EXACT frames equal the oracle (lists included), fused frames are within the fused bounds, and
    the culls removed work."""
    from gsplat import _abi
    from gpu_checks import check_image, check_stages, make_renderer
    ts, abl = kernel
    s, u, W, H = margin_scene(oracle, name)
    for cols in (None, SLAB_COLS[ts]):
        ref = margin_ref(oracle, name, ts, cols)
        for flags, exact in ((_abi.GS_FLAG_EXACT_BLEND, True), (0, False)):
            r = make_renderer(s, W, H, ts, flags=flags, cols=cols)
            ev_on = ev_off = 0
            for tight, debug in ((1, False), (0, False), (0, True)):
                r.set_option(_abi.GS_OPT_TILE_CULL, tight)
                r.set_option(_abi.GS_OPT_BLEND_ABLATION, abl | 4)
                f_off, i_off, st_off = _frame(r, u, debug)
                r.set_option(_abi.GS_OPT_BLEND_ABLATION, abl)
                f_on, i_on, st_on = _frame(r, u, debug)
                cell = (name, ts, abl, cols, exact, tight, debug)
                assert st_on["tight_binning"] == (tight and not debug), cell
                np.testing.assert_array_equal(f_on.view(np.uint32), f_off.view(np.uint32), err_msg=str(cell))
                np.testing.assert_array_equal(i_on, i_off, err_msg=str(cell))
                if exact:  # every tap of a debug frame, the (subset) lists of a product frame, the image bit for bit
                    check_stages(r, ref, exact_image=True, debug=debug, oracle=oracle, W=W, H=H)
                else:  # these scenes put many decisions within rounding of their thresholds on purpose: flagged pixels abound
                    check_image(r, ref, False, max_ill=0.5)
                assert st_on["num_evaluated"] <= st_off["num_evaluated"], (cell, st_on["num_evaluated"], st_off["num_evaluated"])
                ev_on += st_on["num_evaluated"]
                ev_off += st_off["num_evaluated"]
            assert ev_on < ev_off, (name, ts, abl, cols, exact, ev_on, ev_off)  # the switch and the culls exist in this kernel
            r.destroy()
