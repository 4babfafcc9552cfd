"""The slab reach cull (csrc/k_preprocess.hip, in_frustum_slab) at its margins and under non-rigid view matrices.

A tile-column slab context (cols=(c0, c1), the multi-GPU partition) drops most gaussians in phase 1 of the projection, before
their records are read, by a closed-form bound of their screen radius.  A gaussian the bound drops is gone for the frame: the
exact slab test never sees it.  The bound rests on lambda_max(cov2d) <= |J|_F^2 |W|_2^2 s_max^2 with W the view's 3x3, and the
C ABI takes whatever view matrix the host wrote: scaled, sheared, anisotropic.  The cases:

  * non-rigid views: view' = [A 0; 0 1] view of an orbit camera (slab_restate.apply_view), A a uniform scale k in {0.25, 3, 8},
    diag(5, 1, 1), diag(1, 1, 6), a shear (depth gains 4 x) and the rigid control, at three canvases (tile 16; tile 8 ragged, the
    alias column past the canvas; tile 32), scale modifier 1 and 3, over two partitions of the canvas whose slabs are column 0
    alone, the last column alone, one middle column, one wider than 75 %, one of 30 .. 75 % and one under 30 % of the canvas: the
    widths at which gs_preprocess_prepare picks each cull-chunk instantiation (1, 4, 8 for reference binning; 2, 4, 8 for tight);
    and a finite view scaled by 2^65, whose squared norm overflows f32: an infinite or NaN reach must keep the gaussian;
  * rigid margins: thin long splats whose centres lie 0 .. 1.2 oracle radii outside every slab edge, a third of them tilted out
    of the image plane, under a pinhole whose tan_fov uniforms are half the projection's, so that the 1.3 tan_fov clamp of the
    Jacobian is active on the outer parts of the canvas.

The unmarked tests PROVE with the oracle's slab tile counts and the restated bound (tests/slab_restate.py) that the inputs are
adversarial: a bound that took the view for rigid would drop splats the oracle gives to a slab, and the margin scene has splats
on both sides of every slab edge's reach.  The minimum counts are conditions on the seeded scenes, not measurements of the code
under test.  The GPU tests compare every slab with oracle.render(cols=): a debug frame tap by tap (the per-gaussian tile counts
included), a product frame as a harmless subset with a bit-equal image, and the concatenated slabs with the whole-canvas frame.
"""
import numpy as np
import pytest

import slab_restate as sl
from support import F, cached, mk

STEP = 21
N = 6000
SHAPES = [(256, 128, 16), (200, 120, 8), (320, 192, 32)]  # (W, H, tile size)
SHAPE_IDS = ["256x128t16", "200x120t8", "320x192t32"]
# two partitions of the canvas per tile size.  The first: column 0 alone, a slab wider than 75 %, the last column alone; the
# second: a slab of 30 .. 75 %, one middle column, a slab under 30 %, the rest
PARTITIONS = {16: ([(0, 1), (1, 15), (15, 16)], [(0, 5), (5, 6), (6, 9), (9, 16)]),
              8: ([(0, 1), (1, 24), (24, 25)], [(0, 8), (8, 9), (9, 14), (14, 25)]),
              32: ([(0, 1), (1, 9), (9, 10)], [(0, 4), (4, 5), (5, 7), (7, 10)])}
VIEWS = {"rigid": None, "k0.25": sl.uniform_scale(0.25), "k3": sl.uniform_scale(3.0), "k8": sl.uniform_scale(8.0),
         "diag511": np.diag([5.0, 1.0, 1.0]), "diag116": np.diag([1.0, 1.0, 6.0]), "shear": sl.shear_z_by_x(4.0)}
# a finite view whose squared norm, 2^130, is no f32: the factor arrives as +inf (and the reach as inf or NaN), which must KEEP
HUGE_VIEW = sl.uniform_scale(2.0 ** 65)
# (splat, slab) pairs the oracle gives a tile to while a bound with the rigid factor 1 drops them, at least, per canvas and at scale
# modifier 1 (the seeded scenes deliver 22 .. 232 for k = 8, diag(5, 1, 1) and the shear, 1 .. 6 for k = 3: profiles/slab_reach.txt)
NEED_DROPPED = {"k8": 8, "diag511": 8, "shear": 8, "k3": 1}
NEED_EDGE = 16  # splats per slab edge and group of the rigid margin scene


def slabs_of(ts):
    a, b = PARTITIONS[ts]
    return a + b


def splats():
    from gsplat import synth
    return cached(("slab_reach_scene", N), lambda: synth.bicycle_like(N))


def uniforms(W, H, view, mod=1.0):
    from gpu_checks import orbit_uniforms
    u = orbit_uniforms(W, H, step=STEP)
    A = HUGE_VIEW if view == "k2^65" else VIEWS[view]
    if A is not None:
        u = sl.apply_view(u, A)
    return sl.with_scale_modifier(u, mod)


def slab_counts(oracle, key, s, u, W, H, ts, cols):
    return cached(("slab_counts", key, W, H, ts, cols), lambda: oracle.preprocess(s, u, W, H, ts, cols)[1])


def dropped_by_rigid_bound(oracle, W, H, ts, view, mod):
    """(pairs with a slab tile count above 0, of them dropped by the bound with factor 1, ... with the view's squared norm)."""
    s, u = splats(), uniforms(W, H, view, mod)
    ntx = oracle.num_tiles(W, H, ts)[0]
    w2 = sl.spectral_norm(u) ** 2
    live = lost1 = lostw = 0
    for cols in slabs_of(ts):
        has = slab_counts(oracle, (view, mod), s, u, W, H, ts, cols) > 0
        live += int(has.sum())
        lost1 += int((has & ~sl.keeps(s, u, W, ts, ntx, cols, 1.0)).sum())
        lostw += int((has & ~sl.keeps(s, u, W, ts, ntx, cols, w2)).sum())
    return live, lost1, lostw


# ---- the rigid margin scene ---------------------------------------------------------------------------------------------------------
def margin_uniforms(W, H):
    """Identity view, w = z, focal = half the canvas: pixel = (x / z + 1) W / 2.  The tan_fov words are HALF the projection's, so
    the Jacobian's clamp |t / z| <= 1.3 tan_fov = 0.65 is active on the outer 17.5 % of the canvas on either side."""
    u = np.zeros(40, F)
    u[0] = u[5] = u[10] = u[15] = 1.0
    u[16] = u[21] = u[26] = u[27] = 1.0
    u[35] = u[36] = 0.5
    u[37], u[38] = W / 2.0, H / 2.0
    u[39] = 1.0
    return u


def margin_scene(oracle, W, H, ts):
    """About 2 000 thin long splats (log-scales near ln 0.6, ln 0.002, ln 0.002), the long axis along screen x or up to 30 degrees
    off it, a third tilted up to 40 degrees out of the image plane (their radius then depends on where they stand: the Jacobian's
    third column, and its clamp).  For every boundary between two slabs of PARTITIONS[ts] and either side of it, centres at
    0 .. 1.2 oracle radii from the boundary: outside the slab on the other side, whose edge they test.  Returns (splats, uniforms,
    boundary column and side per splat)."""
    def make():
        rng = np.random.Generator(np.random.Philox(key=[4301, ts]))
        u = margin_uniforms(W, H)
        bounds = sorted({c for part in PARTITIONS[ts] for (c0, c1) in part for c in (c0, c1)} - {0, oracle.num_tiles(W, H, ts)[0]})
        per = 2000 // (2 * len(bounds))
        b = np.repeat(np.array(bounds, np.float64), 2 * per)
        side = np.tile(np.repeat([-1.0, 1.0], per), len(bounds))
        n = b.size
        s = np.zeros((n, 80), F)
        # depth sets the radius (3 sigma = 1.8 focal / z pixels for an untilted splat): 35 .. 95 px on a 256-pixel canvas, less
        # where the canvas (plus the 4 % a centre may lie outside it) leaves no room for 1.2 radii on that side of the boundary
        room = np.where(side < 0, b * ts + 0.04 * W, 1.04 * W - b * ts)
        z = 1.8 * (W / 2.0) / np.minimum(rng.uniform(35.0, 95.0, n) * W / 256.0, room / 1.25)
        s[:, 4:7] = np.log([0.6, 0.002, 0.002]) + rng.uniform(-0.05, 0.05, (n, 3))
        th = np.where(np.arange(n) % 2 == 0, 0.0, rng.uniform(-np.pi / 6, np.pi / 6, n))
        ph = np.where(np.arange(n) % 3 == 0, rng.uniform(-0.7, 0.7, n), 0.0)
        # q = qz(th) qy(ph), (r, x, y, z)
        s[:, 8] = np.cos(th / 2) * np.cos(ph / 2)
        s[:, 9] = -np.sin(th / 2) * np.sin(ph / 2)
        s[:, 10] = np.cos(th / 2) * np.sin(ph / 2)
        s[:, 11] = np.sin(th / 2) * np.cos(ph / 2)
        s[:, 12] = rng.uniform(-2.0, 3.0, n)
        s[:, 16:19] = rng.uniform(-1.5, 1.5, (n, 3))
        py = rng.uniform(0.1 * H, 0.9 * H, n)
        d = rng.uniform(0.0, 1.2, n)
        px = b * ts
        for _ in range(3):  # the radius of a tilted splat depends on where it stands: place, project, place again
            s[:, 0], s[:, 1], s[:, 2] = (2.0 * px / W - 1.0) * z, (2.0 * py / H - 1.0) * z, z
            r = sl.oracle_centre_radius(oracle.preprocess(s, u, W, H, ts)[0], W)[1]
            px = np.clip(b * ts + side * d * np.where(np.isnan(r), 0.0, r), -0.04 * W, 1.04 * W)
        return s, u, b.astype(np.int64), side
    return cached(("slab_margin_scene", W, H, ts), make)


def edge_groups(oracle, W, H, ts):
    """Per tested slab edge (slab, side of it): how many splats outside the slab on that side have a slab tile count above 0 with
    the centre more than 0.8 oracle radii from the edge, and how many have a count of 0 with the centre within 1.2 radii."""
    s, u, _, _ = margin_scene(oracle, W, H, ts)
    ntx = oracle.num_tiles(W, H, ts)[0]
    cx, r = sl.oracle_centre_radius(oracle.preprocess(s, u, W, H, ts)[0], W)
    out = {}
    for cols in slabs_of(ts):
        cnt = slab_counts(oracle, "margin", s, u, W, H, ts, cols)
        for side, edge in ((-1, cols[0]), (1, cols[1])):
            if edge in (0, ntx):
                continue
            with np.errstate(invalid="ignore"):
                dist = (cx - edge * ts) * side  # > 0: outside the slab, past this edge
                outside = dist > 0
                reach_far = outside & (cnt > 0) & (dist > 0.8 * r) & (dist < 1.2 * r)  # (not the far ones the alias column brings)
                miss_near = outside & (cnt == 0) & (dist < 1.2 * r)
            out[cols, side] = (int(reach_far.sum()), int(miss_near.sum()))
    return out


# ---- the inputs are adversarial (oracle and restatement only: CPU suite) -------------------------------------------------------------
def test_slab_widths_reach_every_cull_chunk_count():
    for W, H, ts in SHAPES:
        ntx = -(-W // ts)
        for part in PARTITIONS[ts]:
            assert part[0][0] == 0 and part[-1][1] == ntx and all(a[1] == b[0] for a, b in zip(part[:-1], part[1:]))
        slabs = slabs_of(ts)
        width = [(c1 - c0) / ntx for c0, c1 in slabs]
        assert (0, 1) in slabs and (ntx - 1, ntx) in slabs
        assert any(c1 - c0 == 1 and 0 < c0 and c1 < ntx for c0, c1 in slabs)
        assert any(w > 0.75 for w in width) and any(0.3 < w <= 0.75 for w in width) and any(w < 0.3 for w in width)
        assert {sl.cull_chunks(ntx, c, False) for c in slabs} == {1, 4, 8}
        assert {sl.cull_chunks(ntx, c, True) for c in slabs} == {2, 4, 8}


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_rigid_bound_would_drop_what_the_oracle_keeps(oracle, shape):
    """Under the non-rigid views the bound with factor 1 drops (splat, slab) pairs the oracle gives tiles to (so the GPU cases
    below fail on a kernel that assumes an orthonormal view), the bound with the view's squared spectral norm drops none, and
    under the rigid view the bound with factor 1 drops none."""
    W, H, ts = shape
    for view in VIEWS:
        for mod in (1.0, 3.0):
            live, lost1, lostw = dropped_by_rigid_bound(oracle, W, H, ts, view, mod)
            print("pairs", shape, view, "modifier", mod, "live", live, "dropped by factor 1:", lost1, "by |W|^2:", lostw)
            assert live >= 1000, (view, mod, live)
            assert lostw == 0, (view, mod, lostw)
            if view == "rigid":
                assert lost1 == 0, (mod, lost1)
            if mod == 1.0 and view in NEED_DROPPED:
                assert lost1 >= NEED_DROPPED[view], (view, lost1)


def test_an_overflowing_norm_is_a_live_case(oracle):
    W, H, ts = SHAPES[0]
    u = uniforms(W, H, "k2^65")
    assert np.isfinite(u).all()
    with np.errstate(over="ignore"):
        assert np.isinf(F(sl.spectral_norm(u) ** 2))
    live, lost1, lostw = dropped_by_rigid_bound(oracle, W, H, ts, "k2^65", 1.0)
    print("pairs k2^65 live", live, "dropped by factor 1:", lost1, "by inf:", lostw)
    assert live >= 1000 and lost1 >= 8 and lostw == 0


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_margin_scene_straddles_every_slab_edge(oracle, shape):
    W, H, ts = shape
    s, u, _, _ = margin_scene(oracle, W, H, ts)
    assert 1800 <= s.shape[0] <= 2000
    ntx = oracle.num_tiles(W, H, ts)[0]
    groups = edge_groups(oracle, W, H, ts)
    assert len(groups) == 2 * len(slabs_of(ts)) - 4  # every edge of every slab but the canvas's own
    for key, (reach_far, miss_near) in groups.items():
        print("edge", shape, key, "reaching from beyond 0.8 r:", reach_far, "missing within 1.2 r:", miss_near)
        assert reach_far >= NEED_EDGE and miss_near >= NEED_EDGE, (key, reach_far, miss_near)
    # the rigid bound keeps every splat a slab has tiles of
    for cols in slabs_of(ts):
        has = slab_counts(oracle, "margin", s, u, W, H, ts, cols) > 0
        assert not (has & ~sl.keeps(s, u, W, ts, ntx, cols, 1.0)).any(), cols
    # the clamp of the Jacobian is active for a part of the tilted splats
    tilted = s[:, 10] != 0
    assert (tilted & (np.abs(s[:, 0] / s[:, 2]) > 0.65)).sum() >= 100


# ---- the kernels (GPU) ----------------------------------------------------------------------------------------------------------------
def check_slabs(oracle, s, u, W, H, ts, partitions):
    """Every slab of every partition against oracle.render(cols=): a debug frame tap by tap, a product frame (tight binning) as a
    harmless subset with a bit-equal image; each partition's slabs side by side are the whole-canvas context's image."""
    from gpu_checks import check_stages
    whole = mk(s, W, H, ts, exact=True)
    whole.render_uniforms(u)
    whole.wait()
    img = whole.read_rgba8()
    whole.destroy()
    for part in partitions:
        parts = []
        for cols in part:
            ref = oracle.render(s, u, W, H, ts, cols=cols)
            r = mk(s, W, H, ts, exact=True, cols=cols)
            r.render_uniforms(u, debug=True)
            r.wait()
            check_stages(r, ref, exact_image=True)
            r.render_uniforms(u)
            r.wait()
            assert r.stats()["tight_binning"] == 1, cols
            check_stages(r, ref, exact_image=True, debug=False, oracle=oracle, W=W, H=H)
            parts.append(r.read_rgba8())
            r.destroy()
        np.testing.assert_array_equal(np.concatenate(parts, axis=1), img, err_msg=str(part))


@pytest.mark.gpu
@pytest.mark.parametrize("mod", [1.0, 3.0], ids=["mod1", "mod3"])
@pytest.mark.parametrize("view", list(VIEWS))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_slabs_are_exact_under_any_view(oracle, shape, view, mod):
    W, H, ts = shape
    check_slabs(oracle, splats(), uniforms(W, H, view, mod), W, H, ts, PARTITIONS[ts])


@pytest.mark.gpu
def test_an_overflowing_norm_keeps_every_gaussian(oracle):
    """A finite view scaled by 2^65: the factor is +inf in f32.  The cull then drops nothing, the slabs are still the oracle's."""
    W, H, ts = SHAPES[0]
    check_slabs(oracle, splats(), uniforms(W, H, "k2^65"), W, H, ts, PARTITIONS[ts])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_slabs_are_exact_at_the_reach_margin(oracle, shape):
    W, H, ts = shape
    s, u, _, _ = margin_scene(oracle, W, H, ts)
    check_slabs(oracle, s, u, W, H, ts, PARTITIONS[ts])


@pytest.mark.gpu
def test_fused_slabs_under_a_scaled_view(oracle):
    """Flags 0 (the fused blend) under k = 8: the lists as above, the image within check_image's envelope."""
    from gpu_checks import check_image, check_product_lists
    W, H, ts = SHAPES[0]
    s, u = splats(), uniforms(W, H, "k8")
    for cols in slabs_of(ts):
        ref = oracle.render(s, u, W, H, ts, cols=cols, want_illcond=True)
        r = mk(s, W, H, ts, cols=cols)
        r.render_uniforms(u)
        r.wait()
        check_product_lists(r, ref, oracle, W, H, ts)
        check_image(r, ref, exact_image=False)
        r.destroy()


@pytest.mark.gpu
def test_hidden_splats_on_slabs_under_a_scaled_view(oracle):
    """GS_FLAG_SPLAT_STATE (the STATE instantiations of the projection) with every third splat hidden, under k = 8."""
    import state_restate as sr
    from gpu_checks import check_stages
    W, H, ts = SHAPES[0]
    s, u = splats(), uniforms(W, H, "k8")
    state = np.where(np.arange(s.shape[0]) % 3 == 1, sr.HIDDEN, 0).astype(np.uint8)
    for cols in slabs_of(ts):
        ref = sr.state_frame(oracle, s, u, W, H, ts, state, cols=cols)
        r = mk(s, W, H, ts, exact=True, state=True, cols=cols)
        r.write_state(state)
        r.render_uniforms(u, debug=True)
        r.wait()
        check_stages(r, ref, exact_image=True)
        r.render_uniforms(u)
        r.wait()
        check_stages(r, ref, exact_image=True, debug=False, oracle=oracle, W=W, H=H)
        r.destroy()


@pytest.mark.gpu
def test_frame_graph_carries_the_view_norm(oracle):
    """GS_OPT_FRAME_GRAPH on slab contexts: a rigid frame captures the graph, the k = 8 frame replays it.  Whatever the reach bound
    needs of the view has to travel with the replayed frame's uniforms."""
    from gsplat import _abi
    from gpu_checks import check_stages
    W, H, ts = SHAPES[0]
    s = splats()
    for cols in ((0, 1), (5, 6), (6, 9), (9, 16)):
        r = mk(s, W, H, ts, exact=True, cols=cols)
        r.set_option(_abi.GS_OPT_FRAME_GRAPH, 1)
        for k, view in enumerate(("rigid", "k8", "rigid", "shear")):
            u = uniforms(W, H, view)
            r.render_uniforms(u)
            r.wait()
            check_stages(r, oracle.render(s, u, W, H, ts, cols=cols), exact_image=True, debug=False, oracle=oracle, W=W, H=H)
            assert r.stats()["graph_frames"] == k + 1, (cols, view)
        r.destroy()
