"""The two reference-binning pipelines at the tile counts where their instance sort changes its plan.

Both pipelines pick their code path from M = ntx * (nty + 1), the largest tile id a rect can produce (row nty and column ntx, the
clamp row and column, included).  The rules are restated here and never read from the library:

  full-key sort (GS_OPT_EMIT_ORDER 1 and every debug frame)   passes = ceil(bits(M * 1000 + 999) / 8), 8-bit digits
  tile sort (GS_OPT_EMIT_ORDER 0)                             passes = ceil(bits(M) / 8), digits of ceil(bits(M) / passes) bits,
                                                              u16 sort words while M < 0xFFFF, else u32 keys sorted by key / 1000

PLAN_GRIDS puts one canvas on either side of every boundary of those rules (and on M = 65534, the largest u16 id, one below the
ranges kernel's 0xFFFF pad; M = 65535, the one canvas whose u32 keys are sorted by key / 1000 in two 8-bit passes; M = 2, one 2-bit
digit).  EXACT_GRIDS x EXACT_COUNTS then set the instance count I of a frame exactly, around the emission chunk (1024 slots), the
sort tile (8192 pairs: the full and the padded sweep) and every residue of the ranges kernels' 4- and 8-key vector loads.

Every frame is compared with the CPU oracle bit for bit: all taps of a debug frame, keys (the u16 frames rebuild theirs), values,
ranges, counts and the EXACT image of product frames in both emission orders.  Nothing here has a tolerance.
"""
import numpy as np
import pytest

from gpu_checks import check_stages
from support import cached, mk, pinhole

# M -> (ntx, nty) with M = ntx * (nty + 1); the canvas is (ts * ntx) x (ts * nty)
PLAN_GRIDS = {2: (1, 1), 64: (8, 7), 65: (5, 12), 255: (15, 16), 256: (16, 15), 1023: (33, 30), 1024: (32, 31), 4095: (63, 64),
              4096: (64, 63), 16383: (127, 128), 16384: (128, 127), 16776: (72, 232), 16777: (883, 18), 65534: (302, 216),
              65535: (255, 256), 65536: (256, 255)}
PLAN_CASES = [(M, 8) for M in PLAN_GRIDS] + [(65, 16), (16384, 16)]  # (tile 16: key / 1000 is not only ever taken of tile-8 ids)
EXACT_GRIDS = (255, 1024, 65535, 65536)  # one per family of the tile sort: u16 one pass; u16 2 x 6 bits; u32 2 x 8; u32 3 x 6
EXACT_COUNTS = (1, 1023, 1024, 1025, 8191, 8192, 8193, 16388)  # mod 8: 1 7 0 1 7 0 1 4;  mod 4: 1 3 0 1 3 0 1 0
MAX_INSTANCES = 1 << 20


def bits(v):
    return int(v).bit_length()


def expected_plan(M):
    """What the rules above give for M: passes of the full-key sort, passes and bits per digit of the tile sort, u16 words."""
    full = -(-bits(M * 1000 + 999) // 8)
    tile = -(-bits(M) // 8)
    return {"full_passes": full, "tile_passes": tile, "tile_bits": -(-bits(M) // tile), "u16": M < 0xFFFF}


def test_the_plan_rules_switch_where_the_cases_say():
    """The restated rules really change between the neighbours the cases were chosen as."""
    p = {M: expected_plan(M) for M in PLAN_GRIDS}
    assert all(ntx * (nty + 1) == M for M, (ntx, nty) in PLAN_GRIDS.items())
    assert [p[M]["full_passes"] for M in (64, 65, 16776, 16777)] == [2, 3, 3, 4]
    assert [p[M]["tile_passes"] for M in (255, 256, 65535, 65536)] == [1, 2, 2, 3]
    assert [p[M]["tile_bits"] for M in (2, 255, 256, 1023, 1024, 4095, 4096, 16383, 16384, 65535, 65536)] == [2, 8, 5, 5, 6, 6, 7, 7, 8, 8, 6]
    assert [p[M]["u16"] for M in (65534, 65535)] == [True, False]


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------
def _records(ndc_x, ndc_y, z, scale, logit, rng):
    """Records under support.pinhole: centres at the NDC positions and depths z, log-scales of `scale` (n or n x 3), identity rotation."""
    n = np.size(z)
    z = np.asarray(z, np.float64)
    s = np.zeros((n, 80), dtype=np.float32)
    s[:, 0] = (np.asarray(ndc_x, np.float64) * z).astype(np.float32)
    s[:, 1] = (np.asarray(ndc_y, np.float64) * z).astype(np.float32)
    s[:, 2] = z.astype(np.float32)
    s[:, 4:7] = np.log(np.broadcast_to(np.reshape(scale, (n, -1)), (n, 3))).astype(np.float32)
    s[:, 8] = 1.0
    s[:, 12] = logit
    s[:, 16:19] = rng.uniform(0.2, 1.5, (n, 3)).astype(np.float32)
    return s


def small_splats(ntx, nty, ts, rng, n=3000):
    """n splats of 0.5 .. 3 pixels of sigma at NDC positions uniform in +-1.08 (the frustum test passes up to 1.1: the centres past
    +-1 land in the clamp column ntx and the clamp row nty, whose column is the alias of SURVEY A.3); depths 0.5 .. 19, about 900 buckets."""
    W, H = ts * ntx, ts * nty
    z = rng.uniform(0.5, 19.0, n)
    sig = rng.uniform(0.5, 3.0, (n, 1))
    scale = np.concatenate([sig / (W / 2.0), sig / (H / 2.0), np.full((n, 1), 1e-3)], axis=1) * z[:, None]
    return _records(rng.uniform(-1.08, 1.08, n), rng.uniform(-1.08, 1.08, n), z, scale, rng.uniform(-2.0, 2.0, n), rng)


def corner_splats(rng):
    """Four splats just outside the four corners (NDC +-1.05): tile 0 .. tile M = ntx * nty + ntx."""
    x = np.array([-1.05, 1.05, -1.05, 1.05])
    y = np.array([-1.05, -1.05, 1.05, 1.05])
    z = rng.uniform(0.5, 19.0, 4)
    return _records(x, y, z, 1e-4 * z, rng.uniform(-2.0, 2.0, 4), rng)


def whole_canvas(rng, k):
    """Faint splats over the whole canvas (sigma = 3 in NDC): (ntx + 1) (nty + 1) instances each."""
    z = rng.uniform(0.5, 19.0, k)
    return _records(np.zeros(k), np.zeros(k), z, 3.0 * z, np.full(k, -4.0), rng)


def filler(ntx, nty, ts, tiles, z, rng):
    """One splat per entry of `tiles` (tile ids ty * ntx + tx, ty <= nty) centred on the tile's centre, sigma 1e-4 z: the projected
    covariance is the 0.3 px^2 floor, the 3-sigma radius 2 pixels, the rect that one tile -- a tile count of exactly 1."""
    W, H = ts * ntx, ts * nty
    tiles = np.asarray(tiles, np.int64)
    px = ts * (tiles % ntx) + ts / 2.0
    py = ts * (tiles // ntx) + ts / 2.0
    z = np.asarray(z, np.float64)
    return _records(2.0 * px / W - 1.0, 2.0 * py / H - 1.0, z, 1e-4 * z, rng.uniform(-2.0, 2.0, tiles.size), rng)


def plan_scene(ntx, nty, ts, key):
    """About 3000 small splats, the four corners, and three whole-canvas splats at the first, the middle and the last index (each the
    single owner of dozens of emission chunks and, on the large canvases, of several sort tiles).  Returns (splats, uniforms, W, H)."""
    def make():
        rng = np.random.Generator(np.random.Philox(key=[5150, key]))
        small, corners, whole = small_splats(ntx, nty, ts, rng), corner_splats(rng), whole_canvas(rng, 3)
        h = small.shape[0] // 2
        s = np.concatenate([whole[0:1], small[:h], corners[:2], whole[1:2], corners[2:], small[h:], whole[2:3]])
        return s, pinhole(ts * ntx, ts * nty), ts * ntx, ts * nty
    return cached(("plan_scene", ntx, nty, ts, key), make)


def exact_scene(oracle, ntx, nty, ts, I, key):
    """A scene of exactly I instances: a base (in record order the four corners, one whole-canvas splat and small splats, each kept
    while the base stays at or below I / 2 -- so the large canvases and the small I go without the whole-canvas splat) and one
    filler per missing instance.  Half of the fillers sit on tiles of the last tile row of the canvas and of the clamp row nty below
    it (the largest ids: the top digit of every plan set), at the END of the record order, the last eight of them also deeper than
    everything else: in both emission orders the last, padded sort tile then holds those ids next to its pads."""
    def make():
        rng = np.random.Generator(np.random.Philox(key=[5151, key]))
        W, H = ts * ntx, ts * nty
        u = pinhole(W, H)
        cand = np.concatenate([corner_splats(rng), whole_canvas(rng, 1), small_splats(ntx, nty, ts, rng)])
        counts = oracle.preprocess(cand, u, W, H, ts)[1].astype(np.int64)
        keep, have = np.zeros(cand.shape[0], bool), 0
        for i, c in enumerate(counts):
            if c and have + c <= I // 2:
                keep[i], have = True, have + int(c)
        k = I - have
        rows = [nty - 1] + ([nty] if (ts * nty + ts / 2.0) / (ts * nty) * 2.0 - 1.0 < 1.08 else [])  # (a centre in the clamp row must pass the frustum test)
        last = np.concatenate([r * ntx + np.arange(ntx) for r in rows])
        forced = last[rng.integers(0, last.size, k // 2)]
        forced[-1:] = last[-1]
        tiles = np.concatenate([rng.integers(0, ntx * nty, k - forced.size), forced])
        z = rng.uniform(0.5, 19.0, k)
        z[k - min(k, 8):] = np.sort(rng.uniform(19.5, 19.9, min(k, 8)))
        return np.concatenate([cand[keep], filler(ntx, nty, ts, tiles, z, rng)]), u, W, H
    return cached(("exact_scene", ntx, nty, ts, I, key), make)


def behind_scene(ntx, nty, ts):
    s, u, W, H = plan_scene(ntx, nty, ts, 256)
    s = s.copy()
    s[:, 0:3] *= -1.0  # (ndc unchanged, depth negative)
    return s, u, W, H


def _lists(oracle, s, u, W, H, ts):
    """The oracle's stages up to the sorted keys (no blend)."""
    gdata, counts = oracle.preprocess(s, u, W, H, ts)
    offsets, total = oracle.scan(counts)
    keys, values = oracle.emit(gdata, offsets, counts, total, W, ts)
    return counts, total, keys, oracle.sort(keys, values)[0]


@pytest.mark.parametrize("M,ts", PLAN_CASES)
def test_plan_scenes_reach_what_they_are_for(oracle, M, ts):
    """On the oracle alone: tile 0 and tile M occur, at least 500 depth buckets, at least one whole-canvas count, at most 1 Mi instances."""
    ntx, nty = PLAN_GRIDS[M]
    s, u, W, H = plan_scene(ntx, nty, ts, M)
    assert oracle.num_tiles(W, H, ts) == (ntx, nty)
    counts, total, _, skeys = _lists(oracle, s, u, W, H, ts)
    tile = skeys.astype(np.int64) // 1000
    assert tile.min() == 0 and tile.max() == M
    assert np.unique(skeys.astype(np.int64) % 1000).size >= 500
    assert int((counts == (ntx + 1) * (nty + 1)).sum()) >= 1
    assert 0 < total <= MAX_INSTANCES


@pytest.mark.parametrize("M", EXACT_GRIDS)
def test_exact_scenes_have_their_instance_counts(oracle, M):
    """On the oracle alone: every exact scene has exactly I instances, the 8191 .. 8193 ones with ids of the last tile rows at the end of
    both emission orders; a filler has a tile count of 1, on its own tile, on 500 random tiles."""
    ntx, nty = PLAN_GRIDS[M]
    for I in EXACT_COUNTS:
        s, u, W, H = exact_scene(oracle, ntx, nty, 8, I, M)
        counts, total, keys, skeys = _lists(oracle, s, u, W, H, 8)
        assert total == I <= MAX_INSTANCES and skeys.size == I
        if I >= 8191:
            # the last record owns the last instance of the index order; being in the deepest bucket too, it owns the last one of the
            # (bucket, index) order as well: in both, the instance next to the pads is on one of the last tile rows
            assert counts[-1] == 1 and int(keys[-1]) // 1000 >= (nty - 1) * ntx
            assert int(keys[-1]) % 1000 == int((keys % 1000).max())
            assert int((skeys.astype(np.int64) // 1000 >= (nty - 1) * ntx).sum()) >= 2000
    rng = np.random.Generator(np.random.Philox(key=[5152, M]))
    tiles = rng.integers(0, ntx * nty, 500)
    f = filler(ntx, nty, 8, tiles, rng.uniform(0.5, 19.0, 500), rng)
    gdata, counts = oracle.preprocess(f, pinhole(8 * ntx, 8 * nty), 8 * ntx, 8 * nty, 8)
    np.testing.assert_array_equal(counts, 1)
    np.testing.assert_array_equal(gdata[:, 13].astype(np.int64) * ntx + gdata[:, 12], tiles)


def test_behind_scene_has_no_instance(oracle):
    ntx, nty = PLAN_GRIDS[256]
    s, u, W, H = behind_scene(ntx, nty, 8)
    assert _lists(oracle, s, u, W, H, 8)[1] == 0 and s.shape[0] > 3000


# ---- the frames ---------------------------------------------------------------------------------------------------------------------
def _product_frames(oracle, r, u, ref, W, H, plan, report=None):
    """A product frame of the reference's binning in each emission order: lists, ranges, counts and the EXACT image against the oracle,
    the frame's order and the passes of its instance sort against the plan."""
    from gsplat import _abi
    r.set_option(_abi.GS_OPT_TILE_CULL, 0)
    for order in (1, 0):  # gaussian-index order + full-key sort; depth-ordered emission + tile sort
        r.set_option(_abi.GS_OPT_EMIT_ORDER, order)
        r.render_uniforms(u)
        r.wait()
        check_stages(r, ref, exact_image=True, debug=False, oracle=oracle, W=W, H=H)
        st = r.stats()
        if report is not None:
            report["order%d" % order] = st["sort_passes"]
        assert st["tight_binning"] == 0 and st["depth_ordered"] == 1 - order
        assert st["sort_passes"] == (plan["full_passes"] if order else plan["tile_passes"])


@pytest.mark.gpu
@pytest.mark.parametrize("M,ts", PLAN_CASES)
def test_frames_at_the_plan_boundaries(oracle, M, ts):
    ntx, nty = PLAN_GRIDS[M]
    s, u, W, H = plan_scene(ntx, nty, ts, M)
    plan = expected_plan(M)
    ref = oracle.render(s, u, W, H, ts)
    r = mk(s, W, H, ts, exact=True)
    r.render_uniforms(u, debug=True)
    r.wait()
    check_stages(r, ref, exact_image=True)  # every tap, the unsorted keys included
    rep = {"debug": r.stats()["sort_passes"]}
    assert rep["debug"] == plan["full_passes"] and r.stats()["depth_ordered"] == 0
    _product_frames(oracle, r, u, ref, W, H, plan, rep)
    r.destroy()
    print("M %d tile %d: I %d, expected %s, sort_passes %s" % (M, ts, ref["num_intersections"], plan, rep))


@pytest.mark.gpu
@pytest.mark.parametrize("I", EXACT_COUNTS)
@pytest.mark.parametrize("M", EXACT_GRIDS)
def test_exact_instance_counts(oracle, M, I):
    ntx, nty = PLAN_GRIDS[M]
    s, u, W, H = exact_scene(oracle, ntx, nty, 8, I, M)
    ref = oracle.render(s, u, W, H, 8)
    assert ref["num_intersections"] == I
    r = mk(s, W, H, 8, exact=True)
    _product_frames(oracle, r, u, ref, W, H, expected_plan(M))
    r.destroy()


@pytest.mark.gpu
def test_no_instance_at_all(oracle):
    ntx, nty = PLAN_GRIDS[256]
    s, u, W, H = behind_scene(ntx, nty, 8)
    ref = oracle.render(s, u, W, H, 8)
    assert ref["num_intersections"] == 0
    r = mk(s, W, H, 8, exact=True)
    _product_frames(oracle, r, u, ref, W, H, expected_plan(256))
    r.destroy()
