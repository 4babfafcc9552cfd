"""The gaussian-level sort (k_gsort.hip) with SEVERAL chunks per workgroup run.

The sort cuts its 2048-index chunks into G contiguous runs (G follows GS_OPT_PERSISTENT_GRID); a run's workgroup carries its
bucket bases from chunk to chunk.  At test sizes the default grid (4 workgroups per CU) leaves one chunk per run, so these
tests force G = 4, 8 and 12 (the row pipeline takes a quarter of the value as its own grid: not 1-3) and render scenes whose
gaussian counts straddle the run arithmetic, in BOTH binnings that call the sort: the tight row pipeline (GS_OPT_TILE_CULL 1)
and the depth-ordered emission of the reference's binning (GS_OPT_TILE_CULL 0, GS_OPT_EMIT_ORDER 0).  Every frame is compared
with the CPU oracle: sorted values / ranges (equal, or the proven ordered subset of the tight binning) and the EXACT image,
bit for bit.  Nothing here has a tolerance.
"""
import numpy as np
import pytest

from conftest import scene
from gpu_checks import check_stages, make_renderer, orbit_uniforms
from support import pinhole as _pinhole

pytestmark = pytest.mark.gpu

GC = 2048  # gaussian indices per chunk (k_gsort.hip)
W, H, TS = 256, 160, 16


def _both_binnings(oracle, s, u, G, ref=None, W=W, H=H):
    """Renders the scene with G runs through both callers of the sort and checks each frame against the oracle."""
    from gsplat import _abi
    if ref is None:
        ref = oracle.render(s, u, W, H, TS)
    r = make_renderer(s, W, H, TS, flags=_abi.GS_FLAG_EXACT_BLEND)
    r.set_option(_abi.GS_OPT_PERSISTENT_GRID, G)
    r.set_option(_abi.GS_OPT_EMIT_ORDER, 0)
    for tight in (1, 0):
        r.set_option(_abi.GS_OPT_TILE_CULL, tight)
        r.render_uniforms(u)
        r.wait()
        st = r.stats()
        assert st["tight_binning"] == tight
        if not tight:
            assert st["depth_ordered"] == 1
            np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_VALUES), ref["sorted_values"])
            np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_RANGES), ref["ranges"])
        check_stages(r, ref, exact_image=True, debug=False)  # GS_BUF_VALUES / GS_BUF_RANGES / image against the oracle
    r.destroy()
    return ref


def _buckets(ref):
    return np.unique(ref["sorted_keys"].astype(np.int64) % 1000)


def _small_splats(n, z, key):
    """n small round splats spread over the canvas of _pinhole at the depths z."""
    rng = np.random.Generator(np.random.Philox(key=[977, key]))
    z = np.asarray(z, dtype=np.float32)
    s = np.zeros((n, 80), dtype=np.float32)
    s[:, 0] = (rng.uniform(-0.95, 0.95, n) * z).astype(np.float32)
    s[:, 1] = (rng.uniform(-0.95, 0.95, n) * z).astype(np.float32)
    s[:, 2] = z
    s[:, 4:7] = np.log(rng.uniform(0.004, 0.02, (n, 3)) * np.abs(z)[:, None]).astype(np.float32)
    s[:, 8] = 1.0
    s[:, 12] = rng.uniform(-2.0, 2.0, n).astype(np.float32)
    s[:, 16:19] = rng.uniform(0.2, 1.5, (n, 3)).astype(np.float32)
    return s


_N_CASES = [(1, 4), (2047, 4), (2048, 4), (2049, 4)]
_N_CASES += [(G * GC + d, G) for G in (4, 8, 12) for d in (-1, 0, 1)]
_N_CASES += [(9 * GC + 100, 4),   # 10 chunks in runs of 3: the last run holds ONE chunk, and that one is short
             (24 * GC + 7, 8),    # 25 chunks in runs of 4: 7 runs for G = 8, the last one a single chunk of 7 gaussians
             (27 * GC, 12)]       # 27 chunks in runs of 3: 9 runs for G = 12


@pytest.mark.parametrize("n,G", _N_CASES)
def test_gaussian_counts_around_the_run_arithmetic(oracle, n, G):
    s, u = scene(n), orbit_uniforms(W, H, step=7)
    ref = _both_binnings(oracle, s, u, G)
    if n >= 2047:
        assert _buckets(ref).size >= 20


def test_many_buckets_populated(oracle):
    """An orbit camera over the bicycle-like scene: the visible gaussians of every chunk spread over many depth buckets
    (asserted: at least 20 distinct ones, far more in fact), so every trip of a run advances many carried bases."""
    n = 30000  # 15 chunks: G = 4 -> runs of 4, 4, 4, 3;  G = 8 -> runs of 2 (the last a single chunk)
    s = scene(n)
    for G, step in ((4, 21), (8, 40)):
        u = orbit_uniforms(W, H, step=step)
        ref = _both_binnings(oracle, s, u, G)
        assert _buckets(ref).size >= 20
        vis = ref["tile_counts"] > 0
        assert all(vis[c * GC:(c + 1) * GC].any() for c in range(15))


def test_every_gaussian_in_one_bucket(oracle):
    """All depths inside one bucket (50 * depth in [100.1, 100.9]): the carried base of that single bucket crosses every chunk
    of every run, and the whole frame is one (bucket, index) sequence."""
    n = 10 * GC  # G = 4: runs of 3, 3, 3, 1
    rng = np.random.Generator(np.random.Philox(key=[977, 1]))
    s = _small_splats(n, rng.uniform(2.002, 2.018, n), 2)
    u = _pinhole(W, H)
    ref = _both_binnings(oracle, s, u, 4)
    assert _buckets(ref).tolist() == [100]
    assert int((ref["tile_counts"] > 0).sum()) > 9 * GC


def test_invisible_chunks_inside_a_run(oracle):
    """Whole chunks behind the camera at the start, in the middle and at the end of a run: a trip that finds nothing visible must
    neither move the bases nor end the workgroup's loop, and the chunks behind it must still come out in order."""
    NT, G = 10, 4  # runs {0,1,2} {3,4,5} {6,7,8} {9}
    hidden = (1, 3, 4, 8)  # middle of run 0; first and middle of run 1; last of run 2
    n = NT * GC
    rng = np.random.Generator(np.random.Philox(key=[977, 3]))
    z = rng.uniform(1.0, 6.0, n)  # buckets 50 .. 300
    for c in hidden:
        z[c * GC:(c + 1) * GC] *= -1.0
    s = _small_splats(n, z, 4)
    u = _pinhole(W, H)
    ref = oracle.render(s, u, W, H, TS)
    vis = ref["tile_counts"] > 0
    for c in range(NT):
        assert vis[c * GC:(c + 1) * GC].any() == (c not in hidden)
    assert _buckets(ref).size >= 20
    _both_binnings(oracle, s, u, G, ref=ref)
    # and a frame in which NOTHING is visible: every trip of every run is empty
    s2 = _small_splats(n, -np.abs(z), 5)
    ref2 = _both_binnings(oracle, s2, u, G)
    assert ref2["num_intersections"] == 0
