"""The tight pipeline hands the cull's survivors to the gaussian-level sort DENSELY (k_preprocess.hip -> k_gsort.hip).

The projection compacts the survivors of every UNIT of 1024 consecutive gaussian indices in index order and writes survivor e of
unit u at entry u * 1024 + e of three planes (count word, arena address, index inside the unit) plus unit_n[u]; a sort chunk is
two units, and the sort walks the T = n0 + n1 entries of a chunk as positions that its four waves own in ascending ranges.
Nothing a caller sees changes, so every GPU case renders a scene in the tight binning and compares
  * the EXACT image and the lists with the CPU oracle (gpu_checks.check_stages: nothing has a tolerance), and
  * the KEYS / VALUES / RANGES / TILE_COUNTS / GAUSSIAN_DATA taps with the SAME context's frame of the reference's binning
    (GS_OPT_TILE_CULL 0), whose count words are indexed by the gaussian: per tile the tight (key, value) list is a subsequence of
    that frame's -- the keys of a tight frame are rebuilt from the records' depth words -- the ranges and tile counts are those of
    the list, and the records of the listed gaussians are bit-equal.
The CPU tests restate the position -> (unit, entry) mapping and the waves' ranges in numpy, for every T and every split.
"""
import ctypes

import numpy as np
import pytest

from conftest import scene
from support import cached, mk, oracle_frame, pinhole
import state_restate as sr

GU, GC = 1024, 2048  # gaussian indices per unit / per chunk of the sort (k_gsort.hip)
W, H, TS = 256, 160, 16
TAPS = ("KEYS", "VALUES", "RANGES", "TILE_COUNTS", "GAUSSIAN_DATA")


# ---- CPU: the sort's addressing, restated -----------------------------------------------------------------------------------------
def _wave_positions(T):
    """(position, valid) of item j, lane l of wave w, in (w, j, l) order: what gs_gsort_scatter_kernel<true> computes."""
    R = (T + 255) // 256
    L = 64 * R
    w, j, l = np.meshgrid(np.arange(4), np.arange(8), np.arange(64), indexing="ij")
    p = w * L + j * 64 + l
    return p.ravel(), ((j < R) & (p < T)).ravel()


def test_wave_ranges_cover_every_position_once_in_order():
    """For every T in 0..2048: the positions the four waves hold are exactly 0 .. T-1, each once, and ascending in (wave, item,
    lane) order -- so a wave's items are in index order and the waves own ascending ranges, which is what keeps the rank stable."""
    for T in range(GC + 1):
        p, ok = _wave_positions(T)
        np.testing.assert_array_equal(p[ok], np.arange(T), err_msg="T = %d" % T)
        R = (T + 255) // 256
        assert R <= 8 and 4 * 64 * R >= T
        assert not ok.reshape(4, 8, 64)[:, R:].any()  # rounds past T hold nothing, in every wave


def test_position_to_entry_for_every_split():
    """For every T in 0..2048 and every split n0 + n1 = T with n0, n1 <= 1024: position p is entry p of the chunk's first unit
    when p < n0, else entry p - n0 of the second.  As slots of the chunk's 2048 (unit * 1024 + entry) the positions must hit
    0 .. n0-1 and 1024 .. 1024+n1-1, ascending: strictly increasing slots with the right values at the three joints."""
    splits = 0
    for T in range(GC + 1):
        n0 = np.arange(max(0, T - GU), min(T, GU) + 1, dtype=np.int16)[:, None]
        n1 = (T - n0).astype(np.int16)
        splits += n0.size
        if T == 0:
            continue
        p = np.arange(T, dtype=np.int16)[None, :]
        slot = p + (p >= n0) * (GU - n0)  # second unit: 1024 + (p - n0)
        assert (slot[:, 1:] > slot[:, :-1]).all(), "T = %d" % T
        rows = np.arange(n0.size)
        a, b = n0.ravel() > 0, n1.ravel() > 0
        assert (slot[rows[a], n0.ravel()[a] - 1] == n0.ravel()[a] - 1).all()       # the first unit's last entry
        assert (slot[rows[b], n0.ravel()[b]] == GU).all()                          # the second unit's first entry
        assert (slot[rows[b], T - 1] == GU + n1.ravel()[b] - 1).all()              # ... and its last
        assert (slot[rows[~b], T - 1] == T - 1).all()
    assert splits == (GU + 1) ** 2


def test_record_ids_are_the_visible_indices_in_order():
    """The whole path on random visibility masks of one chunk: the projection's planes (entries in index order, the offset inside
    the unit), then the sort's positions in wave order: id = (p < n0 ? 0 : 1024) + offset is the visible indices, ascending."""
    rng = np.random.Generator(np.random.Philox(key=[977, 50]))
    for density in (0.0, 0.02, 0.4, 0.97, 1.0):
        for _ in range(8):
            vis = rng.random(GC) < density
            off = np.zeros(GC, np.uint16)
            n = []
            for u in range(2):
                idx = np.flatnonzero(vis[u * GU:(u + 1) * GU])
                off[u * GU:u * GU + idx.size] = idx
                n.append(idx.size)
            p, ok = _wave_positions(n[0] + n[1])
            p = p[ok]
            second = p >= n[0]
            e = np.where(second, GU + (p - n[0]), p)
            np.testing.assert_array_equal(np.where(second, GU, 0) + off[e], np.flatnonzero(vis))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _taps(r, u):
    from gsplat import _abi
    r.render_uniforms(u)
    r.wait()
    out = {t: r.read_buffer(getattr(_abi, "GS_BUF_" + t)) for t in TAPS}
    out["GAUSSIAN_DATA"] = out["GAUSSIAN_DATA"].reshape(-1, 16)
    out["rgba8"], out["rgbf"], out["st"] = r.read_rgba8(), r.read_buffer(_abi.GS_BUF_RGB_F32), r.stats()
    return out


def _against_reference_binning(tight, rect, n):
    """The taps of a tight frame against those of the same context's frame with GS_OPT_TILE_CULL 0."""
    assert tight["st"]["tight_binning"] == 1 and rect["st"]["tight_binning"] == 0
    np.testing.assert_array_equal(tight["rgba8"], rect["rgba8"])
    np.testing.assert_array_equal(tight["rgbf"], rect["rgbf"])
    tk, tv, rk, rv = tight["KEYS"], tight["VALUES"], rect["KEYS"], rect["VALUES"]
    assert tk.size == tv.size and (tv < n).all()
    # (key, value) pairs: both lists ascend (the order inside a tile is (bucket, index)); every tight pair is one of the
    # reference frame's, as often at most (a pair can occur twice: the aliased column): an ordered sub-multiset
    tc = (tk.astype(np.uint64) << np.uint64(32)) | tv.astype(np.uint64)
    rc = (rk.astype(np.uint64) << np.uint64(32)) | rv.astype(np.uint64)
    assert (tc[1:] >= tc[:-1]).all() and (rc[1:] >= rc[:-1]).all()
    pos = np.searchsorted(rc, tc, "left") + (np.arange(tc.size) - np.searchsorted(tc, tc, "left"))
    assert tc.size == 0 or (pos.max() < rc.size and (rc[pos] == tc).all()), "a tight (key, value) pair is not in the reference binning's list"
    T = tight["RANGES"].size
    assert T == rect["RANGES"].size
    np.testing.assert_array_equal(tight["RANGES"], np.searchsorted(tk // 1000, np.arange(T), "right").astype(np.uint32))
    np.testing.assert_array_equal(tight["TILE_COUNTS"], np.bincount(tv, minlength=n).astype(np.uint32))
    assert (tight["TILE_COUNTS"] <= rect["TILE_COUNTS"]).all()
    listed = np.unique(tv)
    np.testing.assert_array_equal(tight["GAUSSIAN_DATA"][listed], rect["GAUSSIAN_DATA"][listed])


def _check(oracle, s, u, ref, G=4, chunks=None, cols=None, state=None):
    """One context: a tight frame, a frame of the reference's binning, a tight frame again (the two forms share `counts` and
    `rowptr`: nothing of one may reach the other).  Both tight frames against the oracle and against the frame in between."""
    from gpu_checks import check_stages
    from gsplat import _abi
    n = s.shape[0]
    r = mk(s, W, H, TS, exact=True, cols=cols, state=state is not None)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    r.set_option(_abi.GS_OPT_PERSISTENT_GRID, G)
    r.set_option(_abi.GS_OPT_EMIT_ORDER, 0)
    if chunks:
        r.set_option(_abi.GS_OPT_PROJ_CHUNKS, chunks)
    if state is not None:
        r.write_state(state)
    first = _taps(r, u)
    check_stages(r, ref, exact_image=True, debug=False)
    r.set_option(_abi.GS_OPT_TILE_CULL, 0)
    rect = _taps(r, u)
    check_stages(r, ref, exact_image=True, debug=False)
    r.set_option(_abi.GS_OPT_TILE_CULL, 1)
    again = _taps(r, u)
    check_stages(r, ref, exact_image=True, debug=False)
    r.destroy()
    _against_reference_binning(first, rect, n)
    for k in TAPS + ("rgba8", "rgbf"):
        np.testing.assert_array_equal(again[k], first[k], err_msg=k)
    return first


def _orbit(step):
    from gpu_checks import orbit_uniforms
    return orbit_uniforms(W, H, step)


def _small(z, key, logit=None):
    """One small round splat per depth in z, spread over the canvas of support.pinhole: visible iff z > 0."""
    n = z.size
    rng = np.random.Generator(np.random.Philox(key=[977, key]))
    z = np.asarray(z, dtype=np.float32)
    s = np.zeros((n, 80), dtype=np.float32)
    s[:, 0] = (rng.uniform(-0.95, 0.95, n) * z).astype(np.float32)
    s[:, 1] = (rng.uniform(-0.95, 0.95, n) * z).astype(np.float32)
    s[:, 2] = z
    s[:, 4:7] = np.log(rng.uniform(0.004, 0.02, (n, 3)) * np.abs(z)[:, None]).astype(np.float32)
    s[:, 8] = 1.0
    s[:, 12] = rng.uniform(-2.0, 2.0, n).astype(np.float32) if logit is None else logit
    s[:, 16:19] = rng.uniform(0.2, 1.5, (n, 3)).astype(np.float32)
    return s


N_RUNS = 9 * GC + 100  # 10 chunks, runs of 3 at G = 4: the last run holds one chunk, and that one is short


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 1, N_RUNS])
def test_gaussian_counts_around_unit_and_chunk_boundaries(oracle, n):
    s, u = scene(N_RUNS)[:n], _orbit(7)
    got = _check(oracle, s, u, oracle_frame(oracle, "gsort_dense_n%d" % n, s, u, W, H, TS))
    assert got["VALUES"].size > 0
    if n == N_RUNS:  # both units of every chunk hold survivors and culled gaussians
        vis = got["TILE_COUNTS"] > 0
        assert all(0 < int(vis[k * GU:(k + 1) * GU].sum()) < min(GU, n - k * GU) for k in range((n + GU - 1) // GU))


def _unit_scene():
    """Units that are full (F: every gaussian visible), empty (E) or mixed (M), 9 chunks in runs of 3 at G = 4:
    (F,E) (E,E) (E,F) | (F,F) (F,F) (M,M) | (E,E) (F,E) (M, short M)."""
    kinds = "FE EE EF FF FF MM EE FE MM".replace(" ", "")
    n = 8 * GC + GU + 777
    rng = np.random.Generator(np.random.Philox(key=[977, 51]))
    z = rng.uniform(1.0, 6.0, n)
    for k, kind in enumerate(kinds):
        sl = slice(k * GU, min((k + 1) * GU, n))
        if kind == "E":
            z[sl] *= -1.0
        elif kind == "M":
            z[sl] *= np.where(rng.random(z[sl].size) < 0.4, 1.0, -1.0)
    return z, kinds, n


@pytest.mark.gpu
def test_full_and_empty_units(oracle):
    """T = 1024 from the first unit alone, from the second alone, T = 2048, and T = 0 in the middle and at the start of a run."""
    z, kinds, n = _unit_scene()
    s, u = _small(z, 52), pinhole(W, H)
    ref = oracle_frame(oracle, "gsort_dense_units", s, u, W, H, TS)
    got = _check(oracle, s, u, ref)
    vis = got["TILE_COUNTS"] > 0
    for k, kind in enumerate(kinds):
        m = vis[k * GU:(k + 1) * GU]
        assert m.all() if kind == "F" else (not m.any()) if kind == "E" else (m.any() and not m.all()), "unit %d (%s)" % (k, kind)


@pytest.mark.gpu
def test_survivors_that_end_without_a_tile(oracle):
    """Holes among the entries: gaussians that pass the cull and get no tile -- opacity below 1/255, or a centre in the frustum's
    margin (ndc in 1 .. 1.1) whose ellipse stays off the canvas -- at the first, the last and an interior entry of units whose
    gaussians all pass the cull.  Their count word is 0: the sort skips them, their neighbours keep their order."""
    n = 3 * GC + 500
    rng = np.random.Generator(np.random.Philox(key=[977, 53]))
    z = rng.uniform(1.0, 6.0, n)
    s = _small(z, 54)
    faint = np.array([0, 500, GU - 1, GU, 3 * GU + 17, 4 * GU - 1, 6 * GU, n - 1])
    margin = np.array([1, 501, GU - 2, GU + 1, 2 * GU, 3 * GU - 1, 5 * GU + 300, n - 2])
    s[faint, 12] = -9.0                                          # sigmoid(-9) = 1.2e-4 < 1/255
    s[margin, 0] = (1.06 * z[margin]).astype(np.float32)         # ndc x = 1.06: inside the cull's 1.1, 7 pixels right of the canvas
    s[margin, 4:7] = np.log(0.002 * z[margin])[:, None].astype(np.float32)  # sigma = 0.26 px
    u = pinhole(W, H)
    ref = oracle_frame(oracle, "gsort_dense_holes", s, u, W, H, TS)
    got = _check(oracle, s, u, ref)
    # (a margin splat's rect is clamped into tile column ntx, which aliases to column 0 of the next tile row: whether the tight
    # binning proves that tile empty is its own business, so only the faint ones are asserted to be holes)
    assert not got["TILE_COUNTS"][faint].any()
    assert got["st"]["num_visible"] <= n - faint.size
    keep = np.ones(n, bool)
    keep[faint] = keep[margin] = False
    assert (got["TILE_COUNTS"][keep] > 0).all()


@pytest.mark.gpu
def test_hidden_splats_at_unit_boundaries(oracle):
    """GS_FLAG_SPLAT_STATE: the ordered compaction runs with the state byte; hidden splats on both sides of every unit boundary."""
    n = 3 * GC + 100
    s, u = scene(N_RUNS)[:n], _orbit(7)
    state = np.zeros(n, np.uint8)
    for b in range(0, n, GU):
        state[max(b - 2, 0):b + 2] = sr.HIDDEN
    state[np.arange(7, n, 5)] = sr.HIDDEN
    state[np.arange(3, n, 11)] |= sr.SELECTED
    ref = cached(("gsort_dense_hidden",), lambda: sr.state_frame(oracle, s, u, W, H, TS, state, want_illcond=True))
    got = _check(oracle, s, u, ref, state=state)
    assert got["VALUES"].size > 0 and not (state[got["VALUES"]] & sr.HIDDEN).any()


@pytest.mark.gpu
@pytest.mark.parametrize("chunks,cols", [(2, None), (4, None), (8, None), (4, (7, 9)), (8, (7, 9))])
def test_cull_chunks_per_workgroup(oracle, chunks, cols):
    """GS_OPT_PROJ_CHUNKS 4 / 8: one workgroup writes 2 / 4 units (a unit's first survivor is the prefix at round 4k; at 8 the
    running total crosses the two groups of rounds), on the whole canvas and on a two-column slab (few survivors per unit)."""
    s, u = scene(N_RUNS), _orbit(7)
    ref = oracle_frame(oracle, "gsort_dense_n%d" % N_RUNS, s, u, W, H, TS, cols=cols)
    got = _check(oracle, s, u, ref, chunks=chunks, cols=cols)
    assert got["VALUES"].size > 0


@pytest.mark.gpu
def test_three_frames_in_flight_match_one_at_a_time():
    """GS_OPT_FRAMES_IN_FLIGHT 3 over four orbit cameras, two laps: every frame equals its one-at-a-time render.  Each ring member
    has entry planes and unit counts of its own."""
    from gsplat import _abi
    L = _abi.load()
    s = scene(N_RUNS)
    us = [_orbit(k) for k in (2, 6, 11, 17)]
    seq = mk(s, W, H, TS)
    seq.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    want = []
    for u in us:
        seq.render_uniforms(u)
        seq.wait()
        assert seq.stats()["tight_binning"] == 1
        want.append(seq.read_rgba8())
    seq.destroy()
    assert all((want[0] != w).any() for w in want[1:])
    r = mk(s, W, H, TS)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 3)
    for k in range(3):  # opens the ring: every member sees a frame and grows to it
        r.render_uniforms(us[k])
    r.wait()
    nbytes = W * H * 4
    sinks, tickets = [], []
    for k in range(8):
        p, t = ctypes.c_void_p(), ctypes.c_uint64()
        _abi.check(L.gs_host_alloc(nbytes, ctypes.byref(p)))
        sinks.append(p)
        uu = np.ascontiguousarray(us[k % 4], dtype=np.float32)
        _abi.check(L.gs_render_host(r._ctx, uu.ctypes.data, p, nbytes, ctypes.byref(t)))
        tickets.append(t.value)
    for k in range(8):
        _abi.check(L.gs_wait_ticket(r._ctx, tickets[k]))
        got = np.ctypeslib.as_array(ctypes.cast(sinks[k], ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,)).reshape(H, W, 4)
        np.testing.assert_array_equal(got, want[k % 4], err_msg="frame %d" % k)
    r.wait()
    st = r.stats()
    assert st["frames_in_flight"] == 3 and st["tight_binning"] == 1
    r.destroy()
    for p in sinks:
        L.gs_host_free(p)
