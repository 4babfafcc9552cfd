"""GPU: the tight projection stores a gaussian's GaussianData record at a RECORD SLOT handed out per workgroup trip (16 shards
of bump cursors, k_preprocess.hip), the tile lists name slots, and the gaussian's id rides in the record.  Slot order varies from
run to run; nothing a caller can observe may depend on it.  Every case renders the same camera three ways on ONE context --
gs_render_debug, gs_render with GS_OPT_TILE_CULL 0 (the reference's binning: slot = index) and gs_render with tight binning --
and compares what the three frames leave.

Shapes: the tight projection's workgroup is 1024 gaussians on the whole canvas (4096 on a narrow slab) and the slots come from
16 shards picked by workgroup % 16, so n = 1, 1023 / 1024 / 1025 (one workgroup, full, one splat into the second) and
17 * 1024 + 3 (18 workgroups: shards 0 and 1 serve two of them, the last one holds 3 splats); a scene entirely outside the
frustum (no record at all); a 3-column slab (the 8-chunk kernel); a context with a state plane and hidden splats."""
import ctypes

import numpy as np
import pytest

from conftest import scene
from support import hidden_plane, lattice, make_splats, mk, oracle_frame, pixel_uniforms, state_ref, state_scene

pytestmark = pytest.mark.gpu

W = H = 256
TS = 16
N_BIG = 17 * 1024 + 3


def _orbit(step=3):
    from gpu_checks import orbit_uniforms
    return orbit_uniforms(W, H, step)


def _case(oracle, name):
    """(splats, uniforms, oracle frame, cols, state plane or None) of one shape."""
    cols = state = None
    if name == "n1":
        s = make_splats(W, H, [100.0], [77.0], 9.0, 4.0, 0.4, np.array([2.0], np.float32), color=[[0.5, -0.2, 0.9]])
        u = pixel_uniforms(W, H)
    elif name == "outside":  # ndc x = 5 .. 9: in_frustum fails for every splat
        k = 1500
        s = make_splats(W, H, np.linspace(3.0 * W, 5.0 * W, k), np.full(k, 90.0), 6.0, 6.0, 0.0, np.full(k, 1.0, np.float32),
                        rng=np.random.default_rng(3))
        u = pixel_uniforms(W, H)
    elif name in ("slab", "hidden"):
        s, u, _, _ = state_scene("cfgA")
        if name == "slab":
            cols = (2, 5)
        else:
            state = hidden_plane("cfgA", "every_third")
            return s, u, state_ref(oracle, "cfgA", TS, "every_third", state), cols, state
    else:
        s, u = scene(N_BIG)[:int(name[1:])], _orbit()
    return s, u, oracle_frame(oracle, "record_slots_" + name, s, u, W, H, TS, cols=cols), cols, state


def _subsequence(a, b):
    it = iter(b.tolist())
    return all(x in it for x in a.tolist())


def _frame(r, u, xy, **kw):
    """One frame and everything the checks compare: image, f32 tap, list taps, records, picks, coverage planes."""
    from gsplat import _abi
    r.render_uniforms(u, **kw)
    r.wait()
    out = {"st": r.stats(), "rgba8": r.read_rgba8(), "rgbf": r.read_buffer(_abi.GS_BUF_RGB_F32),
           "vals": r.read_buffer(_abi.GS_BUF_VALUES), "ranges": r.read_buffer(_abi.GS_BUF_RANGES),
           "gdata": r.read_buffer(_abi.GS_BUF_GAUSSIAN_DATA).reshape(-1, 16), "counts": r.read_buffer(_abi.GS_BUF_TILE_COUNTS),
           "pick": r.pick(xy)}
    r.reset_coverage()
    r.accumulate_coverage()
    out["cover"] = r.read_coverage()
    return out


@pytest.mark.parametrize("name", ["n1", "n1023", "n1024", "n1025", "n%d" % N_BIG, "outside", "slab", "hidden"])
def test_tight_frame_is_slot_order_free(oracle, name):
    from gpu_checks import check_image
    from gsplat import _abi
    s, u, ref, cols, state = _case(oracle, name)
    n = s.shape[0]
    r = mk(s, W, H, TS, exact=True, cols=cols, state=state is not None)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    if state is not None:
        r.write_state(state)
    xy = lattice(W, H, 5, 13, 3, 17)
    dbg = _frame(r, u, xy, debug=True)
    r.set_option(_abi.GS_OPT_TILE_CULL, 0)
    rect = _frame(r, u, xy)
    r.set_option(_abi.GS_OPT_TILE_CULL, 1)
    tight = _frame(r, u, xy)
    assert rect["st"]["tight_binning"] == 0 and tight["st"]["tight_binning"] == 1
    if name == "outside":
        assert tight["st"]["num_visible"] == 0 and tight["vals"].size == 0 and not tight["rgba8"][..., :3].any()
    elif name != "hidden":
        assert tight["vals"].size > 0
    # the EXACT image: the same context's reference-binning frame, and the CPU oracle's
    np.testing.assert_array_equal(tight["rgba8"], rect["rgba8"])
    np.testing.assert_array_equal(tight["rgbf"], rect["rgbf"])
    check_image(r, ref, True)
    # ids, not slots: below n, and per tile a subsequence of the reference-binning frame's list
    assert (tight["vals"] < n).all()
    assert tight["ranges"].size == rect["ranges"].size
    t0 = r0 = 0
    for t1, r1 in zip(tight["ranges"].tolist(), rect["ranges"].tolist()):
        assert _subsequence(tight["vals"][t0:t1], rect["vals"][r0:r1]), "tile list is not a subsequence of the reference binning's"
        t0, r0 = t1, r1
    np.testing.assert_array_equal(tight["counts"], np.bincount(tight["vals"], minlength=n).astype(np.uint32))
    # the records of the listed gaussians: bit-equal rows of the debug frame's index-ordered array
    listed = np.unique(tight["vals"])
    np.testing.assert_array_equal(tight["gdata"][listed], dbg["gdata"][listed])
    assert not tight["gdata"][:, 2].any()  # the id word is cleared: padding in the reference's record
    if state is not None:
        assert not (state[tight["vals"]] & 1).any()
    # queries on the frame: picks (front, dominant, median and every other field but the length of the tile's list, which tight
    # binning shortens) and the coverage planes with their totals
    for f in tight["pick"].dtype.names:
        if f != "list_length":
            np.testing.assert_array_equal(tight["pick"][f], rect["pick"][f], err_msg="pick " + f)
    assert (tight["pick"]["list_length"] <= rect["pick"]["list_length"]).all()
    np.testing.assert_array_equal(tight["cover"], rect["cover"])
    for f in ("hits", "sum_q"):
        assert int(tight["cover"][f].astype(np.uint64).sum()) == int(rect["cover"][f].astype(np.uint64).sum())
    # a second tight frame hands the slots out in another order: the taps are the same
    again = _frame(r, u, xy)
    for k in ("rgba8", "rgbf", "vals", "ranges", "gdata", "counts", "pick", "cover"):
        np.testing.assert_array_equal(again[k], tight[k], err_msg=k)
    r.destroy()


def test_three_frames_in_flight_match_one_at_a_time():
    """GS_OPT_FRAMES_IN_FLIGHT 3: six frames of two alternating cameras, enqueued back to back with a copy of each image into its
    own page-locked sink, against the same cameras one frame at a time.  Each ring member has its own records."""
    from gsplat import _abi
    L = _abi.load()
    s = scene(N_BIG)
    us = [_orbit(2), _orbit(6)]
    seq = mk(s, W, H, TS)
    seq.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    want = []
    for u in us:
        seq.render_uniforms(u)
        seq.wait()
        assert seq.stats()["tight_binning"] == 1
        want.append(seq.read_rgba8())
    seq.destroy()
    assert (want[0] != want[1]).any()
    r = mk(s, W, H, TS)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 3)
    for k in range(3):  # opens the ring: every member sees a frame and grows to it
        r.render_uniforms(us[k % 2])
    r.wait()
    nbytes = W * H * 4
    sinks, tickets = [], []
    for k in range(6):
        p, t = ctypes.c_void_p(), ctypes.c_uint64()
        _abi.check(L.gs_host_alloc(nbytes, ctypes.byref(p)))
        sinks.append(p)
        uu = np.ascontiguousarray(us[k % 2], dtype=np.float32)
        _abi.check(L.gs_render_host(r._ctx, uu.ctypes.data, p, nbytes, ctypes.byref(t)))
        tickets.append(t.value)
    for k in range(6):
        _abi.check(L.gs_wait_ticket(r._ctx, tickets[k]))
        got = np.ctypeslib.as_array(ctypes.cast(sinks[k], ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,)).reshape(H, W, 4)
        np.testing.assert_array_equal(got, want[k % 2], err_msg="frame %d" % k)
    r.wait()
    st = r.stats()
    assert st["frames_in_flight"] == 3 and st["tight_binning"] == 1
    r.destroy()
    for p in sinks:
        L.gs_host_free(p)


def test_overflowed_frame_is_rendered_again_in_full():
    """80 000 thin splats as tall as the canvas: 16 row items each, 1.28 M arena slots against the 2^20 a scene of this size starts
    with, and max_intersections far below the instances.  gs_wait grows both and renders the frame again; the record cursors of
    the truncated attempt are gone with its control block.  The image equals the same frame rendered once more (nothing
    overflows any longer) and the reference binning's."""
    from gsplat import _abi
    k = 80000
    rng = np.random.default_rng(11)
    s = make_splats(W, H, rng.uniform(0, W, k), np.full(k, H / 2.0), 0.5, 300.0, 0.0, rng.uniform(-3.0, 0.0, k).astype(np.float32), rng=rng)
    u = pixel_uniforms(W, H)
    r = mk(s, W, H, TS, exact=True, max_intersections=4096)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    r.render_uniforms(u)
    r.wait()
    st = r.stats()
    assert st["tight_binning"] == 1 and st["num_row_slots"] > (1 << 20) and st["row_capacity"] >= st["num_row_slots"]
    assert st["num_intersections"] > 4096 and st["capacity"] >= st["num_intersections"]
    first = (r.read_rgba8(), r.read_buffer(_abi.GS_BUF_RGB_F32), r.read_buffer(_abi.GS_BUF_VALUES), r.read_buffer(_abi.GS_BUF_RANGES))
    assert first[0][..., :3].any() and (first[2] < k).all()
    r.render_uniforms(u)
    r.wait()
    assert r.stats()["row_capacity"] == st["row_capacity"] and r.stats()["capacity"] == st["capacity"]
    second = (r.read_rgba8(), r.read_buffer(_abi.GS_BUF_RGB_F32), r.read_buffer(_abi.GS_BUF_VALUES), r.read_buffer(_abi.GS_BUF_RANGES))
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)
    r.set_option(_abi.GS_OPT_TILE_CULL, 0)
    r.render_uniforms(u)
    r.wait()
    assert r.stats()["tight_binning"] == 0
    np.testing.assert_array_equal(r.read_rgba8(), first[0])
    np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_RGB_F32), first[1])
    r.destroy()
