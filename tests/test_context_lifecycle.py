"""One context through everything it owns, then destroyed -- three times in a row in one process.

Every device and pinned allocation, event and stream of a context is held by an owner (csrc/gs_runtime.h) and released by the
context's destructor or by the owner's reset().  This test walks ONE context through each of them: the arrays a regrow
replaces, both shadows of the ring, the unsorted copies of a debug frame, the rebuilt keys, a ticket's event, the pick
buffers, shadows destroyed while their owner lives, the scene and per-gaussian arrays a re-upload replaces -- and then renders a
frame that must still be the oracle's, byte for byte.  What is asserted: that image, every status code (a non-zero one raises
GsError) and the ring's size after each change of the ring.  Nothing about timing or free device memory: the card is shared.

The camera carries a scale modifier of 2: with it the tight binning of the 5 000 splats yields 5 402 instances (the host
restatement, tools/tight_check) and the reference's binning 8 492, so the first frame overflows the 4 096 the context is created
with and the debug frame overflows the 8 192 the first regrow leaves.
"""
import ctypes

import numpy as np
import pytest

from conftest import scene

W, H, TS = 256, 192, 16
N_FIRST, N_SECOND = 5000, 1300
_REF = {}


def _uniforms():
    from gpu_checks import orbit_uniforms
    u = np.array(orbit_uniforms(W, H), dtype=np.float32).copy()
    u[39] = np.float32(2.0)
    return u


def _refs(oracle):
    """The oracle's frames of both scenes, computed once and shared by the parametrisations."""
    if not _REF:
        u = _uniforms()
        for n in (N_FIRST, N_SECOND):
            _REF[n] = oracle.render(scene(n), u, W, H, TS)["rgba8"]
            _REF[n].setflags(write=False)
    return _REF


def _lifecycle(oracle, flags, graph):
    import gsplat
    from gsplat import _abi
    L = _abi.load()
    ref = _refs(oracle)
    u = _uniforms()
    r = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(scene(N_FIRST)), TS, flags=flags, max_intersections=4096)
    try:
        if graph:
            r.set_option(_abi.GS_OPT_FRAME_GRAPH, 1)
        # the first frame overflows the capacity: gs_wait regrows the (key,value) arrays and renders it again
        r.render_uniforms(u)
        r.wait()
        st = r.stats()
        assert st["capacity"] > 4096 and st["num_intersections"] > 4096
        assert st["frames_in_flight"] == 1
        np.testing.assert_array_equal(r.read_rgba8(), ref[N_FIRST])
        # three frames without a wait: the second and the third open a shadow each
        for _ in range(3):
            r.render_uniforms(u)
        r.wait()
        assert r.stats()["frames_in_flight"] == 3
        # a debug frame: the copies of the unsorted arrays (and, at the reference's instance count, another regrow)
        r.render_uniforms(u, debug=True)
        r.wait()
        assert r.read_buffer(_abi.GS_BUF_KEYS_UNSORTED).size == r.stats()["num_intersections"]
        # a tight frame holds no keys: reading them rebuilds them into a buffer of their own
        r.render_uniforms(u)
        r.wait()
        st = r.stats()
        assert st["tight_binning"] == 1
        assert r.read_buffer(_abi.GS_BUF_KEYS).size == st["num_intersections"]
        # a frame presented into a page-locked sink, its ticket waited for
        nbytes = W * H * 4
        sink, ticket = ctypes.c_void_p(), ctypes.c_uint64()
        _abi.check(L.gs_host_alloc(nbytes, ctypes.byref(sink)))
        try:
            _abi.check(L.gs_render_host(r._ctx, u.ctypes.data, sink, nbytes, ctypes.byref(ticket)))
            _abi.check(L.gs_wait_ticket(r._ctx, ticket.value))
            got = np.ctypeslib.as_array(ctypes.cast(sink, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,)).reshape(H, W, 4).copy()
            r.wait()
        finally:
            L.gs_host_free(sink)
        np.testing.assert_array_equal(got, ref[N_FIRST])
        # queries with contributor records
        res, con = r.pick(np.array([(W // 2, H // 2), (3, 5), (W - 1, H - 1)], np.uint32), max_contrib=4)
        assert (res["status"] == _abi.GS_PICK_OK).all() and con.shape == (3, 4)
        # the shadows go while their owner lives; its next frames run alone (with the frame graph: a capture, then a replay)
        r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
        for _ in range(2):
            r.render_uniforms(u)
        r.wait()
        st = r.stats()
        assert st["frames_in_flight"] == 1
        assert (st["graph_frames"] >= 2) if graph else (st["graph_frames"] == 0)
        np.testing.assert_array_equal(r.read_rgba8(), ref[N_FIRST])
        # a scene of another size: the resident scene, the per-gaussian arrays and the (key,value) arrays are all replaced
        s2 = np.ascontiguousarray(scene(N_SECOND), dtype=np.float32)
        _abi.check(L.gs_upload_splats(r._ctx, s2.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(N_SECOND)))
        r.render_uniforms(u)
        r.wait()
        st = r.stats()
        assert st["num_gaussians"] == N_SECOND and st["frames_in_flight"] == 1
        np.testing.assert_array_equal(r.read_rgba8(), ref[N_SECOND])
    finally:
        r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["timing", "graph"])
def test_context_lifecycle(oracle, variant):
    from gsplat import _abi
    if variant == "timing":  # per-stage events: 1 792 of them, and no frame graph (enqueue_frame issues such frames directly)
        flags, graph = _abi.GS_FLAG_TIMING | _abi.GS_FLAG_AUX_OUTPUTS | _abi.GS_FLAG_F32_TAP | _abi.GS_FLAG_EXACT_BLEND, False
    else:
        flags, graph = _abi.GS_FLAG_EXACT_BLEND | _abi.GS_FLAG_AUX_OUTPUTS, True
    for _ in range(3):
        _lifecycle(oracle, flags, graph)
