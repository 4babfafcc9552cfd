"""GS_FLAG_AUX_OUTPUTS: the per-pixel alpha plane A = 1 - T_final and accumulated-depth plane D = sum of cond z alpha T
(GS_BUF_ALPHA_F32 / GS_BUF_DEPTH_F32, include/gsplat/gs_abi.h).

The reference the GPU planes are held to is tests/aux_restate.py, a numpy restatement of the oracle's blend with the depth
term added; the CPU tests prove that its colour IS the oracle's, bit for bit, on the scenes used here.  EXACT frames must give
both planes bit-equal to it in every blend kernel and binning, fused frames must stay within the colour's envelope, and the
flag must change nothing else (image, f32 tap, evaluation count).
"""
import functools
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import scene
from support import (F, GOLDEN, NODE, SLAB_COLS, host_sources, make_splats, margin_ref, margin_scene, mk, oracle_frame, pixel_uniforms,
                     run_node)

_mk = functools.partial(mk, aux=True)

_CACHE = {}


def _restated(key, ref, W, H, ts, cols=None):
    from aux_restate import restate_ref
    k = ("restate", key, ts, cols)
    if k not in _CACHE:
        _CACHE[k] = restate_ref(ref, W, H, ts, cols)
    return _CACHE[k]


def _config_a(oracle, ts, want_illcond=False):
    from gpu_checks import orbit_uniforms
    s, u = scene(10000), orbit_uniforms(256, 256)
    return s, u, oracle_frame(oracle, "cfgA", s, u, 256, 256, ts, want_illcond=want_illcond)


def _ragged(oracle):
    """tests/golden/ragged_3001_200x120_t8.npz: the golden lists, and the oracle's GaussianData checked against the golden's hash."""
    from gsplat import synth
    if "ragged" not in _CACHE:
        z = np.load(os.path.join(GOLDEN, "ragged_3001_200x120_t8.npz"))
        n, W, H, ts, step = (int(v) for v in z["params"])
        s = synth.bicycle_like(n)
        u = z["uniforms"]
        gdata, _ = oracle.preprocess(s, u, W, H, ts)
        assert hashlib.sha256(np.ascontiguousarray(gdata).tobytes()).hexdigest() == str(z["gdata_sha256"])
        ref = {"gdata": gdata, "sorted_values": z["sorted_values"], "sorted_keys": z["sorted_keys"], "ranges": z["ranges"],
               "rgba8": z["rgba8"], "rgbf_sha256": str(z["rgbf_sha256"]), "num_intersections": int(z["num_intersections"]),
               "tile_counts": z["tile_counts"]}
        _CACHE["ragged"] = (s, u, W, H, ts, ref)
    return _CACHE["ragged"]


# ---- CPU: the restatement is the oracle's blend ---------------------------------------------------------------------------------
def _same_bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("ts", [16, 8])
def test_restatement_colour_is_the_oracle_config_a(oracle, ts):
    s, u, ref = _config_a(oracle, ts)
    rgbf, A, D = _restated("cfgA", ref, 256, 256, ts)
    _same_bits(rgbf, ref["rgbf"])
    assert A.max() > 0.9 and D.max() > 1.0  # the planes are not trivial on this scene


def test_restatement_colour_is_the_oracle_ragged_golden(oracle):
    s, u, W, H, ts, ref = _ragged(oracle)
    rgbf, A, D = _restated("ragged", ref, W, H, ts)
    blended = oracle.blend(ref["gdata"], ref["sorted_values"], ref["ranges"], W, H, ts, want_f32=True)
    _same_bits(rgbf, blended["rgbf"])
    assert hashlib.sha256(np.ascontiguousarray(rgbf).tobytes()).hexdigest() == ref["rgbf_sha256"]
    np.testing.assert_array_equal(blended["rgba8"], ref["rgba8"])


@pytest.mark.parametrize("name", ["transmittance_edge", "live_box", "degenerate_conic"])
def test_restatement_colour_is_the_oracle_margin_scenes(oracle, name):
    s, u, W, H = margin_scene(oracle, name)
    for ts, cols in ((8, None), (16, SLAB_COLS[16])):
        ref = margin_ref(oracle, name, ts, cols)
        rgbf, A, D = _restated(name, ref, W, H, ts, cols)
        _same_bits(rgbf, ref["rgbf"])


def test_abi_constants_agree_across_hosts():
    rjs, idx, dts, napi, hdr = host_sources()
    assert int(re.search(r"#define GS_FLAG_AUX_OUTPUTS (0x[0-9a-fA-F]+)u", hdr).group(1), 16) == 0x8
    assert int(re.search(r"GS_BUF_ALPHA_F32 = (\d+)", hdr).group(1)) == 13
    assert int(re.search(r"GS_BUF_DEPTH_F32 = (\d+)", hdr).group(1)) == 14
    assert re.search(r"#define GS_ABI_VERSION 3\b", hdr)
    from gsplat import _abi
    assert (_abi.GS_FLAG_AUX_OUTPUTS, _abi.GS_BUF_ALPHA_F32, _abi.GS_BUF_DEPTH_F32) == (0x8, 13, 14)
    # no id collides with an existing flag bit / tap
    assert _abi.GS_FLAG_AUX_OUTPUTS & (_abi.GS_FLAG_EXACT_BLEND | _abi.GS_FLAG_F32_TAP | _abi.GS_FLAG_TIMING) == 0
    assert re.search(r"ALPHA_F32: 13\b", dts) and re.search(r"DEPTH_F32: 14\b", dts) and re.search(r"AUX_OUTPUTS: 0x8\b", dts)
    assert "readAlpha(): Float32Array" in dts and "readDepth(normalized?: boolean): Float32Array" in dts
    assert re.search(r"ALPHA_F32: 13\b", idx) and re.search(r"DEPTH_F32: 14\b", idx) and re.search(r"AUX_OUTPUTS: 0x8\b", idx)
    for name in ("FLAG_AUX_OUTPUTS", "BUF_ALPHA_F32", "BUF_DEPTH_F32"):
        assert '"%s", GS_%s' % (name, name) in napi


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _frame(r, u, debug=False):
    r.render_uniforms(u, debug=debug)
    r.wait()
    return r.read_alpha().copy(), r.read_depth().copy()


def _check_planes_exact(r, A, D, restated, cell):
    _, Aref, Dref = restated
    x0, w = r.slab_x0, r.slab_width
    np.testing.assert_array_equal(A.view(np.uint32), Aref[:, x0:x0 + w].view(np.uint32), err_msg="alpha " + str(cell))
    np.testing.assert_array_equal(D.view(np.uint32), Dref[:, x0:x0 + w].view(np.uint32), err_msg="depth " + str(cell))


def _check_planes_fused(A, D, restated, ill, zmax, cell, max_ill=0.005):
    _, Aref, Dref = restated
    dA, dD = np.abs(A - Aref), np.abs(D - Dref)
    tolD = 1e-4 * np.maximum(F(1.0), np.abs(Dref))
    assert dA[~ill].max(initial=0.0) <= 1e-4, (cell, float(dA[~ill].max()))
    assert (dD[~ill] <= tolD[~ill]).all(), (cell, float((dD / tolD)[~ill].max()))
    assert ill.mean() <= max_ill, (cell, float(ill.mean()))
    assert dA.max(initial=0.0) <= 4e-3 and dD.max(initial=0.0) <= 4e-3 * zmax, (cell, float(dA.max()), float(dD.max()))


KERNELS = [(16, 0), (16, 8), (16, 4), (32, 0), (32, 8), (8, 0), (8, 4)]  # (tile, GS_OPT_BLEND_ABLATION): quad, workgroup-per-
KERNEL_IDS = ["quad16", "wg16", "quad16-noculls", "quad32", "wg32", "tile8", "tile8-noculls"]  # tile, culls off


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_exact_planes_bit_equal_config_a(oracle, kernel):
    """EXACT: alpha and depth bit-equal to the restatement in every blend kernel, with tight binning (gs_render), the reference's
    binning (GS_OPT_TILE_CULL 0) and gs_render_debug; the colour stays bit-equal to the oracle."""
    from gsplat import _abi
    from gpu_checks import check_image
    ts, abl = kernel
    s, u, ref = _config_a(oracle, ts)
    restated = _restated("cfgA", ref, 256, 256, ts)
    r = _mk(s, 256, 256, ts, exact=True)
    r.set_option(_abi.GS_OPT_BLEND_ABLATION, abl)
    for tight, debug in ((1, False), (0, False), (0, True)):
        r.set_option(_abi.GS_OPT_TILE_CULL, tight)
        A, D = _frame(r, u, debug)
        assert r.stats()["tight_binning"] == (tight and not debug)
        _check_planes_exact(r, A, D, restated, (ts, abl, tight, debug))
        check_image(r, ref, True)
        assert (r.read_rgba8()[..., 3] == 255).all()
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("abl", [0, 4])
def test_exact_planes_bit_equal_ragged_golden(oracle, abl):
    from gsplat import _abi
    s, u, W, H, ts, ref = _ragged(oracle)
    restated = _restated("ragged", ref, W, H, ts)
    r = _mk(s, W, H, ts, exact=True)
    r.set_option(_abi.GS_OPT_BLEND_ABLATION, abl)
    for debug in (False, True):
        A, D = _frame(r, u, debug)
        _check_planes_exact(r, A, D, restated, ("ragged", abl, debug))
        np.testing.assert_array_equal(r.read_rgba8(), ref["rgba8"])
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [(16, 0), (32, 0), (16, 8), (32, 8), (8, 0)], ids=["quad16", "quad32", "wg16", "wg32", "tile8"])
@pytest.mark.parametrize("name", ["transmittance_edge", "live_box", "degenerate_conic"])
def test_planes_at_the_cull_margins(oracle, name, kernel):
    """The scenes of test_blend_culls.py (decisions at the margins of both parking culls, ragged canvases): the planes with the culls
    on equal those with the culls off bit for bit, in every kernel, binning and mode, on the whole canvas and on a tile-column slab
    that does not start at column 0; EXACT planes equal the restatement."""
    from gsplat import _abi
    ts, abl = kernel
    s, u, W, H = margin_scene(oracle, name)
    for cols in (None, SLAB_COLS[ts]):
        ref = margin_ref(oracle, name, ts, cols)
        restated = _restated(name, ref, W, H, ts, cols)
        for exact in (True, False):
            r = _mk(s, W, H, ts, exact=exact, cols=cols)
            for tight, debug in ((1, False), (0, False), (0, True)):
                r.set_option(_abi.GS_OPT_TILE_CULL, tight)
                r.set_option(_abi.GS_OPT_BLEND_ABLATION, abl | 4)
                A_off, D_off = _frame(r, u, debug)
                r.set_option(_abi.GS_OPT_BLEND_ABLATION, abl)
                A_on, D_on = _frame(r, u, debug)
                cell = (name, ts, abl, cols, exact, tight, debug)
                np.testing.assert_array_equal(A_on.view(np.uint32), A_off.view(np.uint32), err_msg=str(cell))
                np.testing.assert_array_equal(D_on.view(np.uint32), D_off.view(np.uint32), err_msg=str(cell))
                if exact:
                    _check_planes_exact(r, A_on, D_on, restated, cell)
            r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [(16, 0), (32, 0), (16, 8), (8, 0)], ids=["quad16", "quad32", "wg16", "tile8"])
def test_fused_planes_within_the_envelope(oracle, kernel):
    """Fused mode: |dA| <= 1e-4 and |dD| <= 1e-4 max(1, D) on the pixels the oracle does not flag; flagged pixels (a keep/skip
    decision within rounding of its threshold) within 4e-3 (depth: 4e-3 x the largest z), and at most 0.5 % of them."""
    from gsplat import _abi
    ts, abl = kernel
    s, u, ref = _config_a(oracle, ts, want_illcond=True)
    restated = _restated("cfgA", ref, 256, 256, ts)
    ill = ref["illcond"].astype(bool)
    zmax = float(np.nanmax(ref["gdata"].view(np.float32).reshape(-1, 16)[:, 7]))
    r = _mk(s, 256, 256, ts, exact=False)
    r.set_option(_abi.GS_OPT_BLEND_ABLATION, abl)
    for debug in (False, True):
        A, D = _frame(r, u, debug)
        _check_planes_fused(A, D, restated, ill, zmax, (ts, abl, debug))
    r.destroy()


def _outputs(r, u):
    from gsplat import _abi
    r.render_uniforms(u)
    r.wait()
    return r.read_rgba8(), r.read_buffer(_abi.GS_BUF_RGB_F32, np.float32), r.stats()["num_evaluated"]


@pytest.mark.gpu
@pytest.mark.parametrize("ts", [16, 8])
def test_flag_changes_nothing_else_config_a(oracle, ts):
    s, u, ref = _config_a(oracle, ts)
    for exact in (True, False):
        base = _mk(s, 256, 256, ts, exact=exact, aux=False)
        aux = _mk(s, 256, 256, ts, exact=exact, aux=True)
        i0, f0, e0 = _outputs(base, u)
        i1, f1, e1 = _outputs(aux, u)
        np.testing.assert_array_equal(i0, i1)
        np.testing.assert_array_equal(f0.view(np.uint32), f1.view(np.uint32))
        assert e0 == e1 > 0
        base.destroy()
        aux.destroy()


@pytest.mark.gpu
def test_flag_changes_nothing_else_config_b():
    """One 6.1 M-splat 1080p frame (the generator bench.py uses): rgba8, the f32 tap and the evaluation count identical with and
    without the flag in both modes; the fused planes within the fused envelope of the EXACT ones (no oracle at this size)."""
    import torch
    import gsplat
    from gsplat import synth
    from gpu_checks import orbit_uniforms
    n, W, H, ts = 6_100_000, 1920, 1080, 16
    dev = synth.bicycle_like_torch(n, synth.BASE_SEED + 1, "cuda")
    torch.cuda.synchronize()
    pg = gsplat.PackedGaussians.__new__(gsplat.PackedGaussians)
    pg.numGaussians, pg.gaussiansBuffer, pg.sphericalHarmonicsDegree = n, dev, 3
    u = orbit_uniforms(W, H, step=0)
    planes = {}
    for exact in (True, False):
        base = _mk(pg, W, H, ts, exact=exact, aux=False)
        _outputs(base, u)  # the first frame grows the capacity
        i0, f0, e0 = _outputs(base, u)
        base.destroy()
        aux = _mk(pg, W, H, ts, exact=exact, aux=True)
        _outputs(aux, u)
        i1, f1, e1 = _outputs(aux, u)
        np.testing.assert_array_equal(i0, i1)
        np.testing.assert_array_equal(f0.view(np.uint32), f1.view(np.uint32))
        assert e0 == e1 > 0
        planes[exact] = (aux.read_alpha().copy(), aux.read_depth().copy())
        aux.destroy()
    del dev
    (Ae, De), (Af, Df) = planes[True], planes[False]
    assert Ae.max() > 0.9
    dA, dD = np.abs(Af - Ae), np.abs(Df - De)
    zmax = float(De.max() / max(float(Ae.max()), 1e-6)) * 4.0 + 1.0  # (no GaussianData here: a generous stand-in for the largest z)
    # the fused frame's flagged share of pixels is below 0.5 % at this configuration (test_gpu_scale): the same budget here
    assert (dA > 1e-4).mean() <= 0.005 and (dD > 1e-4 * np.maximum(1.0, De)).mean() <= 0.005, (float((dA > 1e-4).mean()))
    assert dA.max() <= 4e-3 and dD.max() <= 4e-3 * zmax, (float(dA.max()), float(dD.max()))


def _pixel_scene(W, H, px, py, z, sig, logit, color):
    """Records in pixel space (identity view and projection; the centre (px, py) in pixels at depth z)."""
    s = make_splats(W, H, px, py, sig, sig, 0.0, np.asarray(logit, np.float32), color=color)
    s[:, 2] = z  # (the projected size scales with 1 / z)
    return s, pixel_uniforms(W, H)


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False])
def test_analytic_planes(oracle, exact):
    W = H = 64
    z0 = 3.25
    s, u = _pixel_scene(W, H, [32.0], [32.0], [z0], [6.0], [2.0], [[0.3, 0.2, 0.1]])
    g = oracle.preprocess(s, u, W, H, 16)[0].view(np.float32).reshape(-1, 16)
    assert g[0, 7] == F(z0)
    r = _mk(s, W, H, 16, exact=exact)
    A, D = _frame(r, u)
    Dn = r.read_depth(normalized=True)
    assert A[32, 32] > 0.5
    rel = 1e-6 if exact else 1e-4
    assert abs(float(D[32, 32] / A[32, 32]) - z0) <= rel * z0 and abs(float(Dn[32, 32]) - z0) <= rel * z0
    reached = A > 0
    assert not reached[0, 0] and not reached[63, 63]
    assert (A[~reached] == 0).all() and (D[~reached] == 0).all() and (Dn[~reached] == 0).all()
    assert (D[reached] > 0).all()
    r.destroy()
    # a near-opaque splat in front of a second one: the normalised depth is the front one's
    zf, zb = 2.0, 5.0
    s, u = _pixel_scene(W, H, [32.0, 30.0], [32.0, 33.0], [zf, zb], [12.0, 12.0], [8.0, 8.0], [[0.5, 0.5, 0.5], [0.1, 0.9, 0.1]])
    r = _mk(s, W, H, 16, exact=exact)
    r.render_uniforms(u)
    r.wait()
    Dn = r.read_depth(normalized=True)
    assert abs(float(Dn[32, 32]) - zf) <= 2e-2 * zf, float(Dn[32, 32])
    r.destroy()


def _direct(s, W, H, ts, u, cols=None):
    """A single context, one frame in flight: the planes every other path must reproduce."""
    from gsplat import _abi
    r = _mk(s, W, H, ts, exact=True, cols=cols)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    A, D = _frame(r, u)
    img = r.read_rgba8()
    r.destroy()
    return A, D, img


def _eq(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32), err_msg=msg)


@pytest.mark.gpu
def test_planes_on_every_path(oracle):
    import torch
    from gsplat import _abi, synth
    import gsplat
    W, H, ts = 256, 256, 16
    s = scene(10000)
    us = [synth.orbit_camera(k, W, H).uniforms(W, H) for k in (1, 4, 7)]
    direct = [_direct(s, W, H, ts, u) for u in us]
    assert not np.array_equal(direct[0][1], direct[2][1])  # the cameras differ in depth
    # three frames enqueued before one gs_wait: the ring of shadows (each owns its planes); the taps describe the last frame
    r = _mk(s, W, H, ts, exact=True)
    for u in us:
        r.render_uniforms(u)
    r.wait()
    assert r.stats()["frames_in_flight"] == 3
    _eq(r.read_alpha(), direct[2][0], "frames in flight: alpha")
    _eq(r.read_depth(), direct[2][1], "frames in flight: depth")
    r.destroy()
    # the frame graph: captured once, replayed; the planes follow the camera
    r = _mk(s, W, H, ts, exact=True)
    r.set_option(_abi.GS_OPT_FRAME_GRAPH, 1)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    for k, u in enumerate(us):
        A, D = _frame(r, u)
        _eq(A, direct[k][0], "graph frame %d: alpha" % k)
        _eq(D, direct[k][1], "graph frame %d: depth" % k)
    assert r.stats()["graph_frames"] >= 2
    r.destroy()
    # two tile-column slabs: their planes are the matching columns of the whole canvas's
    ntx = W // ts
    for cols in ((0, 5), (5, ntx)):
        A, D, _ = _direct(s, W, H, ts, us[1], cols=cols)
        x0, x1 = cols[0] * ts, min(W, cols[1] * ts)
        _eq(A, direct[1][0][:, x0:x1], "slab %s: alpha" % (cols,))
        _eq(D, direct[1][1][:, x0:x1], "slab %s: depth" % (cols,))
    # gs_render_to: rgba8 to the caller's device memory, the planes to the context's own
    r = _mk(s, W, H, ts, exact=True)
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.render_uniforms(us[0], out_ptr=out.data_ptr())
    r.wait()
    np.testing.assert_array_equal(out.cpu().numpy(), direct[0][2])
    _eq(r.read_alpha(), direct[0][0], "gs_render_to: alpha")
    _eq(r.read_depth(), direct[0][1], "gs_render_to: depth")
    r.destroy()
    # PipelinedRenderer: per-slot planes
    p = gsplat.PipelinedRenderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(s), ts, frames_in_flight=2,
                                 flags=_abi.GS_FLAG_EXACT_BLEND | _abi.GS_FLAG_AUX_OUTPUTS)
    slots = [p.render_uniforms(u) for u in us[:2]]
    for k, slot in enumerate(slots):
        _eq(p.read_alpha(slot), direct[k][0], "pipelined slot %d: alpha" % slot)
        _eq(p.read_depth(slot), direct[k][1], "pipelined slot %d: depth" % slot)
    nd = p.read_depth(slots[1], normalized=True)
    a = direct[1][0]
    want = np.zeros_like(a)
    np.divide(direct[1][1], a, out=want, where=a > 0)
    _eq(nd, want, "normalized depth")
    p.destroy()


@pytest.mark.gpu
def test_plane_taps_errors(oracle):
    from gsplat import _abi
    s = scene(2000)
    from gpu_checks import orbit_uniforms
    u = orbit_uniforms(128, 96)
    r = _mk(s, 128, 96, 16, exact=True, aux=True)
    for which in (_abi.GS_BUF_ALPHA_F32, _abi.GS_BUF_DEPTH_F32):
        with pytest.raises(_abi.GsError) as e:
            r.read_buffer(which, np.float32)
        assert e.value.code == -6  # GS_ERR_NO_FRAME
        with pytest.raises(_abi.GsError) as e:
            r.device_ptr(which)
        assert e.value.code == -6
    r.render_uniforms(u)
    r.wait()
    assert r.read_alpha().shape == (96, 128) and r.device_ptr(_abi.GS_BUF_DEPTH_F32)
    r.destroy()
    r = _mk(s, 128, 96, 16, exact=True, aux=False)
    r.render_uniforms(u)
    r.wait()
    for which in (_abi.GS_BUF_ALPHA_F32, _abi.GS_BUF_DEPTH_F32):
        with pytest.raises(_abi.GsError) as e:
            r.read_buffer(which, np.float32)
        assert e.value.code == -1 and "GS_FLAG_AUX_OUTPUTS" in str(e.value)
        with pytest.raises(_abi.GsError) as e:
            r.device_ptr(which)
        assert e.value.code == -1 and "GS_FLAG_AUX_OUTPUTS" in str(e.value)
    r.destroy()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_node_host_planes_match_python(tmp_path):
    from gsplat import _abi, synth
    n, W, H, ts = 8000, 200, 120, 16
    s = scene(n)
    u = synth.orbit_camera(4, W, H).uniforms(W, H)
    rec, ub, out = str(tmp_path / "rec.bin"), str(tmp_path / "u.bin"), str(tmp_path / "planes.bin")
    s.tofile(rec)
    u.tofile(ub)
    info = run_node("aux_check.js", (rec, n, W, H, ts, ub, out))
    assert info["n"] == W * H
    planes = np.fromfile(out, dtype=np.float32).reshape(3, H, W)
    r = _mk(s, W, H, ts, exact=True)
    A, D = _frame(r, u)
    Dn = r.read_depth(normalized=True)
    r.destroy()
    _eq(planes[0], A, "node alpha")
    _eq(planes[1], D, "node depth")
    _eq(planes[2], Dn, "node normalized depth")
