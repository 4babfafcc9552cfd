"""The Node host (gaussian-splatting-wgpu_amd/js + the N-API addon): Camera / PackedGaussians parity
with the Python mirror on CPU, and an end-to-end Renderer.animate() frame on the GPU."""
import json
import struct

import numpy as np
import pytest

from conftest import scene
from support import NODE, run_node

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


def _node(*args):
    return run_node("host_check.js", args)


def test_camera_matches_python_mirror():
    from gsplat.camera import Camera
    th = 0.4
    raw = {"id": 0, "img_name": "x", "width": 800, "height": 800, "fx": 800, "fy": 800, "position": [0.3, -1.0, 2.0],
           "rotation": [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]}
    js = _node("camera", json.dumps(raw))
    c = Camera.default()
    np.testing.assert_allclose(js["default"]["uniforms"], c.uniforms(800, 800), rtol=2e-6, atol=2e-6)
    np.testing.assert_array_equal(np.float32(js["default"]["view"]), c.viewMatrix)
    # the key sequence of host_check.js: w d q (translate) then j i u (rotate), applied in one getCamera()
    c.translate(0.1, -0.1, 0.1)
    c.rotate(0.1, 0.1, 0.1)
    np.testing.assert_allclose(js["moved"]["uniforms"], c.uniforms(640, 480), rtol=1e-5, atol=1e-5)
    assert js["dirtyAfter"] is False
    cj = Camera.from_json(raw)
    np.testing.assert_allclose(js["fromJSON"]["uniforms"], cj.uniforms(800, 800), rtol=1e-5, atol=1e-5)


def _write_ply(path, n, degree, with_uchar=False, seed=0):
    rng = np.random.default_rng(seed)
    nrest = 3 * ((degree + 1) ** 2 - 1)
    props = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + ["f_rest_%d" % i for i in range(nrest)] + \
            ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    for p in props:
        header += "property float %s\n" % p
    if with_uchar:
        header += "property uchar red\n"
    header += "end_header\n"
    data = rng.standard_normal((n, len(props))).astype(np.float32)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        for i in range(n):
            f.write(data[i].tobytes())
            if with_uchar:
                f.write(struct.pack("B", i % 256))
    return props, data


@pytest.mark.parametrize("degree,uchar", [(3, False), (3, True), (1, False), (0, False)])
def test_ply_loader_packs_reference_layout(tmp_path, degree, uchar):
    """ply.ts:162-228: record = pos@0, log_scale@16, rot@32, opacity@48, sh@64 (16 B per coefficient),
    SH order f_dc then f_rest_{rgb*K+i}; lower degrees zero-padded to 16 coefficients."""
    n = 37
    ply = str(tmp_path / "pc.ply")
    props, data = _write_ply(ply, n, degree, uchar, seed=degree)
    out = str(tmp_path / "rec.bin")
    info = _node("ply", ply, out)
    assert info["n"] == n and info["degree"] == degree and info["size"] == n * 320
    rec = np.fromfile(out, dtype=np.float32).reshape(n, 80)
    col = {p: data[:, i] for i, p in enumerate(props)}
    np.testing.assert_array_equal(rec[:, 0:3], np.stack([col["x"], col["y"], col["z"]], 1))
    np.testing.assert_array_equal(rec[:, 4:7], np.stack([col["scale_0"], col["scale_1"], col["scale_2"]], 1))
    np.testing.assert_array_equal(rec[:, 8:12], np.stack([col["rot_%d" % i] for i in range(4)], 1))
    np.testing.assert_array_equal(rec[:, 12], col["opacity"])
    K = (degree + 1) ** 2 - 1
    for c in range(3):
        np.testing.assert_array_equal(rec[:, 16 + c], col["f_dc_%d" % c])
        for i in range(K):
            np.testing.assert_array_equal(rec[:, 16 + 4 * (i + 1) + c], col["f_rest_%d" % (c * K + i)])
    assert not rec[:, 16 + 4 * (K + 1):].any() and not rec[:, 3].any() and not rec[:, 13:16].any()
    # the native loader (C ABI gs_ply_load), directly and through N-API, packs the same bytes
    from gsplat import _abi
    nat, deg = _abi.load_ply(ply)
    assert deg == degree
    np.testing.assert_array_equal(nat.view(np.uint32), rec.view(np.uint32))
    out2 = str(tmp_path / "rec2.bin")
    info2 = _node("plynative", ply, out2)
    assert info2["n"] == n and info2["degree"] == degree
    np.testing.assert_array_equal(np.fromfile(out2, dtype=np.uint32), rec.view(np.uint32).reshape(-1))


def test_native_ply_loader_errors(tmp_path):
    from gsplat import _abi
    with pytest.raises(_abi.GsError):
        _abi.load_ply(str(tmp_path / "missing.ply"))
    bad = tmp_path / "bad.ply"
    bad.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\n")
    with pytest.raises(_abi.GsError):
        _abi.load_ply(str(bad))  # no end_header
    props, _ = _write_ply(str(tmp_path / "d3.ply"), 4, 3)
    raw = (tmp_path / "d3.ply").read_bytes()
    (tmp_path / "trunc.ply").write_bytes(raw[:-10])
    with pytest.raises(_abi.GsError):
        _abi.load_ply(str(tmp_path / "trunc.ply"))


@pytest.mark.gpu
def test_renderer_animate_end_to_end(tmp_path, oracle):
    """new Renderer(canvas, interactiveCamera, device, gaussians, tileSize) -> animate() -> frame sink,
    through N-API, bit-equal to the oracle (exact-blend flag)."""
    from gsplat import synth
    n, W, H, ts = 8000, 256, 160, 16
    s = scene(n)
    u = synth.orbit_camera(4, W, H).uniforms(W, H)
    rec, ub, out = str(tmp_path / "rec.bin"), str(tmp_path / "u.bin"), str(tmp_path / "out.rgba")
    s.tofile(rec)
    u.tofile(ub)
    info = _node("render", rec, n, W, H, ts, ub, out)
    ref = oracle.render(s, u, W, H, ts)
    # the product path bins tightly: its instance list is a subset of the reference's (tests/gpu_checks.py proves which)
    assert info["frames"] == 1 and 0 < info["numIntersections"] <= ref["num_intersections"]
    assert info["nkeys"] == info["numIntersections"] and info["key0"] in set(int(k) for k in ref["sorted_keys"][:4096])
    img = np.fromfile(out, dtype=np.uint8).reshape(H, W, 4)
    np.testing.assert_array_equal(img, ref["rgba8"])


@pytest.mark.gpu
def test_renderer_pipelined_animate_delivers_every_frame_in_order(tmp_path):
    """canvas.pipeline = 3 (extension of the reference's class surface): six animate() calls without awaiting in between; every
    frame arrives once, in order, in a page-locked sink, equal to the synchronous render of its camera (N-API renderToSink /
    hostAlloc over gs_render_host / gs_wait_ticket / gs_host_alloc)."""
    from gsplat import synth
    n, W, H, ts, K = 8000, 256, 160, 16, 6
    s = scene(n)
    us = np.stack([synth.orbit_camera(3 * k, W, H).uniforms(W, H) for k in range(K)]).astype(np.float32)
    rec, ub = str(tmp_path / "rec.bin"), str(tmp_path / "u.bin")
    s.tofile(rec)
    us.tofile(ub)
    info = _node("pipeline", rec, n, W, H, ts, ub, K)
    assert info["same"] and info["delivered"] == K and info["frames"] >= K


@pytest.mark.gpu
def test_renderer_shares_splats(tmp_path):
    """device.shareWith: a second Renderer borrows the first one's resident splats (gs_share_splats) and draws the same frame."""
    from gsplat import synth
    n, W, H, ts = 6000, 192, 128, 16
    s = scene(n)
    u = synth.orbit_camera(9, W, H).uniforms(W, H)
    rec, ub = str(tmp_path / "rec.bin"), str(tmp_path / "u.bin")
    s.tofile(rec)
    u.tofile(ub)
    info = _node("shared", rec, n, W, H, ts, ub)
    assert info["same"] and info["bytes"] == W * H * 4


def test_write_ppm_presentation_sink(tmp_path):
    """js/index.js::writePPM -- binary P6, rgb of every pixel in row-major order, alpha dropped."""
    W, H = 37, 11
    out = tmp_path / "f.ppm"
    _node("ppm", out, W, H)
    raw = out.read_bytes()
    head = b"P6\n%d %d\n255\n" % (W, H)
    assert raw.startswith(head) and len(raw) == len(head) + W * H * 3
    i = np.arange(W * H)
    want = np.stack([i & 255, (i >> 3) & 255, (7 * i) & 255], axis=1).astype(np.uint8)
    np.testing.assert_array_equal(np.frombuffer(raw[len(head):], dtype=np.uint8).reshape(-1, 3), want)


def test_load_camera_file_matches_python_mirror(tmp_path):
    """camera.ts:323-340,344-400: a 3DGS cameras.json -> list of (img_name, Camera); checked against gsplat.camera.Camera.from_json."""
    from gsplat.camera import Camera
    cams = []
    for k, th in enumerate((0.0, 0.7, -1.9)):
        c, s_ = float(np.cos(th)), float(np.sin(th))
        cams.append({"id": k, "img_name": "img_%03d" % k, "width": 1957, "height": 1091, "fx": 1100.0 + k, "fy": 1090.0 - k,
                     "position": [0.5 * k, -1.0, 2.0 + k], "rotation": [[c, 0.0, s_], [0.0, 1.0, 0.0], [-s_, 0.0, c]]})
    path = tmp_path / "cameras.json"
    path.write_text(json.dumps(cams))
    js = _node("camfile", path)
    assert [e["name"] for e in js] == [c["img_name"] for c in cams]
    for e, raw in zip(js, cams):
        ref = Camera.from_json(raw)
        np.testing.assert_allclose(e["cam"]["uniforms"], ref.uniforms(800, 800), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(e["cam"]["view"], ref.viewMatrix, rtol=1e-6, atol=1e-6)


@pytest.mark.gpu
def test_native_handle_refuses_calls_while_a_frame_is_in_flight(tmp_path):
    """gs_ctx is not re-entrant: while renderAsync's worker owns it every other call on the handle throws, destroy() is deferred
    to the frame's completion (no use-after-free), and a negative splat count is rejected."""
    from gsplat import synth
    n, W, H = 200000, 1280, 720
    s = scene(n)
    u = synth.orbit_camera(2, W, H).uniforms(W, H)
    rec, ub = str(tmp_path / "rec.bin"), str(tmp_path / "u.bin")
    s.tofile(rec)
    u.tofile(ub)
    info = _node("busy", rec, n, W, H, ub)
    assert info["refused"] == 3 and info["gone"] and info["badN"]
