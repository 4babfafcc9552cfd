"""The N-API addon's own surface (csrc/napi/gs_napi.c through js.loadNative()): what it exports, what every export does with a
missing context or a wrong argument, and what a handle does with renderToSink frames in flight.  The addon loads without a GPU;
the expectations below were recorded on the shim as it was before its wrappers were rewritten over shared readers."""
import os

import numpy as np
import pytest

from conftest import scene
from support import NODE, ROOT, c_layout, run_node

ADDON = os.path.join(ROOT, "gaussian-splatting-wgpu_amd", "lib", "gsplat_napi.node")
pytestmark = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")

FUNCTIONS = {
    "create", "destroy", "uploadSplats", "renderSync", "renderAsync", "readRgba8", "readBuffer", "stats", "slab", "loadPly", "shareSplats",
    "uploadPly", "hostAlloc", "renderToSink", "pick", "stateRegion", "stateIds", "stateCount", "readState", "writeState", "setOption",
    "listState", "exportSplats", "compact", "exportPly", "savePly", "composeTransform", "transformSplats", "accumulateCoverage",
    "resetCoverage", "readCoverage", "stateCoverage", "attrSummary", "attrHistogram", "attrValues", "stateAttr", "neighCount", "neighRead",
    "stateNeigh"}
NO_CONTEXT = {"create", "destroy", "loadPly", "hostAlloc", "savePly", "composeTransform"}
# constant -> the C expression of gs_abi.h it equals
CONSTANTS = {
    "abiVersion": "GS_ABI_VERSION", "FLAG_EXACT_BLEND": "GS_FLAG_EXACT_BLEND", "FLAG_F32_TAP": "GS_FLAG_F32_TAP", "FLAG_TIMING": "GS_FLAG_TIMING",
    "FLAG_AUX_OUTPUTS": "GS_FLAG_AUX_OUTPUTS", "FLAG_SPLAT_STATE": "GS_FLAG_SPLAT_STATE", "BUF_SPLAT_STATE": "GS_BUF_SPLAT_STATE",
    "OPT_SELECT_TINT": "GS_OPT_SELECT_TINT", "BUF_ALPHA_F32": "GS_BUF_ALPHA_F32", "BUF_DEPTH_F32": "GS_BUF_DEPTH_F32", "PICK_OK": "GS_PICK_OK",
    "PICK_OUTSIDE_SLAB": "GS_PICK_OUTSIDE_SLAB", "PICK_NONE": "GS_PICK_NONE", "PICK_MAX_QUERIES": "GS_PICK_MAX_QUERIES",
    "PICK_MAX_CONTRIB": "GS_PICK_MAX_CONTRIB", "COVERAGE_REC_BYTES": "sizeof(gs_coverage_rec)", "ATTR_COUNT": "GS_ATTR_COUNT"}
NO_HANDLE = ["TypeError", "gsplat: expected a context handle", None]


def _node(*args):
    return run_node("surface_check.js", args)


def test_export_set_and_constants(tmp_path):
    from gsplat import _abi
    got = _node("surface")
    assert len(FUNCTIONS) == 39 and len(CONSTANTS) == 17
    assert sorted(got["functions"]) == sorted(FUNCTIONS)
    assert sorted(got["constants"]) == sorted(CONSTANTS)
    names = sorted(CONSTANTS)
    values = c_layout(tmp_path, "napi_constants", "".join('printf("%%llu\\n", (unsigned long long)(%s));' % CONSTANTS[k] for k in names))
    assert {k: got["constants"][k] for k in names} == dict(zip(names, values))
    assert got["constants"]["abiVersion"] == _abi.load().gs_abi_version()


def test_calls_that_need_no_context(tmp_path):
    from gsplat import _abi
    rec = np.ascontiguousarray(scene(64)[:3])
    src, ply, out = str(tmp_path / "rec.bin"), str(tmp_path / "three.ply"), str(tmp_path / "back.bin")
    rec.tofile(src)
    got = _node("nocontext", src, ply, out)
    assert got["createEmpty"] == ["TypeError", "gsplat.create: {width, height} required", None]
    assert len(got["xform"]) == 408 and bytes(got["xform"]) == bytes(_abi.compose_xform())
    cls, msg, code = got["zeroQuat"]
    assert cls == "Error" and code == "-1" and msg.startswith("gsplat: ")
    assert got["saved"] and got["loaded"] == {"n": 3, "degree": 3, "keys": ["degree", "n", "records"], "bytes": 3 * 320}
    back = np.fromfile(out, dtype=np.uint32)
    np.testing.assert_array_equal(back, rec.view(np.uint32).reshape(-1))
    nat, deg = _abi.load_ply(ply)
    assert deg == 3
    np.testing.assert_array_equal(back, nat.view(np.uint32).reshape(-1))
    cls, msg, code = got["hostAlloc0"]
    assert cls == "TypeError" and msg == "gsplat.hostAlloc: byte count required"


def test_create_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present: create succeeds")
    cls, msg, code = _node("nodevice")["create"]
    assert cls == "Error" and code == "-2" and msg.startswith("gsplat: ")


def test_every_context_call_refuses_a_non_handle():
    got = _node("nohandle")
    assert got["destroy"] is True
    assert set(got["calls"]) == FUNCTIONS - NO_CONTEXT
    assert {k: v for k, v in got["calls"].items() if v != NO_HANDLE} == {}


# ---- misuse on a live handle: (export, argument position) -> what the call throws, in the order of surface_check.js's table -----------
GENERIC = ("Error", None)  # a failed N-API read without a message of the wrapper's own: "N-API call failed: ..."


def _each(fn, positions, want):
    return [(fn, k, want) for k in positions]


def _T(msg):
    return ("TypeError", msg)


ATTR_MSG = _T("gsplat: an attribute is a kind (ATTR.*) and a Float32Array of four parameters")
PICK_MSG = _T("gsplat: pick expects a Uint32Array of x,y pairs")
PICK_RANGE = ("RangeError", "gsplat: pick takes 1..65536 queries and maxContrib 0..256")
MASK_MSG = "gsplat.%s: mask needs maskWidth, maskHeight and width * height bytes"
MISUSE = (
    _each("uploadSplats", [1, 1, 2, 2, 2], _T("gsplat.uploadSplats: need n*320 bytes")) + [("shareSplats", 1, tuple(NO_HANDLE[:2]))] +
    _each("renderSync", [1, 1], _T("gsplat.render: need the 160-byte uniform block")) +
    _each("renderAsync", [1, 1], _T("gsplat.renderAsync: need the 160-byte uniform block")) + [("readBuffer", 1, GENERIC)] +
    [("pick", 1, PICK_MSG), ("pick", 1, PICK_MSG), ("pick", 1, PICK_RANGE), ("pick", 2, GENERIC), ("pick", 2, PICK_RANGE)] +
    [("accumulateCoverage", 1, _T("gsplat.accumulateCoverage: {x0, y0, x1, y1} required"))] +
    _each("accumulateCoverage", [1, 1], _T(MASK_MSG % "accumulateCoverage")) + _each("stateCoverage", range(1, 8), GENERIC) +
    _each("attrSummary", [1, 2, 2], ATTR_MSG) + _each("attrSummary", [3, 4], GENERIC) +
    _each("attrHistogram", [1, 2], ATTR_MSG) + _each("attrHistogram", range(3, 8), GENERIC) +
    _each("attrValues", [1, 2], ATTR_MSG) + _each("attrValues", [3, 4], GENERIC) +
    _each("stateAttr", [1, 2], ATTR_MSG) + _each("stateAttr", range(3, 10), GENERIC) +
    _each("neighCount", range(1, 8), GENERIC) + _each("stateNeigh", range(1, 8), GENERIC) +
    _each("stateRegion", [1, 1], _T("gsplat.stateRegion: {kind} required")) +
    [("stateRegion", 1, _T("gsplat.stateRegion: uniforms must be the 160-byte block")), ("stateRegion", 1, _T(MASK_MSG % "stateRegion"))] +
    _each("stateRegion", [2, 3], GENERIC) +
    _each("stateIds", [1, 1], _T("gsplat.stateIds: expects a Uint32Array of splat indices")) + _each("stateIds", [2, 3], GENERIC) +
    _each("stateCount", [1, 2], GENERIC) + [("writeState", 1, _T("gsplat.writeState: expects a Uint8Array of N state bytes"))] +
    _each("setOption", [1, 2], GENERIC) + _each("listState", [1, 2], _T("gsplat.listState: mask and value must be numbers")) +
    _each("exportSplats", [1, 2], _T("gsplat.exportSplats: mask and value must be numbers")) +
    _each("compact", [1, 2], _T("gsplat.compact: mask and value must be numbers")) +
    _each("exportPly", [1, 2, 3, 4], _T("gsplat.exportPly: expects (handle, path, mask, value, shDegree)")) +
    _each("transformSplats", [1, 1, 2, 3], _T("gsplat.transformSplats: expects (handle, the buffer composeTransform returned, mask, value)")) +
    [("uploadPly", 1, _T("gsplat.uploadPly: path required"))] +
    _each("renderToSink", [1, 2], _T("gsplat.renderToSink: need the 160-byte uniform block and a sink buffer")))
# the exports whose only argument is the handle: nothing to get wrong on a live one
HANDLE_ONLY = {"readRgba8", "resetCoverage", "readCoverage", "neighRead", "readState", "stats", "slab"}


@pytest.mark.gpu
def test_misuse_on_a_live_handle_is_refused_before_anything_runs(tmp_path):
    """One call per argument position with a wrong-typed or too-short value; the handle has rendered nothing afterwards and still
    renders."""
    from gsplat import synth
    n, W, H = 64, 64, 48
    rec, ub = str(tmp_path / "rec.bin"), str(tmp_path / "u.bin")
    scene(n).tofile(rec)
    synth.orbit_camera(4, W, H).uniforms(W, H).astype(np.float32).tofile(ub)
    got = _node("misuse", rec, n, W, H, ub)
    assert set(got["exports"]) == FUNCTIONS - NO_CONTEXT
    assert [(r["fn"], r["pos"]) for r in got["rows"]] == [(fn, k) for fn, k, _ in MISUSE]
    assert {fn for fn, _, _ in MISUSE} == FUNCTIONS - NO_CONTEXT - HANDLE_ONLY
    wrong = []
    for r, (fn, k, (cls, msg)) in zip(got["rows"], MISUSE):
        g = r["got"]
        if g is None or g[0] != cls or g[2] is not None or (g[1] != msg if msg is not None else not g[1].startswith("N-API call failed: ")):
            wrong.append((r, cls, msg))
    assert wrong == []
    assert got["framesAfter"] == 0 and got["bytes"] == H * W * 4


@pytest.mark.gpu
def test_sink_frames_in_flight_hold_the_handle_and_defer_destroy(tmp_path):
    """The mirror of test_js_host's renderAsync case: with three renderToSink frames outstanding the handle refuses renderAsync and
    stats, destroy() returns at once and takes effect when the last frame completes, and every sink holds its frame."""
    from gsplat import synth
    n, W, H = 8000, 256, 160
    rec, ub = str(tmp_path / "rec.bin"), str(tmp_path / "u.bin")
    scene(n).tofile(rec)
    np.stack([synth.orbit_camera(3 * k, W, H).uniforms(W, H) for k in range(3)]).astype(np.float32).tofile(ub)
    import re
    got = _node("sinkflight", rec, n, W, H, ub)
    assert got["renderAsync"] is not None and re.search(r"renderAsync frame|in flight", got["renderAsync"][1])
    assert got["stats"] is not None and re.search(r"in flight", got["stats"][1])
    assert got["destroy"] is True and got["resolved"] == [True] * 3
    assert got["same"] == [True] * 3 and got["bytes"] == [W * H * 4] * 3
    assert got["after"] is not None and re.search(r"destroyed", got["after"][1])
