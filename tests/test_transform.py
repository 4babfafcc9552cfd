"""Splat transforms: move, rotate and scale resident splats in place (include/gsplat/gs_abi.h "splat transforms").

Two layers, two kinds of test.  gs_transform_splats applies exactly the f32 numbers of a gs_xform: the kernel is held, on the uint32
view, to tests/xform_restate.py::apply.  gs_xform_compose is host mathematics: it is held on the CPU to an independent float64
construction (xform_restate.compose64) and to the properties that make a rotated splat look right -- colour and covariance
invariance -- with a transposed-matrix negative control that shows the tests can tell the convention.

One caveat on "bit for bit", written down once: IEEE 754 leaves the sign and payload of a NaN that an OPERATION produces or
propagates unspecified, and x86 (numpy) and gfx950 choose differently (inf * 0 is 0xFFC00000 on the one, 0x7FC00000 on the other).
So in the floats a call COMPUTES (xform_restate.touched_floats of the matching records) a NaN on both sides counts as equal;
everywhere else -- every float of an unflagged part, every non-matching record -- the comparison is the uint32 view and a NaN's
payload must survive.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import scene
import export_restate as er
import state_restate as sr
import xform_restate as xr
from support import (F, NODE, ROOT, TAPS, c_layout, code_of, frame_taps, host_sources, in_region, mk, raw_export, run_node, special_records,
                     state_scene)

CSRC = os.path.join(ROOT, "gaussian-splatting-wgpu_amd", "csrc")
_mk = functools.partial(mk, exact=True, state=True)
HID, SEL = er.HIDDEN, er.SELECTED
ALL_FLAGS = xr.POSITION | xr.ORIENT | xr.SIZE
_CACHE = {}


def _f32(v):
    return [float(F(t)) for t in v]


def _compose_pair(q, t, s, pivot):
    """(GsXform of the library, float64 construction) for the same f32 inputs."""
    from gsplat import _abi
    q, t, s = _f32(q), _f32(t), float(F(s))
    pivot = None if pivot is None else _f32(pivot)
    return _abi.compose_xform(q, t, s, pivot), xr.compose64(q, t, s, pivot)


# ---- CPU: the ABI -----------------------------------------------------------------------------------------------------------------
def test_xform_abi(tmp_path):
    """Both symbols are exported without a GPU and listed; the gs_xform layout and the flag values agree between the compiled header
    and ctypes; null and invalid arguments are refused with a message that names the function; the header has the section and the
    version is still 3; the Node names exist."""
    from gsplat import _abi
    L = _abi.load()
    for name in ("gs_xform_compose", "gs_transform_splats"):
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    assert L.gs_abi_version() == 3
    fields = [n for n, _ in _abi.GsXform._fields_]
    consts = ["GS_XFORM_POSITION", "GS_XFORM_ORIENT", "GS_XFORM_SIZE", "GS_ABI_VERSION"]
    prog = 'printf("%zu", sizeof(gs_xform));'
    prog += "".join('printf(" %%zu", offsetof(gs_xform, %s));' % n for n in fields)
    prog += "".join('printf(" %%u", (unsigned)%s);' % c for c in consts)
    out = c_layout(tmp_path, "xform_layout", prog)
    assert out[0] == ctypes.sizeof(_abi.GsXform) == 408
    assert out[1:1 + len(fields)] == [getattr(_abi.GsXform, n).offset for n in fields]
    assert out[1 + len(fields):] == [1, 2, 4, 3]
    assert [_abi.GS_XFORM_POSITION, _abi.GS_XFORM_ORIENT, _abi.GS_XFORM_SIZE] == [xr.POSITION, xr.ORIENT, xr.SIZE] == [1, 2, 4]
    # refusals of gs_xform_compose
    f3, f4 = ctypes.c_float * 3, ctypes.c_float * 4
    x = _abi.GsXform()
    x.flags = 0xABCD
    one, zero3 = f4(1, 0, 0, 0), f3(0, 0, 0)
    inf, nan = float("inf"), float("nan")
    bad = [(None, zero3, 1.0, None, x), (one, None, 1.0, None, x), (one, zero3, 1.0, None, None),
           (f4(0, 0, 0, 0), zero3, 1.0, None, x), (f4(1, nan, 0, 0), zero3, 1.0, None, x), (f4(inf, 0, 0, 0), zero3, 1.0, None, x),
           (one, zero3, 0.0, None, x), (one, zero3, -2.0, None, x), (one, zero3, inf, None, x), (one, zero3, nan, None, x),
           (one, f3(0, nan, 0), 1.0, None, x), (one, f3(inf, 0, 0), 1.0, None, x), (one, zero3, 1.0, f3(0, 0, -inf), x)]
    for rot, tr, s, pv, o in bad:
        assert L.gs_xform_compose(rot, tr, s, pv, ctypes.byref(o) if o is not None else None) == _abi.GS_ERR_INVALID_ARGUMENT
        assert b"gs_xform_compose" in L.gs_last_error()
    assert x.flags == 0xABCD  # a refusal writes nothing
    assert L.gs_xform_compose(one, zero3, 1.0, None, ctypes.byref(x)) == 0 and x.struct_size == 408 and x.flags == xr.POSITION
    # gs_transform_splats without a context
    n = ctypes.c_uint64(77)
    assert L.gs_transform_splats(None, 0, 0, ctypes.byref(x), ctypes.byref(n)) == _abi.GS_ERR_INVALID_ARGUMENT
    assert b"gs_transform_splats" in L.gs_last_error() and b"null" in L.gs_last_error() and n.value == 77
    rjs, idx, dts, napi, hdr = host_sources()
    assert "splat transforms" in hdr and "#define GS_ABI_VERSION 3\n" in hdr
    for decl in ("int32_t gs_xform_compose(", "int32_t gs_transform_splats(", "typedef struct gs_xform {"):
        assert decl in hdr
    for words in ("12 B read, 12 B written", "16 + 180 B each way", "12 B read, 16 B written", "NOT a bit-exact undo", "NON-UNIFORM"):
        assert words in hdr
    assert "transformSplats(" in dts and "transformSplats(" in rjs
    assert "composeTransform" in idx and "export function composeTransform(" in dts
    for name in ("composeTransform", "transformSplats"):
        assert '{"%s", js_' % name in napi


# ---- CPU: gs_xform_compose against float64 ---------------------------------------------------------------------------------------
TRANSLATE = (0.25, -1.5, 0.625)
PIVOT = (0.3, -1.2, 2.0)


def _is_identity_q(x):
    return abs(x.q[0]) == 1.0 and x.q[1] == 0.0 and x.q[2] == 0.0 and x.q[3] == 0.0


@pytest.mark.parametrize("pivot", [None, PIVOT], ids=["origin", "pivot"])
@pytest.mark.parametrize("scale", [1.0, 0.5, 3.0])
def test_compose_entries_and_flags(scale, pivot):
    """Every entry of q, sh1, sh2, sh3 within 1e-6 absolute of the float64 construction, m and log_scale within 1e-6 (1 + |entry|);
    the flags as specified.  (Entries of orthogonal matrices are <= 1 in magnitude and one rounding to f32 costs <= 2^-25.)"""
    for name, q in xr.issue_rotations():
        x, c = _compose_pair(q, TRANSLATE, scale, pivot)
        for field, want in (("q", c["q"]), ("sh1", c["sh1"]), ("sh2", c["sh2"]), ("sh3", c["sh3"])):
            got = np.array(list(getattr(x, field)), np.float64)
            assert np.abs(got - want.ravel()).max() <= 1e-6, (name, field)
        m = np.array(list(x.m), np.float64)
        assert (np.abs(m - c["m"]) <= 1e-6 * (1 + np.abs(c["m"]))).all(), name
        assert abs(x.log_scale - c["log_scale"]) <= 1e-6 * (1 + abs(c["log_scale"])), name
        want_flags = xr.POSITION | (0 if _is_identity_q(x) else xr.ORIENT) | (0 if scale == 1.0 else xr.SIZE)
        assert x.flags == want_flags and x.struct_size == 408, name
        assert (name == "identity") == _is_identity_q(x)
        for l, D in ((1, c["sh1"]), (2, c["sh2"]), (3, c["sh3"])):  # the construction itself: orthogonal
            assert np.abs(D @ D.T - np.eye(2 * l + 1)).max() < 1e-12
    x, _ = _compose_pair((-2.0, 0, 0, 0), TRANSLATE, scale, pivot)  # -(1,0,0,0) after normalisation: the same rotation
    assert _is_identity_q(x) and not x.flags & xr.ORIENT


def test_compose_homomorphism():
    """D_l(R1 R2) == D_l(R1) D_l(R2) within 1e-5, on the library's f32 matrices."""
    from gsplat import _abi
    rots = [q for _, q in xr.issue_rotations()]
    rng = np.random.default_rng(5)
    for _ in range(40):
        a, b = rots[rng.integers(len(rots))], rots[rng.integers(len(rots))]
        a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
        xa, xb, xab = (_abi.compose_xform(_f32(q)) for q in (a, b, xr.qmul(a, b)))
        for f, w in (("sh1", 3), ("sh2", 5), ("sh3", 7)):
            A, B, AB = (np.array(list(getattr(v, f)), np.float64).reshape(w, w) for v in (xa, xb, xab))
            assert np.abs(A @ B - AB).max() <= 1e-5, f


def _colour_defect(x, R, coef, dirs, transpose=False):
    """max over directions of |colour'(R d) - colour(d)| / sum_j |c_j| per channel, float64 with the f32 matrices of x."""
    new = coef.copy()
    for f, (l, k0, w) in zip(("sh1", "sh2", "sh3"), xr.BANDS):
        D = np.array(list(getattr(x, f)), np.float64).reshape(w, w)
        new[k0:k0 + w] = (D.T if transpose else D) @ coef[k0:k0 + w]
    diff = np.abs(xr.colour_sh(new, dirs @ R.T) - xr.colour_sh(coef, dirs))  # rows (R d)^T = d^T R^T
    return (diff / np.abs(coef).sum(axis=0)[None, :]).max()


def test_compose_colour_invariance():
    """colour'(R d) == colour(d) within 1e-6 sum|c_j| per channel (derivable: sum_i |B_i(d)| <= 2 per band times 2^-25 per entry is
    about 6e-8 sum|c|).  Negative control: with every D_l transposed the same check fails at a 90 degree rotation."""
    rng = np.random.default_rng(11)
    dirs = xr.directions(200, 3)
    for name, q in xr.issue_rotations():
        for scale in (1.0, 0.5, 3.0):
            for pivot in (None, PIVOT):
                x, c = _compose_pair(q, TRANSLATE, scale, pivot)
                coef = rng.uniform(-1, 1, size=(16, 3))
                assert _colour_defect(x, c["R"], coef, dirs) <= 1e-6, (name, scale, pivot)
    x, c = _compose_pair(xr.axis_angle((0, 0, 1), np.pi / 2), (0, 0, 0), 1.0, None)
    coef = rng.uniform(-1, 1, size=(16, 3))
    assert _colour_defect(x, c["R"], coef, dirs) <= 1e-6
    assert _colour_defect(x, c["R"], coef, dirs, transpose=True) > 1e-2


def test_compose_covariance_invariance():
    """Restated records: the float64 covariance of (log_scale', rot') equals s^2 R Sigma R^T within 1e-5 relative Frobenius (the f32
    quaternion product carries a few 2^-24 of relative error); the set includes records with an unnormalised rot."""
    rng = np.random.default_rng(21)
    rec = np.zeros((64, 80), F)
    rec[:, 4:7] = rng.uniform(-4, 1, size=(64, 3))
    rot = rng.normal(size=(64, 4))
    rot[:32] /= np.linalg.norm(rot[:32], axis=1, keepdims=True)
    rot[32:] *= rng.uniform(0.05, 20, size=(32, 1))  # unnormalised
    rec[:, 8:12] = rot
    before = [xr.covariance(a[4:7], a[8:12]) for a in rec]
    for name, q in xr.issue_rotations():
        for scale in (1.0, 0.5, 3.0):
            for pivot in (None, PIVOT):
                x, c = _compose_pair(q, TRANSLATE, scale, pivot)
                out = xr.apply(rec, xr.Xform.from_struct(x).with_flags(ALL_FLAGS))
                s = float(F(scale))
                for sig, b in zip(before, out):
                    want = s * s * c["R"] @ sig @ c["R"].T
                    got = xr.covariance(b[4:7], b[8:12])
                    assert np.linalg.norm(got - want) <= 1e-5 * np.linalg.norm(want), (name, scale, pivot)


def test_restatement_sanity():
    """flags = 0 returns the records bit for bit; each single flag changes exactly its own floats (uint32 view)."""
    rec = special_records(1025)
    x, _ = _compose_pair(xr.axis_angle((0.3, -0.5, 0.81), 0.65), TRANSLATE, 1.7, PIVOT)
    X = xr.Xform.from_struct(x)
    np.testing.assert_array_equal(er.bits(xr.apply(rec, X.with_flags(0))), er.bits(rec))
    sel = np.arange(1025) % 3 != 0
    seen = set()
    for fl in (xr.POSITION, xr.ORIENT, xr.SIZE):
        out = xr.apply(rec, X.with_flags(fl), sel)
        changed = er.bits(out) != er.bits(rec)
        assert not changed[~sel].any()
        cols = set(np.flatnonzero(changed.any(axis=0)).tolist())
        assert cols == set(xr.touched_floats(fl)), fl
        assert not cols & seen
        seen |= cols
    assert len(seen) == 3 + 3 + 4 + 45 and not seen & set(er.PADDING) and not seen & {12, 16, 17, 18}


# ---- CPU: end to end on the oracle ---------------------------------------------------------------------------------------------------
def _sh_scene():
    """cfgA's scene; if bicycle_like leaves bands 1-3 (nearly) zero they are filled with seeded values of magnitude <= 0.5 / (l + 1):
    the test must exercise the SH path."""
    if "sh_scene" not in _CACHE:
        s = np.array(scene(10000), dtype=F, copy=True)
        cols = [16 + 4 * k + c for k in range(1, 16) for c in range(3)]
        if np.abs(s[:, cols]).mean() < 0.02:
            rng = np.random.default_rng(404)
            for l, k0, w in xr.BANDS:
                for k in range(k0, k0 + w):
                    s[:, 16 + 4 * k:16 + 4 * k + 3] = rng.uniform(-0.5 / (l + 1), 0.5 / (l + 1), size=(s.shape[0], 3)).astype(F)
        _CACHE["sh_scene"] = s
    return _CACHE["sh_scene"]


def _moved_uniforms(u, m64):
    """view' = view M^-1, proj' = proj M^-1, cam' = M cam (column-major mat4 in the uniforms), rounded to f32 once."""
    M = np.eye(4)
    M[:3, :] = np.asarray(m64, np.float64).reshape(3, 4)
    Mi = np.linalg.inv(M)
    out = np.array(u, dtype=np.float64)
    for o in (0, 16):
        A = out[o:o + 16].reshape(4, 4).T
        out[o:o + 16] = (A @ Mi).T.ravel()
    out[32:35] = (M @ np.append(out[32:35], 1.0))[:3]
    return out.astype(F)


def _image_distance(a, b):
    d = np.abs(a["rgba8"][..., :3].astype(np.int32) - b["rgba8"][..., :3].astype(np.int32))
    return float(d.mean()), float((d.max(axis=2) > 2).mean())


def test_transformed_scene_renders_the_same_image(oracle):
    """The oracle's frame of cfgA (10 000 splats, 256 x 256, tile 16) against its frame of the restated transform of the whole scene
    by a rigid 37 degree skew rotation plus a translation, seen by the camera moved with it.  The two differ only where f32 rounding
    tips one of the reference's own discontinuities (rect truncation, the 1/255 and 1e-4 tests); the yardstick is the same
    comparison with the transform restated in float64 and rounded once per record float.  The f32 path may show at most twice the
    yardstick's mean absolute difference plus 0.1 LSB, and twice its share of pixels over 2 LSB plus 0.1 %.
    Measured (profiles/transform_ops.txt): f32 mean 0.000254 LSB, 0 % of pixels over 2 LSB; float64 yardstick mean 0.000214 LSB,
    0 %; with every D_l transposed: mean 6.10 LSB, 65.1 % of pixels over 2 LSB."""
    W = H = 256
    ts = 16
    from gpu_checks import orbit_uniforms
    s, u = _sh_scene(), orbit_uniforms(W, H)
    cols = [16 + 4 * k + c for k in range(1, 16) for c in range(3)]
    assert np.abs(s[:, cols]).mean() >= 0.02
    x, c = _compose_pair(xr.axis_angle((0.3, -0.5, 0.81), np.deg2rad(37.0)), (0.4, -0.3, 0.2), 1.0, None)
    assert x.flags == xr.POSITION | xr.ORIENT
    u2 = _moved_uniforms(u, c["m"])
    base = oracle.render(s, u, W, H, ts)
    assert base["rgba8"][..., :3].any()
    X = xr.Xform.from_struct(x)
    f32 = _image_distance(base, oracle.render(xr.apply(s, X), u2, W, H, ts))
    f64 = _image_distance(base, oracle.render(xr.apply(s, xr.xform64(c, x.flags)), u2, W, H, ts))
    bad = _image_distance(base, oracle.render(xr.apply(s, X.transposed_sh()), u2, W, H, ts))
    print("transform end to end: f32 mean %.6f LSB, %.5f %% over 2 LSB; f64 mean %.6f LSB, %.5f %%; transposed mean %.4f LSB, %.3f %%"
          % (f32[0], 100 * f32[1], f64[0], 100 * f64[1], bad[0], 100 * bad[1]))
    bound = (2 * f64[0] + 0.1, 2 * f64[1] + 0.001)
    assert f32[0] <= bound[0] and f32[1] <= bound[1]
    assert bad[0] > bound[0] and bad[1] > bound[1]  # the control: the test can tell the convention


def test_sanitized_host_program(tmp_path):
    """tools/xform_check: gs_xform_compose's translation unit compiled alone with -fsanitize=address,undefined and run over a few
    hundred seeded rotations (orthogonality of every D_l, the refusals).  Skipped where the sanitizer runtime is not installed."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed")
    exe = str(tmp_path / "xform_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san +
                          ["-I", CSRC, os.path.join(ROOT, "tools", "xform_check", "main.cpp"), "-x", "c++",
                           os.path.join(CSRC, "gs_xform_math.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "xform_check ok" in out.stdout


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
FILTERS = [(0, 0), (HID, 0), (SEL, SEL), (0xFF, 0x83), (0, 1)]
FLAG_SETS = [1, 2, 3, 4, 5, 6, 7]


def _assert_records(got, want, rows, flags, msg=""):
    """uint32 view; in the floats the call computed (module docstring) a NaN on both sides is equal."""
    g, w = er.bits(got), er.bits(want)
    ok = g == w
    if rows.size and flags:
        relax = np.zeros(ok.shape, bool)
        relax[np.ix_(rows, xr.touched_floats(flags))] = True
        ok |= relax & np.isnan(got) & np.isnan(want)
    assert ok.all(), "%s: %d floats differ, first at (record, float) %s" % (msg, int((~ok).sum()), np.argwhere(~ok)[0].tolist())


def _edge_xform(k):
    from gsplat import _abi
    ang = 0.3 + 0.37 * k
    axis = ((k % 3) - 0.7, 0.4 + (k % 5) * 0.2, -0.9 + (k % 7) * 0.3)
    return _abi.compose_xform(xr.axis_angle(axis, ang), (0.05 * (k % 4), -0.02 * k, 0.03), 1.25 if k % 2 else 0.8, (0.1, 0.2, -0.3))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 3001])
def test_transform_kernel(n):
    """Every filter x all seven flag sets on records with NaNs, a payload NaN, -0, +-inf and a denormal, under a seeded mix of state
    bytes: the export after the call equals the restatement of the export before it on the matching records, every other record
    and every unflagged float is untouched bit for bit, the state plane is unchanged, *matched is the restated count.  Once with
    guard-filled device memory around the exported buffer."""
    from gsplat import _abi
    rec = special_records(n)
    rng = np.random.default_rng(900 + n)
    plane = rng.choice(np.array([0, HID, SEL, HID | SEL, 0x83, 0x80, 0x42], np.uint8), size=n)
    r = _mk(rec, 64, 64, 8)
    r.write_state(plane)
    cur = r.export_splats()
    np.testing.assert_array_equal(er.bits(cur), er.bits(er.zero_padding(rec)))
    k = 0
    some = 0
    for mask, value in FILTERS:
        sel = er.keep(plane, mask, value)
        rows = np.flatnonzero(sel)
        for fl in FLAG_SETS:
            x = _edge_xform(k)
            k += 1
            x.flags = fl
            want = xr.apply(cur, xr.Xform.from_struct(x), sel)
            assert r.transform(x, mask, value) == rows.size
            got = r.export_splats()
            _assert_records(got, want, rows, fl, "n=%d filter (%#x, %#x) flags %d" % (n, mask, value, fl))
            some += int((er.bits(got) != er.bits(cur)).any())
            cur = got  # the next step starts from what the device holds
    assert some >= (21 if n >= 64 else 7)  # the calls did something
    np.testing.assert_array_equal(r.read_state(), plane)
    x = _edge_xform(k)
    x.flags = 0  # a valid no-op that still reports the count
    assert r.transform(x, HID, 0) == int(er.keep(plane, HID, 0).sum())
    x.flags = ALL_FLAGS
    want = xr.apply(cur, xr.Xform.from_struct(x))
    assert r.transform(x, 0, 0) == n
    got, ids = raw_export(r, 0, 0, True, device=True)  # guards behind the records and the ids are checked inside
    _assert_records(got, want, np.arange(n), ALL_FLAGS, "guarded n=%d" % n)
    np.testing.assert_array_equal(ids, np.arange(n, dtype=np.uint32))
    r.destroy()


CASES = [("cfgA", 8), ("cfgA", 16), ("cfgA", 32), ("ragged", 8)]


def _similarity():
    from gsplat import _abi
    x = _abi.compose_xform(xr.axis_angle((0.3, -0.5, 0.81), np.deg2rad(25.0)), (0.15, 0.1, -0.2), 1.3, (0.0, 0.0, 0.0))
    assert x.flags == ALL_FLAGS
    return x


def _selected_and_moved(name):
    """(plane with the unit sphere selected, restated records after the similarity on the selection)"""
    k = ("moved", name)
    if k not in _CACHE:
        s = state_scene(name)[0]
        inside = in_region(name, "sphere_r1")
        assert 0 < inside.sum() < s.shape[0]
        plane = np.where(inside, SEL, 0).astype(np.uint8)
        _CACHE[k] = (plane, xr.apply(s, xr.Xform.from_struct(_similarity()), inside))
    return _CACHE[k]


@pytest.mark.gpu
@pytest.mark.parametrize("slab", [False, True], ids=["canvas", "slab"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fused"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-t%d" % c)
def test_transform_is_an_upload_of_the_transformed_records(oracle, case, exact, slab):
    """After a sphere selection and a similarity with all three flags on (SEL, SEL) the context is indistinguishable from a fresh
    one given gs_upload_splats(restated records) + gs_state_write(the bytes): every tap of a gs_render_debug frame and of a tight
    gs_render frame and the image, bit for bit; in EXACT mode the image is also the oracle's render of the restated records.  The
    slab contexts reach the smax path (the conservative radius of the slab cull)."""
    from gpu_checks import check_image
    name, ts = case
    s, u, W, H = state_scene(name)
    plane, moved = _selected_and_moved(name)
    ntx = oracle.num_tiles(W, H, ts)[0]
    cols = (ntx // 4, ntx - ntx // 8) if slab else None
    r = _mk(s, W, H, ts, exact=exact, cols=cols)
    assert r.select_sphere((0.0, 0.0, 0.0), 1.0) == int((plane != 0).sum())
    assert r.transform(_similarity()) == int((plane != 0).sum())
    np.testing.assert_array_equal(r.read_state(), plane)
    np.testing.assert_array_equal(er.bits(r.export_splats()), er.bits(er.zero_padding(moved)))
    fresh = _mk(moved, W, H, ts, exact=exact, cols=cols)
    fresh.write_state(plane)
    for debug in (True, False):
        a, b = frame_taps(r, u, debug), frame_taps(fresh, u, debug)
        for t in TAPS + ("rgba8", "rgbf"):
            np.testing.assert_array_equal(a[t], b[t], err_msg="%s debug=%s" % (t, debug))
        if exact:
            k = ("ref", name, ts, cols)
            if k not in _CACHE:
                _CACHE[k] = sr.state_frame(oracle, moved, u, W, H, ts, plane, cols=cols)
            check_image(r, _CACHE[k], True)
    assert a["rgba8"][..., :3].any()
    fresh.destroy()
    r.destroy()


@pytest.mark.gpu
def test_transform_on_frame_paths(oracle):
    """The ring, a captured frame graph, gs_pick, a borrower, an unflagged context and the refusals."""
    from gpu_checks import check_image
    from gsplat import _abi
    from pick_restate import restate_ref
    L = _abi.load()
    name, ts = "cfgA", 16
    s, u, W, H = state_scene(name)
    plane, moved = _selected_and_moved(name)
    m = int((plane != 0).sum())
    ref = sr.state_frame(oracle, moved, u, W, H, ts, plane)
    old = sr.state_frame(oracle, s, u, W, H, ts, plane)
    assert (ref["rgba8"] != old["rgba8"]).any()
    x = _similarity()
    # the ring: three frames enqueued and not waited for; the call drains them; it is not a frame
    r = _mk(s, W, H, ts)
    r.write_state(plane)
    for _ in range(3):
        r.render_uniforms(u)
    assert r.transform(x) == m
    st = r.stats()
    assert st["frames_in_flight"] == 3 and st["frames"] == 3
    check_image(r, old, True)  # the taps still describe the third frame
    np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_VALUES), _frame_values(s, plane, u, W, H, ts))
    for _ in range(3):
        r.render_uniforms(u)
    check_image(r, ref, True)
    assert r.stats()["frames_in_flight"] == 3 and r.stats()["frames"] == 6  # the shadows stayed alive
    # gs_pick after the next frame names the ids of the fresh context
    xy = np.array([(px, py) for py in range(3, H, 17) for px in range(5, W, 13)], np.uint32)
    want = restate_ref(ref, W, H, ts, xy)[0]
    got = r.pick(xy)
    for f in ("first_id", "max_id", "median_id", "hit_count"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    assert (got["hit_count"] > 0).any()
    # a borrower is refused itself and renders the owner's transformed scene
    b = _mk(s, W, H, ts, share_with=r)
    before = r.export_splats()
    c, msg = code_of(lambda: b.transform(x))
    assert c == _abi.GS_ERR_INVALID_ARGUMENT and "owner" in msg and "gs_transform_splats" in msg
    np.testing.assert_array_equal(er.bits(r.export_splats()), er.bits(before))
    b.render_uniforms(u)
    b.wait()
    check_image(b, ref, True)
    # errors change nothing
    cnt = ctypes.c_uint64(77)
    bad = []
    for edit in ("size", "flags", "nan_m", "inf_q", "nan_sh", "nan_scale"):
        y = _abi.GsXform.from_buffer_copy(x)
        if edit == "size":
            y.struct_size = 404
        elif edit == "flags":
            y.flags = 0xF
        elif edit == "nan_m":
            y.m[7] = float("nan")
        elif edit == "inf_q":
            y.q[2] = float("inf")
        elif edit == "nan_sh":
            y.sh3[48] = float("nan")
        else:
            y.log_scale = float("nan")
        bad.append(y)
    for y in bad:
        assert L.gs_transform_splats(r._ctx, SEL, SEL, ctypes.byref(y), ctypes.byref(cnt)) == _abi.GS_ERR_INVALID_ARGUMENT
        assert b"gs_transform_splats" in L.gs_last_error()
    for mask, value in ((0x100, 0), (0, 0x100)):
        assert L.gs_transform_splats(r._ctx, mask, value, ctypes.byref(x), ctypes.byref(cnt)) == _abi.GS_ERR_INVALID_ARGUMENT
    assert L.gs_transform_splats(r._ctx, SEL, SEL, None, ctypes.byref(cnt)) == _abi.GS_ERR_INVALID_ARGUMENT
    assert cnt.value == 77
    np.testing.assert_array_equal(er.bits(r.export_splats()), er.bits(before))
    np.testing.assert_array_equal(r.read_state(), plane)
    # a non-finite member of an UNFLAGGED part is not looked at; a null matched is accepted
    y = _abi.GsXform.from_buffer_copy(x)
    y.flags = xr.POSITION
    y.sh2[3] = float("nan")
    y.log_scale = float("inf")
    assert L.gs_transform_splats(r._ctx, 0, 1, ctypes.byref(y), None) == 0  # (0, 1) matches nothing
    np.testing.assert_array_equal(er.bits(r.export_splats()), er.bits(before))
    b.destroy()
    r.destroy()
    # a captured graph: a replay after the transform is the fresh context's frame and graph_frames goes on counting
    g = _mk(s, W, H, ts)
    g.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    g.set_option(_abi.GS_OPT_FRAME_GRAPH, 1)
    g.write_state(plane)
    for _ in range(2):
        g.render_uniforms(u)
        g.wait()
    check_image(g, old, True)
    assert g.stats()["graph_frames"] == 2
    assert g.transform(x) == m
    check_image(g, old, True)
    for k in range(2):
        g.render_uniforms(u)
        g.wait()
        check_image(g, ref, True)
        assert g.stats()["graph_frames"] == 3 + k
    g.destroy()
    # without GS_FLAG_SPLAT_STATE: (0, 0) is accepted, anything else refused; before an upload: GS_ERR_NO_SCENE
    f = _mk(s, W, H, ts, state=False)
    c, msg = code_of(lambda: f.transform(x))
    assert c == _abi.GS_ERR_INVALID_ARGUMENT and "GS_FLAG_SPLAT_STATE" in msg
    np.testing.assert_array_equal(er.bits(f.export_splats()), er.bits(er.zero_padding(s)))
    assert f.transform(x, 0, 0) == s.shape[0]
    np.testing.assert_array_equal(er.bits(f.export_splats()), er.bits(er.zero_padding(xr.apply(s, xr.Xform.from_struct(x)))))
    f.destroy()
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(cfg), 64, 64, 8, _abi.GS_FLAG_SPLAT_STATE
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    assert L.gs_transform_splats(ctx, 0, 0, ctypes.byref(x), ctypes.byref(cnt)) == _abi.GS_ERR_NO_SCENE
    _abi.check(L.gs_upload_splats(ctx, None, 0))  # N == 0
    assert L.gs_transform_splats(ctx, 0, 0, ctypes.byref(x), ctypes.byref(cnt)) == 0 and cnt.value == 0
    cnt.value = 77
    assert L.gs_transform_splats(ctx, SEL, SEL, ctypes.byref(x), ctypes.byref(cnt)) == 0 and cnt.value == 0
    _abi.check(L.gs_destroy(ctx))


def _frame_values(s, plane, u, W, H, ts):
    """GS_BUF_VALUES of the product frame of (s, plane) on a context that is not transformed afterwards."""
    from gsplat import _abi
    r = _mk(s, W, H, ts)
    r.write_state(plane)
    for _ in range(3):
        r.render_uniforms(u)
    r.wait()
    out = r.read_buffer(_abi.GS_BUF_VALUES)
    r.destroy()
    return out


@pytest.mark.gpu
def test_python_hosts():
    """Renderer.translate_selected / rotate_selected / scale_selected are transform(compose_xform(...)) on the selection, and
    PipelinedRenderer.transform drains every slot and asks the owner."""
    import gsplat
    from gsplat import _abi
    name, ts = "cfgA", 16
    s, u, W, H = state_scene(name)
    inside = in_region(name, "sphere_r1")
    m = int(inside.sum())
    q, piv = _f32(xr.axis_angle((1, 2, -1), 0.4)), (0.1, -0.2, 0.3)
    steps = [_abi.compose_xform(translate=(0.5, 0.0, -0.25)), _abi.compose_xform(rot=q, pivot=piv), _abi.compose_xform(scale=0.75, pivot=piv)]
    assert [x.flags for x in steps] == [xr.POSITION, xr.POSITION | xr.ORIENT, xr.POSITION | xr.SIZE]
    want = s
    for x in steps:
        want = xr.apply(want, xr.Xform.from_struct(x), inside)
    r = _mk(s, W, H, ts)
    assert r.select_sphere((0.0, 0.0, 0.0), 1.0) == m
    assert r.translate_selected((0.5, 0.0, -0.25)) == m and r.rotate_selected(q, piv) == m and r.scale_selected(0.75, piv) == m
    np.testing.assert_array_equal(er.bits(r.export_splats()), er.bits(er.zero_padding(want)))
    r.render_uniforms(u)
    r.wait()
    img = r.read_rgba8()
    r.destroy()
    p = gsplat.PipelinedRenderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(s), ts, frames_in_flight=3,
                                 flags=_abi.GS_FLAG_EXACT_BLEND | _abi.GS_FLAG_F32_TAP | _abi.GS_FLAG_SPLAT_STATE)
    p.render_uniforms(u)  # in flight when the calls come
    assert p.select_sphere((0.0, 0.0, 0.0), 1.0) == m
    p.render_uniforms(u)
    for x in steps:
        assert p.transform(x) == m
    np.testing.assert_array_equal(er.bits(p.export_splats()), er.bits(er.zero_padding(want)))
    slots = [p.render_uniforms(u) for _ in range(3)]
    for slot in slots:
        np.testing.assert_array_equal(p.read_rgba8(slot), img)
    assert img[..., :3].any()
    p.destroy()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_node_host_transform_matches_python(tmp_path):
    """tests/js/xform_check.js selects a sphere, composes and applies a similarity, renders and exports through the Node host: the
    struct, the records and the image equal what the Python host makes of the same sequence, byte for byte."""
    from gsplat import _abi
    s, u, W, H = state_scene("cfgA")
    n, ts = s.shape[0], 16
    rec, ub, out = (str(tmp_path / f) for f in ("rec.bin", "u.bin", "out.bin"))
    s.tofile(rec)
    np.ascontiguousarray(u, F).tofile(ub)
    info = run_node("xform_check.js", (rec, n, W, H, ts, ub, out))
    x = _abi.compose_xform(rot=(0.9, 0.1, -0.3, 0.2), translate=(0.15, 0.1, -0.2), scale=1.3, pivot=(0.1, 0.0, -0.1))
    r = _mk(s, W, H, ts, exact=False)
    m = r.select_sphere((0.0, 0.0, 0.0), 1.0)
    assert r.transform(x) == m
    r.render_uniforms(u)
    r.wait()
    img = r.read_rgba8()
    exported = r.export_splats()
    r.destroy()
    assert info["selected"] == m and info["matched"] == m and info["matchedAll"] == n and info["structBytes"] == 408 and info["flags"] == 7
    raw = np.fromfile(out, dtype=np.uint8)
    o = 0
    for want in (np.frombuffer(bytes(x), np.uint8), img, exported):
        nb = want.nbytes
        np.testing.assert_array_equal(raw[o:o + nb], np.ascontiguousarray(want).view(np.uint8).ravel())
        o += nb
    assert raw.size == o
    assert info["errors"] == {"borrower": "-1", "badMask": "-1", "zeroQuaternion": "-1"}
