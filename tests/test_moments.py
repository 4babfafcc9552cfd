"""Moments (gs_abi.h "moments"): gs_attr_moments and gs_moments_host against the Fraction restatement of tests/moments_restate.py,
bit for bit on hi and lo; the rules and the verbs of gsplat.moments."""
import ctypes
import functools
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import attr_restate as ar
import moments_restate as mr
from conftest import scene
from support import F, ROOT, SLAB_COLS, c_layout, cached, code_of, frame_taps, guarded, is_fill, mk, state_scene, timeless

_mk = functools.partial(mk, state=True)
CSRC = os.path.join(ROOT, "gaussian-splatting-wgpu_amd", "csrc")
SEL = (2, 2)
SIZED = ("scene", "wild", "cancel")
CELLS = [(k, n) for k in SIZED for n in mr.LENGTHS] + [("outlier", 1043), ("nonfinite", 1043)]


def positions(kind, n):
    """(n, 3) float32, seeded, once per session."""
    def make():
        if kind == "scene":
            return np.ascontiguousarray(scene(10000)[:n, 0:3])
        if kind == "wild":
            return mr.wild(n)
        if kind == "cancel":
            return mr.cancel(n)
        return mr.outlier() if kind == "outlier" else mr.nonfinite()
    return cached(("moments_positions", kind, n), make)


def records(pos):
    """scene() records with the given centres."""
    rec = np.array(scene(10000)[:pos.shape[0]], dtype=F, copy=True)
    rec[:, 0:3] = pos
    return np.ascontiguousarray(rec)


def want_xyz(kind, n, where):
    """The restatement of (X, Y, Z) over one cell and filter, computed once and shared by the CPU and the GPU tests."""
    def make():
        pos = positions(kind, n)
        return mr.restate([pos[:, 0], pos[:, 1], pos[:, 2]], mr.keep_of(where, mr.third(n)))
    return cached(("moments_want", kind, n, where), make)


def tie_scene():
    """Every set of mr.ties() in one plane, told apart by the state byte (set k: k + 1)."""
    vals, st = [], []
    for k, (v, _, _) in enumerate(mr.ties()):
        vals += v
        st += [k + 1] * len(v)
    return np.array(vals, F), np.array(st, np.uint8)


def _attrs(*kinds):
    from gsplat import attributes
    return [attributes.attr(k) for k in kinds]


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_moments_abi(tmp_path):
    """Both symbols are exported without a GPU and listed; gs_exact is 16 bytes, gs_attr_moments 160, every offset agrees between the
    compiled header and ctypes; the version is still 3 and GS_ATTR_COUNT 16; a null ctx and the host call's bad arguments are refused
    with the call's name; the renderer classes gained no public method; the header points from "There is no mean" to the call."""
    from gsplat import _abi, moments, renderer
    L = _abi.load()
    for name in ("gs_attr_moments", "gs_moments_host"):
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    assert L.gs_abi_version() == 3
    fe, fm = [n for n, _ in _abi.GsExact._fields_], [n for n, _ in _abi.GsAttrMoments._fields_]
    prog = 'printf("%zu %zu", sizeof(gs_exact), sizeof(struct gs_attr_moments));'
    prog += "".join('printf(" %%zu", offsetof(gs_exact, %s));' % n for n in fe)
    prog += "".join('printf(" %%zu", offsetof(struct gs_attr_moments, %s));' % n for n in fm)
    prog += 'printf(" %u %u %u", (unsigned)GS_MOMENTS_MAX_ATTRS, (unsigned)GS_ABI_VERSION, (unsigned)GS_ATTR_COUNT);'
    out = c_layout(tmp_path, "moments_layout", prog)
    assert out[0] == ctypes.sizeof(_abi.GsExact) == 16 and out[1] == ctypes.sizeof(_abi.GsAttrMoments) == 160
    assert out[2:4] == [getattr(_abi.GsExact, n).offset for n in fe] == [0, 8]
    assert out[4:8] == [getattr(_abi.GsAttrMoments, n).offset for n in fm] == [0, 8, 16, 64]
    assert out[8:] == [3, 3, 16] and _abi.GS_MOMENTS_MAX_ATTRS == 3
    rec = _abi.GsAttrMoments()
    a = _attrs(ar.POS_X)[0]
    assert L.gs_attr_moments(None, ctypes.byref(a), 1, 0, 0, ctypes.byref(rec)) == _abi.GS_ERR_INVALID_ARGUMENT
    assert b"gs_attr_moments" in L.gs_last_error() and b"null ctx" in L.gs_last_error()
    # gs_moments_host: n_planes outside 1 .. 3, null pointers, a filter without a plane; the record is untouched
    x = np.arange(4, dtype=F)
    ptrs = (ctypes.c_void_p * 4)(*[x.ctypes.data] * 4)
    out = guarded(160, np.uint8)
    po = ctypes.cast(out.ctypes.data, ctypes.POINTER(_abi.GsAttrMoments))
    for args, fragment in (((ptrs, 0, 4, None, 0, 0, po), "0 planes"), ((ptrs, 4, 4, None, 0, 0, po), "4 planes"),
                           ((None, 1, 4, None, 0, 0, po), "null planes"), ((ptrs, 1, 4, None, 4, 4, po), "null state"),
                           (((ctypes.c_void_p * 2)(x.ctypes.data, None), 2, 4, None, 0, 0, po), "null plane 1"),
                           ((ptrs, 1, 4, None, 0x100, 0, po), "does not fit the state byte"), ((ptrs, 1, 1 << 31, None, 0, 0, po), "2^31"),
                           ((ptrs, 1, 4, None, 0, 0, None), "null moments")):
        assert L.gs_moments_host(*args) == _abi.GS_ERR_INVALID_ARGUMENT, fragment
        msg = L.gs_last_error().decode()
        assert "gs_moments_host" in msg and fragment in msg, msg
    assert is_fill(out)
    for bad in ([], [x] * 4):
        code, msg = code_of(lambda: moments.host_moments(bad))
        assert code == _abi.GS_ERR_INVALID_ARGUMENT and "gs_moments_host" in msg
    # n == 0: zeros
    assert mr.same(moments.host_moments([np.zeros(0, F)]), mr.restate([np.zeros(0, F)]))
    # free functions only
    import test_abi
    for cname in ("Renderer", "PipelinedRenderer"):
        live = {n for n in vars(getattr(renderer, cname)) if not n.startswith("_") and callable(getattr(getattr(renderer, cname), n))}
        assert live == set(test_abi.PYTHON_HOST_SURFACE[cname]) - {"__init__"}
    import gsplat
    assert gsplat.moments is moments
    hdr = open(os.path.join(ROOT, "include", "gsplat", "gs_abi.h")).read()
    assert "gs_attr_moments" in hdr[hdr.index("There is no mean"):][:600]
    assert "moments.mean" in gsplat.attributes.summary.__doc__


def test_restatement_is_pinned():
    """The Fraction restatement against math.fsum of the float64 values and products, which are exact (where no product leaves
    float64's range), and against the tie sets' stated answers."""
    for kind, n in (("scene", 1025), ("cancel", 1025), ("outlier", 1043), ("nonfinite", 1043)):
        pos = positions(kind, n)
        for where in mr.FILTERS:
            mr.check_against_fsum([pos[:, 0], pos[:, 1], pos[:, 2]], mr.keep_of(where, mr.third(n)))
    w = positions("wild", 3001)
    mr.check_against_fsum([w[:, 0], w[:, 1], w[:, 2]], products=False)  # (a product of two denormals is not a double)
    for vals, hi, lo in mr.ties():
        got = mr.restate([np.array(vals, F)])
        assert got["sum"][0] == (hi, lo)
        assert Fraction(hi) + Fraction(lo) == sum(Fraction(v) for v in vals)
    assert mr.restate([np.array([-0.0, 0.0, -0.0], F)])["sum"][0] == (0.0, 0.0)
    assert mr.bits(mr.restate([np.array([-0.0], F)])["sum"][0][0]) == 0  # an exact zero is +0.0


@pytest.mark.parametrize("kind,n", CELLS)
def test_host_moments(kind, n):
    """gs_moments_host on every scene, length and filter: (X, Y, Z); one, two and three planes with a repeated one; with and without
    a state plane."""
    from gsplat import moments
    pos = positions(kind, n)
    st = mr.third(n)
    for where in mr.FILTERS:
        got = moments.host_moments([pos[:, 0], pos[:, 1], pos[:, 2]], st, where)
        assert mr.same(got, want_xyz(kind, n, where)), (kind, n, where)
    assert mr.same(moments.host_moments([pos[:, 0], pos[:, 1], pos[:, 2]]), want_xyz(kind, n, (0, 0)))  # no plane at all
    if n in (5, 1025, 1043):
        keep = mr.keep_of(mr.THIRD, st)
        for planes in ([pos[:, 1]], [pos[:, 2], pos[:, 0]], [pos[:, 1], pos[:, 1]], [pos[:, 2], pos[:, 0], pos[:, 2]]):
            assert mr.same(moments.host_moments(planes, st, mr.THIRD), mr.restate(planes, keep)), (kind, n, len(planes))
            assert mr.same(moments.host_moments(planes), mr.restate(planes)), (kind, n, len(planes))
    if kind == "nonfinite":
        full = want_xyz(kind, n, (0, 0))
        assert full["matched"] - full["counted"] == len(mr.EDGES)
        assert abs(full["sum"][0][0]) < 1e5  # the 1e30 beside a NaN is in no sum


def test_host_ties():
    from gsplat import moments
    vals, st = tie_scene()
    for k, (v, hi, lo) in enumerate(mr.ties()):
        got = moments.host_moments([vals], st, (0xFF, k + 1))
        assert got["matched"] == got["counted"] == len(v)
        assert (mr.bits(got["sum"][0][0]), mr.bits(got["sum"][0][1])) == (mr.bits(hi), mr.bits(lo)), (v, got["sum"][0])
        assert mr.same(got, mr.restate([vals], st == k + 1))


def test_python_rules():
    """mean_of / covariance_of through host_moments against their Fraction restatement, on the cancel and the scene data; no splat
    counted: ValueError."""
    from gsplat import moments
    for kind in ("cancel", "scene"):
        pos = positions(kind, 1025)
        m = moments.host_moments([pos[:, 0], pos[:, 1], pos[:, 2]])
        for j in range(3):
            assert mr.bits(moments.mean_of(m, j)) == mr.bits(mr.mean(pos[:, j])), (kind, j)
            for k in range(3):
                assert mr.bits(moments.covariance_of(m, j, k)) == mr.bits(mr.covariance(pos[:, j], pos[:, k])), (kind, j, k)
            assert moments.covariance_of(m, j, j) >= 0.0
        c = moments._covariance(m)
        np.testing.assert_array_equal(c, c.T)
    empty = moments.host_moments([np.array([np.nan, np.inf], F)])
    assert (empty["matched"], empty["counted"]) == (2, 0)
    for fn in (lambda: moments.mean_of(empty), lambda: moments.covariance_of(empty), lambda: moments._axes(empty, "principal_axes")):
        with pytest.raises(ValueError):
            fn()
    two = moments.host_moments([np.arange(2, dtype=F)] * 3)
    with pytest.raises(ValueError):
        moments._axes(two, "principal_axes")
    # the quaternion of a rotation matrix, against compose_xform's own matrix
    rng = np.random.default_rng(2)
    for _ in range(20):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        r, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                      [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                      [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])
        got = np.array(moments._quaternion(R))
        assert min(np.abs(got - q).max(), np.abs(got + q).max()) < 1e-12


def test_sanitized_host_program(tmp_path):
    """tools/moments_check: gs_exact_sum.h compiled alone with -fsanitize=address,undefined and run as its own process over the wild
    and the cancel values; it checks the limb bounds at the extreme exponents itself.  Skipped where the sanitizer runtime is not
    installed."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed")
    exe = str(tmp_path / "moments_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san +
                          ["-I", CSRC, os.path.join(ROOT, "tools", "moments_check", "main.cpp"), "-o", exe])
    for kind, k in (("wild", 3), ("cancel", 2), ("nonfinite", 3), ("outlier", 1)):
        pos = positions(kind, 1025 if kind in SIZED else 1043)[:, :k]
        path = tmp_path / (kind + ".txt")
        path.write_text("%d %d\n" % (k, pos.shape[0]) + "\n".join(" ".join("%08x" % int(w) for w in row) for row in pos.view(np.uint32)) + "\n")
        out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")
        assert lines[0] == "moments_check ok"
        want = mr.restate([pos[:, j] for j in range(k)])
        assert lines[1] == "counted %d" % want["counted"]
        order = [want["sum"][j] for j in range(k)] + [want["prod"][j][l] for j in range(k) for l in range(j, k)]
        got = [tuple(int(x, 16) for x in ln.split()) for ln in lines[2:2 + len(order)]]
        assert got == [(mr.bits(hi), mr.bits(lo)) for hi, lo in order], kind


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", CELLS)
def test_moments_xyz(kind, n):
    """gs_attr_moments of (X, Y, Z) on every scene, length and filter; 3001 splats also with GS_OPT_PERSISTENT_GRID 1 and 2 (several
    trips per thread), where the answer does not change."""
    from gsplat import _abi, moments
    pos = positions(kind, n)
    r = _mk(records(pos), 64, 64, 16)
    r.write_state(mr.third(n))
    for grid in ((0, 1, 2) if n == 3001 else (0,)):
        if grid:
            r.set_option(_abi.GS_OPT_PERSISTENT_GRID, grid)
        for where in mr.FILTERS:
            got = moments.moments(r, _attrs(ar.POS_X, ar.POS_Y, ar.POS_Z), where)
            assert mr.same(got, want_xyz(kind, n, where)), (kind, n, where, grid, got, want_xyz(kind, n, where))
    if n in (5, 1025, 1043):  # one and two planes, a repeated one
        keep = mr.keep_of(mr.THIRD, mr.third(n))
        for kinds in ((ar.POS_Y,), (ar.POS_Z, ar.POS_X), (ar.POS_Y, ar.POS_Y), (ar.POS_Z, ar.POS_X, ar.POS_Z)):
            planes = [pos[:, k] for k in kinds]
            assert mr.same(moments.moments(r, _attrs(*kinds), mr.THIRD), mr.restate(planes, keep)), (kind, n, kinds)
            assert mr.same(moments.moments(r, _attrs(*kinds)), mr.restate(planes)), (kind, n, kinds)
    r.destroy()


@pytest.mark.gpu
def test_moments_spread_over_slots():
    """scene(10000): 10 workgroups on the default grid, more than the 8 slot copies, so two pairs of them share a copy; dense and
    filtered, against gs_moments_host (which test_host_moments holds to the restatement) and, dense, against the restatement."""
    from gsplat import moments
    rec = scene(10000)
    n = rec.shape[0]
    st = mr.third(n)
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    planes = [np.ascontiguousarray(rec[:, j]) for j in range(3)]
    for where in mr.FILTERS:
        assert mr.same(moments.moments(r, _attrs(ar.POS_X, ar.POS_Y, ar.POS_Z), where), moments.host_moments(planes, st, where)), where
    assert mr.same(moments.moments(r, _attrs(ar.POS_X, ar.POS_Y, ar.POS_Z)), mr.restate(planes))
    r.destroy()


@pytest.mark.gpu
def test_moments_ties():
    from gsplat import moments
    vals, st = tie_scene()
    pos = np.zeros((vals.size, 3), F)
    pos[:, 0] = vals
    r = _mk(records(pos), 64, 64, 16)
    r.write_state(st)
    for k, (v, hi, lo) in enumerate(mr.ties()):
        got = moments.moments(r, _attrs(ar.POS_X), (0xFF, k + 1))
        assert got["matched"] == got["counted"] == len(v)
        assert (mr.bits(got["sum"][0][0]), mr.bits(got["sum"][0][1])) == (mr.bits(hi), mr.bits(lo)), (v, got["sum"][0])
        assert mr.same(got, mr.restate([vals], st == k + 1))
    r.destroy()


@pytest.mark.gpu
def test_moments_scratch_route():
    """One, two and three attributes that are not position planes, against the restatement of gs_attr_read's own values: record
    kinds, LOG_SCALE_MAX over NaN log-scales, DIST2 and PLANE, a COVER_SUM after one accumulate, a position mixed with a record kind."""
    from gsplat import attributes, moments
    import test_attributes as ta
    s, u, W, H = state_scene("cfgA")
    n = 3001
    rec = np.ascontiguousarray(s[:n])
    r = _mk(rec, W, H, 16)
    st = mr.third(n)
    r.write_state(st)
    r.render_uniforms(u)
    r.wait()
    r.accumulate_coverage()
    groups = [(ar.OPACITY_LOGIT,), (ar.DIST2, ar.PLANE), (ar.DC_R, ar.OPACITY_LOGIT, ar.LOG_SCALE_MAX), (ar.COVER_SUM,),
              (ar.POS_Y, ar.DC_R), (ar.COVER_SUM, ar.POS_X, ar.COVER_SUM), (ar.LOG_SCALE_SUM, ar.POS_Z, ar.ANISOTROPY)]
    for kinds in groups:
        attrs = [ta._attr(k) for k in kinds]
        planes = [attributes.values(r, a) for a in attrs]
        if ar.COVER_SUM in kinds:
            assert (planes[kinds.index(ar.COVER_SUM)] > 0).sum() > 100
        for where in mr.FILTERS:
            got = moments.moments(r, attrs, where)
            assert mr.same(got, mr.restate(planes, mr.keep_of(where, st))), (kinds, where)
    r.destroy()
    hand = ta.hand_records()  # NaN log-scales, +-inf positions and logits
    r = _mk(hand, 64, 64, 16)
    st = mr.third(hand.shape[0])
    r.write_state(st)
    for kinds in ((ar.LOG_SCALE_MAX,), (ar.LOG_SCALE_MAX, ar.POS_X), (ar.OPACITY_LOGIT, ar.LOG_SCALE_MIN, ar.DC_R)):
        attrs = [ta._attr(k) for k in kinds]
        planes = [attributes.values(r, a) for a in attrs]
        for where in ((0, 0), mr.THIRD):
            got = moments.moments(r, attrs, where)
            want = mr.restate(planes, mr.keep_of(where, st))
            assert mr.same(got, want), (kinds, where)
            assert want["counted"] < want["matched"]
    r.destroy()


def _records_of(r, n):
    """The 160 bytes of a few calls, dense and filtered."""
    from gsplat import _abi
    import test_attributes as ta
    L = _abi.load()
    o = r._state_owner() if hasattr(r, "_state_owner") else r
    out = []
    for kinds in ((ar.POS_X, ar.POS_Y, ar.POS_Z), (ar.OPACITY_LOGIT, ar.POS_Y), (ar.DIST2,)):
        arr = (_abi.GsAttr * len(kinds))(*[ta._attr(k) for k in kinds])
        for where in ((0, 0), mr.THIRD):
            rec = _abi.GsAttrMoments()
            _abi.check(L.gs_attr_moments(o._ctx, arr, len(kinds), where[0], where[1], ctypes.byref(rec)))
            out.append(bytes(rec))
    return out


def _want_records(s, st):
    import test_attributes as ta
    out = []
    for kinds in ((ar.POS_X, ar.POS_Y, ar.POS_Z), (ar.OPACITY_LOGIT, ar.POS_Y), (ar.DIST2,)):
        planes = [ar.value(k, s, ta._p(k)) for k in kinds]
        for where in ((0, 0), mr.THIRD):
            out.append(mr.restate(planes, mr.keep_of(where, st)))
    return out


def _as_bytes(want):
    from gsplat import _abi
    rec = _abi.GsAttrMoments()
    rec.matched, rec.counted = want["matched"], want["counted"]
    for j in range(3):
        rec.sum[j].hi, rec.sum[j].lo = want["sum"][j]
        for l in range(j, 3):
            rec.prod[mr.PROD[j][l]].hi, rec.prod[mr.PROD[j][l]].lo = want["prod"][j][l]
    return bytes(rec)


def _cfg_a():
    def make():
        s, u, W, H = state_scene("cfgA")
        s = np.ascontiguousarray(s[:3001])
        st = mr.third(3001)
        return s, u, W, H, st, [_as_bytes(w) for w in _want_records(s, st)]
    return cached("moments_cfgA", make)


@pytest.mark.gpu
def test_slab_and_borrower_answer_the_same():
    """Two runs agree; a slab context, a borrower of gs_share_splats and a pipelined renderer give the owner's 160 bytes."""
    s, u, W, H, st, want = _cfg_a()
    owner = _mk(s, W, H, 16)
    owner.write_state(st)
    assert _records_of(owner, 3001) == want
    assert _records_of(owner, 3001) == want
    slab = _mk(s, W, H, 16, cols=SLAB_COLS[16])
    slab.write_state(st)
    assert _records_of(slab, 3001) == want
    slab.destroy()
    borrower = _mk(s, W, H, 16, share_with=owner)
    assert _records_of(borrower, 3001) == want
    borrower.destroy()
    import gsplat
    from gsplat import _abi
    p = gsplat.PipelinedRenderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(s), 16, frames_in_flight=2, flags=_abi.GS_FLAG_SPLAT_STATE)
    p.write_state(st)
    p.render_uniforms(u)
    p.render_uniforms(u)
    assert _records_of(p, 3001) == want
    p.destroy()
    owner.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_moments_disturb_nothing(graph):
    """Three frames in flight (and again with the frame graph): the calls are made without waiting and answer right, and the next
    frame's taps, image and statistics and the state plane are those of a context that never made them."""
    from gsplat import _abi, synth
    s, u, W, H, st, want = _cfg_a()
    cams = [synth.orbit_camera(k, W, H).uniforms(W, H) for k in (1, 7, 2)]
    a, b = _mk(s, W, H, 16), _mk(s, W, H, 16)
    for r in (a, b):
        r.set_option(_abi.GS_OPT_FRAME_GRAPH, graph)
        r.write_state(st)
    for rep in range(2):
        for uu in cams:
            a.render_uniforms(uu)
            b.render_uniforms(uu)
        assert _records_of(a, 3001) == want  # (no wait in between)
        ta, tb = frame_taps(a, u, False), frame_taps(b, u, False)
        for k in ta:
            np.testing.assert_array_equal(ta[k], tb[k], err_msg=k)
        assert timeless(a.stats()) == timeless(b.stats())
        assert a.stats()["frames_in_flight"] == 3
        np.testing.assert_array_equal(a.read_state(), st)
    if graph:
        assert a.stats()["graph_frames"] == b.stats()["graph_frames"] > 0
    a.destroy()
    b.destroy()


@pytest.mark.gpu
def test_moments_refusals_and_lifecycle():
    from gsplat import _abi, attributes, moments
    L = _abi.load()
    s, u, W, H, st, _ = _cfg_a()
    n = s.shape[0]
    INV = _abi.GS_ERR_INVALID_ARGUMENT
    xyz = (_abi.GsAttr * 4)(*_attrs(ar.POS_X, ar.POS_Y, ar.POS_Z, ar.POS_X))
    out = guarded(160, np.uint8)
    po = ctypes.cast(out.ctypes.data, ctypes.POINTER(_abi.GsAttrMoments))
    # before any upload: GS_ERR_NO_SCENE; N == 0: zeros
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(_abi.GsConfig), W, H, 16, _abi.GS_FLAG_SPLAT_STATE
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    assert L.gs_attr_moments(ctx, xyz, 3, 0, 0, po) == _abi.GS_ERR_NO_SCENE
    assert is_fill(out)
    _abi.check(L.gs_upload_splats(ctx, None, 0))
    _abi.check(L.gs_attr_moments(ctx, xyz, 3, 0, 0, po))
    assert not out.any()
    L.gs_destroy(ctx)
    out.fill(0xA5)

    r = _mk(s, W, H, 16)
    r.write_state(st)

    def refused(call, *fragments):
        assert call() == INV, fragments
        msg = L.gs_last_error().decode()
        assert "gs_attr_moments" in msg and all(f in msg for f in fragments), msg
        assert is_fill(out)

    refused(lambda: L.gs_attr_moments(r._ctx, xyz, 0, 0, 0, po), "0 attributes")
    refused(lambda: L.gs_attr_moments(r._ctx, xyz, 4, 0, 0, po), "4 attributes")
    refused(lambda: L.gs_attr_moments(r._ctx, None, 1, 0, 0, po), "null attributes")
    refused(lambda: L.gs_attr_moments(r._ctx, xyz, 3, 0, 0, None), "null moments")
    refused(lambda: L.gs_attr_moments(r._ctx, xyz, 3, 0x100, 0, po), "0x100", "does not fit the state byte")
    bad = (_abi.GsAttr * 2)(attributes.attr(ar.POS_X), attributes.attr(99))
    refused(lambda: L.gs_attr_moments(r._ctx, bad, 2, 0, 0, po), "kind 99")
    _abi.check(L.gs_attr_moments(r._ctx, bad, 1, 0, 0, po))  # (the second slot is not read with n_attrs = 1)
    out.fill(0xA5)
    bad[1] = attributes.attr(ar.POS_Y)
    bad[1].struct_size = 20
    refused(lambda: L.gs_attr_moments(r._ctx, bad, 2, 0, 0, po), "struct_size 20")
    bad[1] = attributes.attr(ar.PLANE, (0, 0, 1, float("inf")))
    refused(lambda: L.gs_attr_moments(r._ctx, bad, 2, 0, 0, po), "p[3]", "not finite")
    # the centroid of a selection follows a transform; after a compaction and an append the call answers for the new scene
    lo, hi = (-1.0, -0.5, -1.0), (0.5, 1.0, 1.5)
    r.write_state(np.zeros(n, np.uint8))
    assert r.select_box(lo, hi) > 100
    r.rotate_selected((0.9, 0.1, -0.3, 0.2), pivot=moments.centroid(r).astype(F))
    r.translate_selected((0.3, -1.7, 12.5))
    rec, ids = r.export_splats(2, 2, with_ids=True)
    want = mr.restate([rec[:, 0], rec[:, 1], rec[:, 2]])
    np.testing.assert_array_equal(moments.centroid(r), [mr.mean(rec[:, j]) for j in range(3)])
    assert mr.same(moments.moments(r, _attrs(ar.POS_X, ar.POS_Y, ar.POS_Z), SEL), want)
    kept = r.compact(2, 2)
    assert kept.size == rec.shape[0]
    assert mr.same(moments.moments(r, _attrs(ar.POS_X, ar.POS_Y, ar.POS_Z)), want)
    from gsplat import insert
    insert.append(r, s[:5])
    both = np.concatenate([rec, s[:5]])
    assert mr.same(moments.moments(r, _attrs(ar.POS_X, ar.POS_Y, ar.POS_Z)), mr.restate([both[:, 0], both[:, 1], both[:, 2]]))
    r.destroy()
    # a context without the plane: (0, 0) works, any other filter is refused
    q = mk(s, W, H, 16)
    assert mr.same(moments.moments(q, _attrs(ar.POS_X, ar.POS_Y, ar.POS_Z)), mr.restate([s[:, 0], s[:, 1], s[:, 2]]))
    code, msg = code_of(lambda: moments.moments(q, _attrs(ar.POS_X), mr.THIRD))
    assert code == INV and "GS_FLAG_SPLAT_STATE" in msg and "gs_attr_moments" in msg
    q.destroy()


def _angle(a, b):
    """Between two lines (unit vectors up to sign)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return math.atan2(np.linalg.norm(np.cross(a, b)), abs(float(np.dot(a, b))))


@pytest.mark.gpu
def test_verbs():
    """centroid against centre on a scene with one far outlier; oriented_bounds holds every selected centre with no slack;
    fit_plane against numpy's SVD of the same points; align_selected diagonalises the covariance.

    The yardstick of the last two.  Both fits are backward stable: each returns the exact normal of a matrix within p eps |C| of
    the true one, eps = 2^-52, and a perturbation E turns an eigenvector by at most |E| / gap (Davis-Kahan), gap = the distance of
    the smallest eigenvalue from the next.  With p <= the number of rows m (a modest polynomial in LAPACK's bounds; the centring
    and the 2000-term sums of the SVD route are inside it) the two may disagree by Y64 = 2 m eps lambda_max / gap.  The aligned
    covariance is computed from positions that a float32 transform wrote: every coordinate is off by up to 4 roundings of 2^-24
    of the scene's reach |p|, which moves an entry of the covariance by up to 2 sqrt(lambda_max) 4 2^-24 |p|; in units of
    lambda_max that is Y32 = 8 2^-24 |p| / sqrt(lambda_max), and the off-diagonals stay below (Y64 + Y32) lambda_max.  Both are
    printed; profiles/moments.txt records what was measured."""
    from gsplat import attributes, moments
    # centroid and centre
    base = np.array(scene(10000)[:1000], dtype=F, copy=True)
    base[7, 0:3] = (900.0, -400.0, 250.0)
    r = _mk(base, 64, 64, 16)
    r.write_state(np.full(1000, 2, np.uint8))
    c = moments.centroid(r)
    np.testing.assert_array_equal(c, [mr.mean(base[:, j]) for j in range(3)])
    assert np.abs(attributes.centre(r).astype(np.float64) - c).max() > 100  # the midpoint of the bounds went with the outlier
    rest = np.delete(base[:, 0:3].astype(np.float64), 7, axis=0).mean(axis=0)
    assert np.abs(c - rest).max() < 1  # ... the centroid by a thousandth of its distance
    cov = moments.covariance(r)
    for j in range(3):
        for k in range(3):
            assert mr.bits(cov[j, k]) == mr.bits(mr.covariance(base[:, j], base[:, k]))
    a = attributes.attr(ar.POS_Y)
    assert mr.bits(moments.mean(r, a, SEL)) == mr.bits(mr.mean(base[:, 1]))
    assert mr.bits(moments.variance(r, a, SEL)) == mr.bits(mr.covariance(base[:, 1], base[:, 1]))
    assert moments.std(r, a, SEL) == math.sqrt(moments.variance(r, a, SEL))
    r.write_state(np.zeros(1000, np.uint8))
    for fn in (lambda: moments.centroid(r), lambda: moments.covariance(r), lambda: moments.principal_axes(r), lambda: moments.fit_plane(r)):
        with pytest.raises(ValueError):
            fn()
    r.destroy()
    # oriented_bounds: every selected centre inside under the attribute's own f32 expression, every face touched
    s = np.ascontiguousarray(scene(10000)[:3001])
    st = mr.third(3001)
    sel = (st & 0x04) != 0
    r = _mk(s, 64, 64, 16)
    r.write_state(st)
    ob = moments.oriented_bounds(r, mr.THIRD)
    w, axes = moments.principal_axes(r, mr.THIRD)
    assert w[0] >= w[1] >= w[2] >= 0 and abs(np.linalg.det(axes) - 1) < 1e-12
    np.testing.assert_array_equal(ob["axes"], axes.astype(F))
    for k in range(3):
        v = ar.value(ar.PLANE, s, tuple(ob["planes"][k].p))[sel]
        assert v.min() == ob["lo"][k] and v.max() == ob["hi"][k]  # contains all, and no face can move inwards
        assert ob["half"][k] == (float(ob["hi"][k]) - float(ob["lo"][k])) / 2
    r.destroy()
    # fit_plane and align_selected on a planted plane
    pts = mr.planted_plane()
    m = pts.shape[0]
    r = _mk(records(pts), 64, 64, 16)
    r.write_state(np.full(m, 2, np.uint8))
    normal, offset, rms = moments.fit_plane(r)
    p64 = pts.astype(np.float64)
    mid = p64.mean(axis=0)
    svd_normal = np.linalg.svd(p64 - mid)[2][2]
    lam = np.linalg.eigvalsh(np.cov(p64.T, bias=True))[::-1]
    y64 = 2 * m * 2.0 ** -52 * lam[0] / (lam[1] - lam[2])
    angle = _angle(normal, svd_normal)
    print("fit_plane: angle to the SVD normal %.3e rad, yardstick Y64 %.3e; rms %.6e" % (angle, y64, rms))
    assert angle <= y64
    truth = np.array([0.3, -0.2, -1.0]) / np.linalg.norm([0.3, -0.2, -1.0])
    assert _angle(normal, truth) < 5 * 1e-3 / math.sqrt(m)  # the planted plane, within the noise's own uncertainty
    assert abs(offset + float(np.dot(normal, mid))) < 1e-12 and abs(rms - math.sqrt(lam[2])) < 1e-9
    reach = float(np.abs(p64).max())
    y32 = 8 * 2.0 ** -24 * reach / math.sqrt(lam[0])
    assert moments.align_selected(r) == m
    cov = moments.covariance(r)
    off = max(abs(cov[0, 1]), abs(cov[0, 2]), abs(cov[1, 2]))
    print("align_selected: largest off-diagonal %.3e of lambda_max, yardstick Y64 + Y32 %.3e" % (off / lam[0], y64 + y32))
    assert off <= (y64 + y32) * lam[0]
    assert cov[0, 0] >= cov[1, 1] >= cov[2, 2]
    np.testing.assert_allclose(moments.centroid(r), mid, atol=4 * 2.0 ** -24 * reach)  # the pivot stays
    r.destroy()
