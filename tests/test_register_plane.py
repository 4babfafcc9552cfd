"""Point-to-plane registration (gs_abi.h "registration"): gs_pair_plane_moments and gs_pair_plane_moments_host against the restatement of
tests/plane_pairs_restate.py, bit for bit on hi and lo and on both counts; fit_plane, plane_step and align(metric="plane") of
gsplat.register."""
import ctypes
import functools
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import knn_restate
import moments_restate as mr
import pairs_restate as pr
import plane_pairs_restate as pp
import test_register as tr
import xform_restate as xr
from support import F, ROOT, SLAB_COLS, c_layout, cached, code_of, guarded, is_fill, mk, timeless

_mk = functools.partial(mk, state=True)
CSRC = tr.CSRC
SEL, REST = (2, 2), (2, 0)
KINDS = ("scene", "far", "spread", "nonfinite", "cancel")
LENGTHS = (1, 3, 5, 1023, 1025, 1043)
CELLS = [(k, n) for k in KINDS for n in LENGTHS]
PARTNERS = ("nearest", "perm", "beyond")
PIVOTS = ((0.0, 0.0, 0.0), (1.0e4, -3.0e3, 77.5))
INF = float("inf")


def positions(kind, n):
    """test_register's position kinds; `nonfinite` is a fixed scene of 1043 splats, cut to n."""
    return np.ascontiguousarray(tr.positions(kind, 1043)[:n]) if kind == "nonfinite" else tr.positions(kind, n)


def partner(kind, n, pk):
    return cached(("plane_partner", kind, n, pk), lambda: pr.partner(pk, positions(kind, n)))


def normals(nk, n):
    return cached(("plane_normals", nk, n), lambda: pp.normals(nk, n))


def columns(kind, n, pk, nk, pivot):
    """The restatement's per-splat terms of one case, computed once and shared by the CPU and the GPU tests."""
    return cached(("plane_columns", kind, n, pk, nk, pivot), lambda: pp.columns(positions(kind, n), partner(kind, n, pk), normals(nk, n), pivot))


def cases():
    """[(partner kind, normal kind, pivot, filter)]: every partner kind with every normal plane about the zero pivot and a far one,
    without a filter and with the one that keeps a third."""
    return [(pk, nk, pivot, where) for pk in PARTNERS for nk in pp.NORMALS for pivot in PIVOTS for where in ((0, 0), mr.THIRD)]


def want_of(kind, n, pk, nk, pivot, where, max_d2=INF):
    return pp.record(columns(kind, n, pk, nk, pivot), mr.keep_of(where, mr.third(n)), max_d2)


def _pivot3(pivot):
    return (ctypes.c_float * 3)(*[float(v) for v in pivot])


def _host(pos, part, nrm, st, where, pivot, max_d2):
    """gs_pair_plane_moments_host with max_dist2 given as it is (the Python wrapper squares a distance)."""
    from gsplat import _abi, register
    planes = [np.ascontiguousarray(pos[:, a]) for a in range(3)]
    out = _abi.GsPairPlaneMoments()
    _abi.check(_abi.load().gs_pair_plane_moments_host(planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, pos.shape[0], part.ctypes.data,
                                                      nrm.ctypes.data, None if st is None else st.ctypes.data, where[0], where[1], _pivot3(pivot),
                                                      float(max_d2), ctypes.byref(out)))
    return register._plane_result(out), bytes(out)


def _dev(r, where, pivot, max_d2=INF, part=None, nrm=None):
    """gs_pair_plane_moments likewise: (the record as a dict, its 480 bytes)."""
    from gsplat import _abi, register
    o = r._state_owner() if hasattr(r, "_state_owner") else r
    out = _abi.GsPairPlaneMoments()
    _abi.check(o._L.gs_pair_plane_moments(o._ctx, where[0], where[1], None if part is None else part.ctypes.data,
                                          None if nrm is None else nrm.ctypes.data, _pivot3(pivot), float(max_d2), ctypes.byref(out)))
    return register._plane_result(out), bytes(out)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_plane_abi(tmp_path):
    """Both symbols are exported without a GPU and listed; gs_pair_plane_moments is 480 bytes and every offset agrees between the
    compiled header and ctypes; the version is still 3; a null ctx and the host call's bad arguments -- a null or non-finite pivot
    among them -- are refused with the call's name and the record untouched; n == 0 gives zeros; the renderer classes gained no
    public method."""
    from gsplat import _abi, register, renderer
    L = _abi.load()
    for name in ("gs_pair_plane_moments", "gs_pair_plane_moments_host"):
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    assert L.gs_abi_version() == 3
    fm = [n for n, _ in _abi.GsPairPlaneMoments._fields_]
    prog = 'printf("%zu", sizeof(struct gs_pair_plane_moments));'
    prog += "".join('printf(" %%zu", offsetof(struct gs_pair_plane_moments, %s));' % n for n in fm)
    prog += 'printf(" %u", (unsigned)GS_ABI_VERSION);'
    out = c_layout(tmp_path, "plane_layout", prog)
    assert out[0] == ctypes.sizeof(_abi.GsPairPlaneMoments) == 480
    assert out[1:7] == [getattr(_abi.GsPairPlaneMoments, n).offset for n in fm] == [0, 8, 16, 352, 448, 464]
    assert out[7] == 3
    rec = guarded(480, np.uint8)
    po = ctypes.cast(rec.ctypes.data, ctypes.POINTER(_abi.GsPairPlaneMoments))
    P = _pivot3((0, 0, 0))
    assert L.gs_pair_plane_moments(None, 0, 0, None, None, P, 1.0, po) == _abi.GS_ERR_INVALID_ARGUMENT
    assert b"gs_pair_plane_moments" in L.gs_last_error() and b"null ctx" in L.gs_last_error()
    x, ids, st, nr = np.arange(4, dtype=F), np.arange(4, dtype=np.uint32), np.zeros(4, np.uint8), np.ones(12, F)
    X, I, S, N = x.ctypes.data, ids.ctypes.data, st.ctypes.data, nr.ctypes.data
    bad = [_pivot3(v) for v in ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, float("-inf")))]
    for args, fragment in (((None, X, X, 4, I, N, None, 0, 0, P, 1.0, po), "null position plane"), ((X, X, None, 4, I, N, None, 0, 0, P, 1.0, po), "null position plane"),
                           ((X, X, X, 4, None, N, None, 0, 0, P, 1.0, po), "null partner"), ((X, X, X, 4, I, None, None, 0, 0, P, 1.0, po), "null normal"),
                           ((X, X, X, 4, I, N, None, 4, 4, P, 1.0, po), "null state"),
                           ((X, X, X, 4, I, N, S, 0x100, 0, P, 1.0, po), "does not fit the state byte"), ((X, X, X, 4, I, N, S, 0, 0, P, float("nan"), po), "max_dist2"),
                           ((X, X, X, 4, I, N, S, 0, 0, P, -1.0, po), "max_dist2"), ((X, X, X, 1 << 31, I, N, S, 0, 0, P, 1.0, po), "2^31"),
                           ((X, X, X, 4, I, N, S, 0, 0, None, 1.0, po), "null pivot"), ((X, X, X, 4, I, N, S, 0, 0, bad[0], 1.0, po), "pivot[0]"),
                           ((X, X, X, 4, I, N, S, 0, 0, bad[1], 1.0, po), "pivot[1]"), ((X, X, X, 4, I, N, S, 0, 0, bad[2], 1.0, po), "pivot[2]"),
                           ((X, X, X, 4, I, N, S, 0, 0, P, 1.0, None), "null moments")):
        assert L.gs_pair_plane_moments_host(*args) == _abi.GS_ERR_INVALID_ARGUMENT, fragment
        msg = L.gs_last_error().decode()
        assert "gs_pair_plane_moments_host" in msg and fragment in msg, msg
    assert is_fill(rec)
    # n == 0: zeros; -0.0 is a valid bound
    empty = register.host_pair_plane_moments(np.zeros((0, 3), F), np.zeros(0, np.uint32), np.zeros((0, 3), F))
    assert pp.same(empty, pp.restate(np.zeros((0, 3), F), np.zeros(0, np.uint32), np.zeros((0, 3), F))) and empty["matched"] == 0
    assert all(mr.bits(v) == 0 for e in pp.flat(empty) for v in e)
    two = _host(np.zeros((2, 3), F), np.array([1, 0], np.uint32), np.ones((2, 3), F), None, (0, 0), (0, 0, 0), -0.0)[0]
    assert two["paired"] == 2
    import test_abi
    for cname in ("Renderer", "PipelinedRenderer"):
        live = {n for n in vars(getattr(renderer, cname)) if not n.startswith("_") and callable(getattr(getattr(renderer, cname), n))}
        assert live == set(test_abi.PYTHON_HOST_SURFACE[cname]) - {"__init__"}
    assert "design choice" in register.fit_plane.__doc__ and "surface.estimate" in register.plane_step.__doc__


def test_plane_restatement_is_pinned():
    """The integer columns of plane_pairs_restate against the term-by-term Fraction sum."""
    for kind, n in (("scene", 1025), ("far", 1023), ("spread", 1043), ("nonfinite", 1043), ("cancel", 5)):
        pos, keep = positions(kind, n), mr.keep_of(mr.THIRD, mr.third(n))
        for pk, nk, pivot in (("nearest", "unit", PIVOTS[1]), ("perm", "huge", PIVOTS[0]), ("beyond", "nan_third", PIVOTS[1])):
            want = pp.by_fractions(pos, partner(kind, n, pk), normals(nk, n), keep, pivot=pivot)
            assert pp.same(pp.record(columns(kind, n, pk, nk, pivot), keep), want), (kind, pk, nk)


@pytest.mark.parametrize("kind,n", CELLS)
def test_host_pair_plane_moments(kind, n):
    """gs_pair_plane_moments_host on every position kind and length (quad boundary, partial last quad, tiny), partner kind (nearest, a
    permutation, ids at and past N), normal plane (unit; NaN for a third; un-normalised and huge, where c or r overflows and the pair
    is dropped), pivot (zero, far) and filter; the nearest partners also at a d2 that occurs (inclusive) and just below it; through the
    Python wrapper."""
    from gsplat import register
    pos, st = positions(kind, n), mr.third(n)
    for pk, nk, pivot, where in cases():
        got, _ = _host(pos, partner(kind, n, pk), normals(nk, n), st, where, pivot, INF)
        assert pp.same(got, want_of(kind, n, pk, nk, pivot, where)), (kind, n, pk, nk, pivot, where)
    valid, d2, _ = columns(kind, n, "nearest", "unit", PIVOTS[0])
    if valid.any():
        med = np.sort(d2[valid])[valid.sum() // 2]
        for d in (med, np.nextafter(med, F(-1))) if med > 0 else (med,):
            got, _ = _host(pos, partner(kind, n, "nearest"), normals("unit", n), st, (0, 0), PIVOTS[0], d)
            assert pp.same(got, want_of(kind, n, "nearest", "unit", PIVOTS[0], (0, 0), d)), (kind, n, d)
        if med > 0:
            assert want_of(kind, n, "nearest", "unit", PIVOTS[0], (0, 0), med)["paired"] > want_of(kind, n, "nearest", "unit", PIVOTS[0], (0, 0), np.nextafter(med, F(-1)))["paired"]
    got = register.host_pair_plane_moments(pos, partner(kind, n, "perm"), normals("unit", n), st, mr.THIRD, pivot=PIVOTS[1])
    assert pp.same(got, want_of(kind, n, "perm", "unit", PIVOTS[1], mr.THIRD))
    got = register.host_pair_plane_moments(pos, partner(kind, n, "perm"), normals("unit", n))  # no state plane at all
    assert pp.same(got, want_of(kind, n, "perm", "unit", PIVOTS[0], (0, 0)))
    if n >= 1023:
        full, third, huge = (want_of(kind, n, "perm", nk, PIVOTS[0], (0, 0)) for nk in pp.NORMALS)
        assert full["paired"] > third["paired"] > 0.5 * full["paired"]  # a NaN normal: matched, not paired
        if kind == "far":  # lever arms of 1e4 against normals of up to 2^126
            assert full["paired"] > huge["paired"] > 0  # an overflowed c or r drops the pair


def test_edge_rules():
    """Each rule by its own small case: a NaN partner normal leaves the splat matched but not paired; j == i pairs with r = 0 and
    d2 = 0; an overflowed d2 passes only max_dist2 = +inf (and then counts as 2^128); an exact zero sum is {+0.0, +0.0}; an id at or
    past N is never read."""
    from gsplat import register
    Z = (0.0, 0.0, 0.0)
    pos = np.array([[0, 0, 0], [1, 2, 2], [5, 5, 5], [2e19, 0, 0], [-2e19, 0, 0]], F)
    up = np.tile(np.array([0, 0, 1], F), (5, 1))
    nan = up.copy()
    nan.view(np.uint32)[1] = knn_restate.NAN_BITS
    part = np.array([1, 0, 1, 4, 3], np.uint32)
    for nrm, paired in ((up, 5), (nan, 3)):  # with splat 1's normal NaN, 0 -> 1 and 2 -> 1 are matched, not paired
        got, _ = _host(pos, part, nrm, None, (0, 0), Z, INF)
        assert (got["matched"], got["paired"]) == (5, paired) and pp.same(got, pp.restate(pos, part, nrm))
    # the overflowed d2 of 3 <-> 4 (4e19 squared) passes +inf only; then the d2 sum holds 2 x 2^128 + 9 + 9 + 34
    got, _ = _host(pos, part, up, None, (0, 0), Z, F(3.0e38))
    assert got["paired"] == 3 and pp.same(got, pp.restate(pos, part, up, None, F(3.0e38)))
    got, _ = _host(pos, part, up, None, (0, 0), Z, INF)
    assert register.exact(got["d2"]) == 2 * Fraction(2) ** 128 + 9 + 9 + 34 and got["paired"] == 5
    # j == i: r = 0 and d2 = 0 at the bound 0: h, rr and d2 are exact zeros, +0.0 in both halves; G is not
    me = np.arange(5, dtype=np.uint32)
    got, _ = _host(pos, me, up, None, (0, 0), (1.0, 1.0, 1.0), 0.0)
    assert got["paired"] == 5 and pp.same(got, pp.restate(pos, me, up, None, F(0), (1.0, 1.0, 1.0)))
    assert all(mr.bits(v) == 0 for e in got["h"] + [got["rr"], got["d2"]] for v in e)
    assert register.exact(got["G"][5][5]) == 5 and register.exact(got["G"][0][0]) > 0
    # ids at and past N: arrays of exactly N elements, nothing paired, every sum +0.0
    past = np.array([5, 6, 1 << 31, pr.NONE - 1, pr.NONE], np.uint32)
    got, _ = _host(pos, past, up, None, (0, 0), Z, INF)
    assert (got["matched"], got["paired"]) == (5, 0) and all(mr.bits(v) == 0 for e in pp.flat(got) for v in e)


# ---- the fit -------------------------------------------------------------------------------------------------------------------------
def _patches(offset, rng, m=18, s=0.1, jitter=0.2, shift=(0.0, 0.0, 0.0)):
    """Three mutually non-parallel planar patches (z = 0, x = -1 and a plane tilted by 53 degrees about x), well apart, each an m x m
    lattice of spacing s whose nodes sit at (i + offset + jitter) s."""
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    frames = ((np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])),
              (np.array([-1.0, 0.0, 0.5]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0])),
              (np.array([0.5, -1.0, 1.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.6, 0.8])))
    out = []
    for k, (o, e1, e2) in enumerate(frames):
        uv = (g + offset[k] + rng.uniform(-jitter, jitter, g.shape)) * s
        out.append(o + uv[:, :1] * e1 + uv[:, 1:] * e2 + np.asarray(shift))
    return np.concatenate(out)


SPACING = 0.1
PLANE = dict(radius=4 * SPACING, normal_radius=3 * SPACING)


def patch_scene(shift=(0.0, 0.0, 0.0)):
    """972 fixed splats on the three patches and a moving copy of 972 sampled at DIFFERENT lattice offsets (about half a spacing),
    turned by 2 degrees about its centroid and shifted by (0.3, -0.25, 0.2) spacings: within the radius of four spacings.  `truth`:
    where the moving splats belong."""
    def make():
        from gsplat import _abi
        rng = np.random.default_rng(7)
        fixed = _patches(np.zeros((3, 2)), rng, shift=shift).astype(F)
        truth = _patches(np.array([[0.5, 0.5], [0.37, 0.61], [0.55, 0.43]]), rng, shift=shift).astype(F)
        st = np.concatenate([np.zeros(fixed.shape[0], np.uint8), np.full(truth.shape[0], 2, np.uint8)])
        X = _abi.compose_xform(rot=xr.axis_angle((0.3, -0.5, 0.81), np.radians(2.0)), translate=(0.03, -0.025, 0.02),
                               pivot=truth.astype(np.float64).mean(axis=0))
        base = tr.records(np.concatenate([fixed, truth]))
        rec0 = xr.apply(base, xr.Xform.from_struct(X), st == 2)
        return dict(rec0=rec0, st=st, truth=truth, normal=pp.fixed_normals(rec0, st, PLANE["normal_radius"]))
    return cached(("plane_patch_scene", tuple(shift)), make)


def _pose_error(rec, sc):
    """rms distance of the moving splats to where they belong."""
    mov = sc["st"] == 2
    return float(np.sqrt(((rec[mov, 0:3].astype(np.float64) - sc["truth"].astype(np.float64)) ** 2).sum(axis=1).mean()))


def test_fit_plane_against_float64():
    """fit_plane against numpy.linalg.lstsq on the rows of the same pairs held in float64 (the f32 rows the definition forms,
    promoted): x to 1e-9 of its largest component -- test_fit_against_float64's margin for the same reason: both are solutions of one
    well-conditioned least-squares problem (eigenvalue ratio about 0.05, printed), one exact and rounded once, one in double.
    Measured on these scenes (near the origin, and 1e4 away with the pivot at the centroid): 1.4e-15 of the largest component on both.
    The quaternion is that of the rotation vector; rms_plane, rms and predicted equal their Fraction restatements bit for bit; fewer
    than 6 pairs raise."""
    from gsplat import register
    for shift in ((0.0, 0.0, 0.0), (1.0e4, -1.0e4, 1.0e4)):
        sc = patch_scene(shift)
        rec, st = sc["rec0"], sc["st"]
        mov, fix = pr.masks(st, SEL, REST)
        near = knn_restate.planes(rec, 1, PLANE["radius"], src=fix, qry=mov)[1]
        c = pp.centroid32(rec, mov)
        m = register.host_pair_plane_moments(rec, near, sc["normal"], st, SEL, pivot=c)
        assert pp.same(m, pp.restate(rec[:, :3], near, sc["normal"], mov, INF, c)) and m["paired"] == 972
        f = register.fit_plane(m, c)
        valid, d2, rows = pp.rows(rec[:, :3], near, sc["normal"], c)
        keep = valid & mov
        A, b = rows[keep, 0:6].astype(np.float64), rows[keep, 6].astype(np.float64)
        x64 = np.linalg.lstsq(A, b, rcond=None)[0]
        diff = np.abs(f["x"] - x64).max() / np.abs(x64).max()
        print("shift", shift, "eigen ratio %.3g" % (f["eigen"][0] / f["eigen"][-1]), "max |x - x64| / max |x64| = %.3e" % diff)
        assert f["eigen"][0] > 1e-3 * f["eigen"][-1] and diff <= 1e-9
        theta = math.sqrt(float((f["x"][0:3] ** 2).sum()))
        assert abs(2 * math.acos(f["rot"][0]) - theta) < 1e-9 and abs(sum(v * v for v in f["rot"]) - 1) < 1e-15
        np.testing.assert_array_equal(f["translate"], f["x"][3:6])
        np.testing.assert_array_equal(f["pivot"], c.astype(np.float64))
        assert f["scale"] == 1.0 and 0.8 * math.radians(2.0) < theta < 1.2 * math.radians(2.0)  # one step nearly undoes the 2 degrees
        n = m["paired"]
        rr, dd = register.exact(m["rr"]), register.exact(m["d2"])
        assert mr.bits(f["rms_plane"]) == mr.bits(math.sqrt(float(rr / n))) and mr.bits(f["rms"]) == mr.bits(math.sqrt(float(dd / n)))
        direct = math.sqrt(float((b * b).sum() / n))
        assert abs(f["rms_plane"] - direct) <= 1e-12 * direct
        res = math.sqrt(float(((b - A @ x64) ** 2).sum() / n))  # the model's own residual: what "predicted" predicts
        assert abs(f["predicted"] - res) <= 1e-6 * res
        assert register.xform_of(f) is not None
    few = register.host_pair_plane_moments(np.zeros((5, 3), F), np.arange(5, dtype=np.uint32), np.ones((5, 3), F))
    assert few["paired"] == 5
    with pytest.raises(ValueError, match="5 pairs"):
        register.fit_plane(few, (0, 0, 0))


def test_degenerate_normals():
    """All normals bit-equal (one plane): with damping == 0 a ValueError that names the eigenvalues; with damping > 0 a solution whose
    translation along the two free directions and whose rotation about the normal are EXACTLY 0.  The scene: a lattice on z = 0, its
    moving copy at the same x and y (p = q tangentially), lifted and tilted in z only; normals (0, 0, 1): g = (uy, -ux, 0, 0, 0, 1), so
    rows and columns 2, 3, 4 of G and h are exact zeros and the rational solve leaves x[2] = x[3] = x[4] = 0."""
    from gsplat import register
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2).astype(np.float64) * 0.25
    fixed = np.column_stack([g, np.zeros(g.shape[0])]).astype(F)
    moving = np.column_stack([g, 0.05 + 0.01 * g[:, 0] - 0.02 * g[:, 1]]).astype(F)
    n = fixed.shape[0]
    pos = np.concatenate([fixed, moving])
    part = np.concatenate([np.full(n, pr.NONE), np.arange(n)]).astype(np.uint32)
    st = np.concatenate([np.zeros(n), np.full(n, 2)]).astype(np.uint8)
    nrm = np.tile(np.array([0, 0, 1], F), (2 * n, 1))
    c = pp.centroid32(pos, st == 2)
    m = register.host_pair_plane_moments(pos, part, nrm, st, SEL, pivot=c)
    assert m["paired"] == n
    with pytest.raises(ValueError, match="eigenvalues"):
        register.fit_plane(m, c)
    f = register.fit_plane(m, c, damping=1e-3)
    assert f["x"][2] == 0.0 and f["x"][3] == 0.0 and f["x"][4] == 0.0 and f["translate"][0] == 0.0 and f["translate"][1] == 0.0
    assert f["rot"][3] == 0.0 and f["x"][5] < -0.03 and abs(f["x"][0]) > 1e-3 and abs(f["x"][1]) > 1e-3  # it does move along z and tilt
    assert f["predicted"] < 0.1 * f["rms_plane"] and f["eigen"][0] > 0


STEPS = 6


def convergence():
    """Both metrics for STEPS steps on patch_scene() with align's trimming, host twins only: knn_restate, surface.host_estimate,
    host_pair_plane_moments (through the restated step, which the restatement test pins to it), xform_restate."""
    def make():
        from gsplat import register
        sc = patch_scene()
        out = {}
        for metric in ("plane", "point"):
            rec, prev = sc["rec0"], None
            for _ in range(STEPS):
                md = PLANE["radius"] if prev is None else min(PLANE["radius"], 3.0 * prev)
                if metric == "plane":
                    mov, fix = pr.masks(sc["st"], SEL, REST)
                    near = knn_restate.planes(rec, 1, PLANE["radius"], src=fix, qry=mov)[1]
                    c = pp.centroid32(rec, mov)
                    f = register.fit_plane(register.host_pair_plane_moments(rec, near, sc["normal"], sc["st"], SEL, md, c), c)
                    rec = xr.apply(rec, xr.Xform.from_struct(register.xform_of(f)), mov)
                else:
                    rec, f, _ = pr.step(rec, sc["st"], PLANE["radius"], max_dist=md)
                prev = f["rms"]
            out[metric] = _pose_error(rec, sc)
        out["initial"] = _pose_error(sc["rec0"], sc)
        return out
    return cached("plane_convergence", make)


def test_plane_converges_where_point_stalls():
    """The reason for the feature.  Three non-parallel planar patches on jittered lattices of spacing 0.1; the moving copy is sampled
    at different lattice offsets and displaced by 2 degrees and a third of a spacing (pose error 6.2e-2 rms).  After 6 steps each,
    computed on the CPU: the point metric is left at 4.8e-2 (it pulls every splat to a lattice node that is not its own: the
    tangential part of each pair is sampling noise), the plane metric at 1.8e-7 (f32 rounding of the positions) -- a factor of 2.7e5,
    where the test was to be chosen for at least 4.  Asserted: plane < point / 2."""
    got = convergence()
    print("pose error: initial %.3e, point %.3e, plane %.3e" % (got["initial"], got["point"], got["plane"]))
    assert got["plane"] < got["point"] / 2.0
    assert got["plane"] < 1e-3 * got["initial"]


def test_sanitized_plane_program(tmp_path):
    """tools/plane_pairs_check: gs_plane_pair_host.h compiled alone with -fsanitize=address,undefined and run as its own process; it
    runs the pairing loop over its partner planes (all NONE, ids >= N, every id equal, j == i) and normal planes (unit, NaN, huge) in
    two orders of summation and compares the limbs, and prints the record of a file's scene, which must be the restatement's.  Skipped
    where the sanitizer runtime is not installed."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed")
    exe = str(tmp_path / "plane_pairs_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san +
                          ["-I", CSRC, os.path.join(ROOT, "tools", "plane_pairs_check", "main.cpp"), "-o", exe])
    for kind, n, pk, nk, pivot in (("nonfinite", 1043, "beyond", "nan_third", PIVOTS[1]), ("spread", 1025, "perm", "huge", PIVOTS[0]),
                                   ("far", 1023, "nearest", "unit", PIVOTS[1])):
        pos, part, nrm = positions(kind, n), partner(kind, n, pk), normals(nk, n)
        path = tmp_path / (kind + ".txt")
        rows = np.column_stack([pos.view(np.uint32), part, nrm.view(np.uint32)])
        head = "%d\n" % n + " ".join("%08x" % int(w) for w in np.asarray(pivot, F).view(np.uint32)) + "\n"
        path.write_text(head + "\n".join(" ".join("%08x" % int(w) for w in row) for row in rows) + "\n")
        out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")
        assert lines[0] == "plane_pairs_check ok"
        want = want_of(kind, n, pk, nk, pivot, (0, 0))
        assert lines[1] == "matched %d paired %d" % (want["matched"], want["paired"])
        got = [tuple(int(x, 16) for x in ln.split()) for ln in lines[2:31]]
        assert got == [(mr.bits(hi), mr.bits(lo)) for hi, lo in pp.flat(want)], kind


# ---- the scenes of the step and of the loop: built on the CPU, checked on the CPU ----------------------------------------------------
def step_want():
    def make():
        sc = patch_scene()
        out, f, near = pp.step(sc["rec0"], sc["st"], PLANE["radius"], sc["normal"])
        return dict(out=out, fit=f, near=near)
    return cached("plane_step_want", make)


def align_want():
    def make():
        sc = patch_scene()
        out, steps = pp.align(sc["rec0"], sc["st"], PLANE["radius"], PLANE["normal_radius"], max_iters=3)
        return dict(out=out, steps=steps)
    return cached("plane_align_want", make)


def test_restated_plane_step_and_loop():
    """What the GPU tests rely on, asserted on the restatement alone: the step pairs every moving splat, every fixed normal is
    resolved and no moving one is; three steps of the loop bring the plane rms from 2.7e-2 to f32 rounding, and the second step is
    trimmed by the first's point rms."""
    sc, w = patch_scene(), step_want()
    mov = sc["st"] == 2
    assert w["fit"]["paired"] == 972 and (w["near"][~mov] == pr.NONE).all() and (w["near"][mov] < 972).all()
    assert np.isfinite(sc["normal"][~mov]).all() and np.isnan(sc["normal"][mov]).all()
    steps = align_want()["steps"]
    print("align: rms_plane per step", [f["rms_plane"] for f in steps], "rms", [f["rms"] for f in steps])
    assert len(steps) == 3 and steps[2]["rms_plane"] < 1e-4 * steps[0]["rms_plane"]
    assert steps[0]["max_dist"] == PLANE["radius"] and steps[1]["max_dist"] == min(PLANE["radius"], 3.0 * steps[0]["rms"])
    assert _pose_error(align_want()["out"], sc) < 1e-5


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
BIG = 70001  # 1 mod 4: 69 workgroups' worth of quads and a partial last quad


def _big():
    """70001 splats (more than one workgroup; with GS_OPT_PERSISTENT_GRID 1 more than one trip), a permutation with ids past N, unit
    normals with NaN for a third: (positions, partner, normal, state, the restated record over the third, that of the host twin)."""
    def make():
        rng = np.random.default_rng(53)
        pos = (rng.normal(size=(BIG, 3)) * np.array([3.0, 2.0, 1.0])).astype(F)
        part, nrm, st = pr.partner("perm", pos), pp.normals("nan_third", BIG), mr.third(BIG)
        part[1::7] = np.resize(np.array([BIG, BIG + 1, 1 << 31, pr.NONE - 1, pr.NONE], np.uint64), part[1::7].size).astype(np.uint32)
        want = pp.restate(pos, part, nrm, mr.keep_of(mr.THIRD, st), INF, PIVOTS[1])
        host, raw = _host(pos, part, nrm, st, mr.THIRD, PIVOTS[1], INF)
        return pos, part, nrm, st, want, host, raw
    return cached("plane_big", make)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 5, 1023, 1025, 1043))
def test_plane_moments_host_arrays(n):
    """gs_pair_plane_moments with HOST partner and normal arrays == the host twin == the restatement, on every case of
    test_host_pair_plane_moments for the `scene` and `spread` positions; twice in a row, and with GS_OPT_PERSISTENT_GRID 1, the same
    480 bytes."""
    from gsplat import _abi, register
    for kind in ("scene", "spread"):
        pos, st = positions(kind, n), mr.third(n)
        r = _mk(tr.records(pos), 64, 64, 16)
        r.write_state(st)
        seen = {}
        for grid in (0, 1):
            if grid:
                r.set_option(_abi.GS_OPT_PERSISTENT_GRID, grid)
            for pk, nk, pivot, where in cases():
                got, raw = _dev(r, where, pivot, INF, partner(kind, n, pk), normals(nk, n))
                assert pp.same(got, want_of(kind, n, pk, nk, pivot, where)), (kind, n, pk, nk, pivot, where, grid)
                assert raw == _host(pos, partner(kind, n, pk), normals(nk, n), st, where, pivot, INF)[1]
                assert seen.setdefault((pk, nk, pivot, where), raw) == raw
        got = register.pair_plane_moments(r, mr.THIRD, INF, PIVOTS[1], partner(kind, n, "perm"), normals("unit", n))
        assert pp.same(got, want_of(kind, n, "perm", "unit", PIVOTS[1], mr.THIRD))
        r.destroy()


@pytest.mark.gpu
def test_plane_moments_many_workgroups():
    """70001 splats: device record == host twin == restatement bit for bit; two runs agree; GS_OPT_PERSISTENT_GRID 1 (one workgroup,
    69 trips per thread) and the default agree."""
    from gsplat import _abi
    pos, part, nrm, st, want, host, host_raw = _big()
    assert pp.same(host, want) and 0 < want["paired"] < want["matched"]
    r = _mk(_records_of(pos), 64, 64, 16)
    r.write_state(st)
    got, raw = _dev(r, mr.THIRD, PIVOTS[1], INF, part, nrm)
    assert pp.same(got, want) and raw == host_raw == pp.as_bytes(want)
    assert _dev(r, mr.THIRD, PIVOTS[1], INF, part, nrm)[1] == raw
    r.set_option(_abi.GS_OPT_PERSISTENT_GRID, 1)
    assert _dev(r, mr.THIRD, PIVOTS[1], INF, part, nrm)[1] == raw
    r.destroy()


def _records_of(pos):
    """Records with the given centres and one splat's other attributes throughout (any count)."""
    rec = np.repeat(np.array(tr.records(pos[:1]), dtype=F), pos.shape[0], axis=0)
    rec[:, 0:3] = pos
    return np.ascontiguousarray(rec)


def _own(n):
    """The `scene` positions of n splats with a radius that holds the whole scene: (records, state, radius)."""
    pos = positions("scene", n)
    lo, hi = pos.min(axis=0).astype(np.float64), pos.max(axis=0).astype(np.float64)
    return tr.records(pos), mr.third(n), 2.0 * float(np.linalg.norm(hi - lo)) + 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 5, 1023, 1025, 1043))
def test_plane_moments_own_planes(n):
    """partner == NULL and normal == NULL.  Never-estimated planes: GS_OK, paired == 0 and all-zero sums, also with a host partner
    array.  After a real nearest.search and surface.estimate: the restatement of the planes the searches left (knn_restate and
    gs_surface_host restate those), == the host twin."""
    from gsplat import nearest, surface
    rec, st, radius = _own(n)
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    got, raw = _dev(r, mr.THIRD, PIVOTS[0])
    assert (got["matched"], got["paired"]) == (int(((st & 4) == 4).sum()), 0) and raw[16:] == bytes(464)
    got, raw = _dev(r, (0, 0), PIVOTS[0], INF, partner("scene", n, "perm"))  # partners, but no normal was ever estimated
    assert (got["matched"], got["paired"]) == (n, 0) and raw[16:] == bytes(464)
    nearest.search(r, 1, radius)
    surface.estimate(r, radius)
    near, nrm = nearest.read(r)[1], surface.read(r)[0]
    np.testing.assert_array_equal(near, knn_restate.planes(rec, 1, radius)[1])
    np.testing.assert_array_equal(nrm.view(np.uint32), surface.host_estimate(rec[:, :3], radius)[0].view(np.uint32))
    for where in ((0, 0), mr.THIRD):
        for pivot in PIVOTS:
            got, raw = _dev(r, where, pivot)
            want = pp.restate(rec[:, :3], near, nrm, mr.keep_of(where, st), INF, pivot)
            assert pp.same(got, want) and raw == pp.as_bytes(want), (n, where, pivot)
            assert raw == _host(np.ascontiguousarray(rec[:, :3]), near, nrm, st, where, pivot, INF)[1]
    if n >= 1023:
        assert want["paired"] == want["matched"] > 0  # every normal is resolved at this radius
    r.destroy()


def _cfg_records(r):
    """The 480 bytes of a few calls on the ctx's own planes after a search and an estimate over cfgA's 3001 splats, and of one with
    host arrays."""
    from gsplat import nearest, surface
    s, _, _, _, st, small, whole = tr._cfg_a()
    nearest.search(r, 1, 4.0 * small, source=(0, 0), query=mr.THIRD)
    surface.estimate(r, 8.0 * small)
    out = [_dev(r, where, pivot, md)[1] for where in ((0, 0), mr.THIRD) for pivot in PIVOTS for md in (INF, F(2.0 * small) ** 2)]
    out.append(_dev(r, mr.THIRD, PIVOTS[1], INF, pr.partner("perm", s[:, 0:3]), pp.normals("nan_third", 3001))[1])
    return out


def _cfg_want():
    def make():
        from gsplat import surface
        s, _, _, _, st, small, whole = tr._cfg_a()
        near = knn_restate.planes(s, 1, 4.0 * small, qry=mr.keep_of(mr.THIRD, st))[1]
        nrm = surface.host_estimate(np.ascontiguousarray(s[:, 0:3]), 8.0 * small)[0]
        out = [pp.as_bytes(pp.restate(s[:, 0:3], near, nrm, mr.keep_of(where, st), md, pivot))
               for where in ((0, 0), mr.THIRD) for pivot in PIVOTS for md in (INF, F(2.0 * small) ** 2)]
        full = pp.restate(s[:, 0:3], near, nrm, mr.keep_of(mr.THIRD, st))
        assert 0 < full["paired"] < full["matched"]  # some queries have no partner in the radius, or a partner without a normal
        return out + [pp.as_bytes(pp.restate(s[:, 0:3], pr.partner("perm", s[:, 0:3]), pp.normals("nan_third", 3001), mr.keep_of(mr.THIRD, st), INF, PIVOTS[1]))]
    return cached("plane_cfg_want", make)


@pytest.mark.gpu
def test_plane_slab_borrower_and_pipeline_answer_the_same():
    """A slab context, a borrower of gs_share_splats -- which reads ITS OWN planes: nothing paired until it has searched and estimated
    -- and a pipelined renderer return the owner's 480 bytes, which are the restatement's."""
    import gsplat
    from gsplat import _abi
    s, u, W, H, st, small, whole = tr._cfg_a()
    want = _cfg_want()
    owner = _mk(s, W, H, 16)
    owner.write_state(st)
    assert _cfg_records(owner) == want
    assert _cfg_records(owner) == want
    slab = _mk(s, W, H, 16, cols=SLAB_COLS[16])
    slab.write_state(st)
    assert _cfg_records(slab) == want
    slab.destroy()
    borrower = _mk(s, W, H, 16, share_with=owner)
    got, raw = _dev(borrower, mr.THIRD, PIVOTS[0])
    assert got["matched"] == 1001 and raw[16:] == bytes(464)  # the owner has searched and estimated, the borrower has not
    assert _cfg_records(borrower) == want
    borrower.destroy()
    p = gsplat.PipelinedRenderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(s), 16, frames_in_flight=2, flags=_abi.GS_FLAG_SPLAT_STATE)
    p.write_state(st)
    p.render_uniforms(u)
    p.render_uniforms(u)
    assert _cfg_records(p) == want
    p.destroy()
    owner.destroy()


def _same_fit(f, w):
    for k in ("x", "translate", "pivot"):
        np.testing.assert_array_equal(np.asarray(f[k]).view(np.uint64), np.asarray(w[k]).view(np.uint64), err_msg=k)
    assert [mr.bits(v) for v in f["rot"]] == [mr.bits(v) for v in w["rot"]]
    for k in ("rms", "rms_plane", "predicted"):
        assert mr.bits(f[k]) == mr.bits(w[k]), k
    assert f["paired"] == w["paired"]


@pytest.mark.gpu
def test_plane_step_and_align_match_restatement():
    """plane_step on the patch scene equals the host restatement of the same step bit for bit -- the nearest plane, x, the transform's
    numbers, every float of every record afterwards -- and leaves the last frame's taps and the statistics as they were; a step on a
    ctx whose normals were never estimated is refused (0 pairs) and moves nothing; align(metric="plane") for 3 steps equals the
    restated loop, through a PipelinedRenderer too."""
    import gsplat
    from gsplat import _abi, nearest, register, surface, synth
    sc, w, al = patch_scene(), step_want(), align_want()
    r = _mk(sc["rec0"], 64, 64, 16)
    r.write_state(sc["st"])
    r.render_uniforms(synth.orbit_camera(3, 64, 64).uniforms(64, 64))
    r.wait()
    before, stats = tr._taps(r), timeless(r.stats())
    with pytest.raises(ValueError, match="0 pairs"):  # no estimate yet: every normal reads NaN
        register.plane_step(r, PLANE["radius"])
    np.testing.assert_array_equal(r.export_splats().view(np.uint32), sc["rec0"].view(np.uint32))
    info = surface.estimate(r, PLANE["normal_radius"], source=REST, query=REST)
    assert info["queried"] == 972 and info["unresolved"] == 0
    np.testing.assert_array_equal(surface.read(r)[0].view(np.uint32), sc["normal"].view(np.uint32))
    f = register.plane_step(r, PLANE["radius"])
    tr._same_frame(r, before, stats)
    _same_fit(f, w["fit"])
    assert (f["moved"], f["search"]["queried"], f["search"]["sources"], f["radius"], f["max_dist"]) == (972, 972, 972, PLANE["radius"], PLANE["radius"])
    np.testing.assert_array_equal(nearest.read(r)[1], w["near"])
    got = r.export_splats()
    np.testing.assert_array_equal(got.view(np.uint32), w["out"].view(np.uint32))
    assert (got[972:, 0:3] != sc["rec0"][972:, 0:3]).any() and (got[972:, 8:12] != sc["rec0"][972:, 8:12]).any()
    np.testing.assert_array_equal(r.read_state(), sc["st"])
    r.destroy()

    def run(q):
        steps = register.align(q, PLANE["radius"], max_iters=3, metric="plane", normal_radius=PLANE["normal_radius"])
        assert len(steps) == len(al["steps"]) == 3
        for f, g in zip(steps, al["steps"]):
            _same_fit(f, g)
            assert (f["radius"], f["max_dist"]) == (g["radius"], g["max_dist"])
        o = q._state_owner() if hasattr(q, "_state_owner") else q
        np.testing.assert_array_equal(o.export_splats().view(np.uint32), al["out"].view(np.uint32))

    r = _mk(sc["rec0"], 64, 64, 16)
    r.write_state(sc["st"])
    run(r)
    r.destroy()
    p = gsplat.PipelinedRenderer(gsplat.Canvas(64, 64), None, 0, gsplat.PackedGaussians(sc["rec0"]), 16, frames_in_flight=2, flags=_abi.GS_FLAG_SPLAT_STATE)
    p.write_state(sc["st"])
    run(p)
    p.destroy()


@pytest.mark.gpu
def test_plane_refusals_and_point_align_unchanged():
    """GS_ERR_NO_SCENE before an upload, zeros for N == 0; a NaN or negative max_dist2, a null or non-finite pivot, a null record and
    a filter that does not fit are refused with the call's name and the record untouched; a ctx without the state plane takes (0, 0)
    only; wrong array lengths raise.  align(metric="point"), spelled out and by default, returns on test_register's align scene what
    it returned before."""
    from gsplat import _abi, register
    L = _abi.load()
    INV = _abi.GS_ERR_INVALID_ARGUMENT
    out = guarded(480, np.uint8)
    po = ctypes.cast(out.ctypes.data, ctypes.POINTER(_abi.GsPairPlaneMoments))
    P = _pivot3((0, 0, 0))
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(_abi.GsConfig), 64, 64, 16, _abi.GS_FLAG_SPLAT_STATE
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    assert L.gs_pair_plane_moments(ctx, 0, 0, None, None, P, 1.0, po) == _abi.GS_ERR_NO_SCENE
    assert is_fill(out)
    _abi.check(L.gs_upload_splats(ctx, None, 0))
    _abi.check(L.gs_pair_plane_moments(ctx, 0, 0, None, None, P, 1.0, po))
    assert not out.any()
    L.gs_destroy(ctx)
    out.fill(0xA5)
    al = tr.align_scene()
    r = _mk(al["rec0"], 64, 64, 16)
    r.write_state(al["st0"])
    bad = _pivot3((0, float("nan"), 0))
    for call, fragment in ((lambda: L.gs_pair_plane_moments(r._ctx, 0, 0, None, None, P, float("nan"), po), "max_dist2"),
                           (lambda: L.gs_pair_plane_moments(r._ctx, 0, 0, None, None, P, -1.0, po), "max_dist2"),
                           (lambda: L.gs_pair_plane_moments(r._ctx, 0, 0, None, None, None, 1.0, po), "null pivot"),
                           (lambda: L.gs_pair_plane_moments(r._ctx, 0, 0, None, None, bad, 1.0, po), "pivot[1]"),
                           (lambda: L.gs_pair_plane_moments(r._ctx, 0, 0, None, None, P, 1.0, None), "null moments"),
                           (lambda: L.gs_pair_plane_moments(r._ctx, 0x100, 0, None, None, P, 1.0, po), "does not fit the state byte")):
        assert call() == INV, fragment
        msg = L.gs_last_error().decode()
        assert "gs_pair_plane_moments" in msg and fragment in msg, msg
    assert is_fill(out)
    with pytest.raises(ValueError):
        register.pair_plane_moments(r, partner=np.zeros(5, np.uint32))
    with pytest.raises(ValueError):
        register.pair_plane_moments(r, normal=np.zeros((5, 3), F))
    with pytest.raises(ValueError, match="metric"):
        register.align(r, 1.0, metric="plain")
    steps = register.align(r, metric="point", **tr.ALIGN)
    assert [(f["paired"], mr.bits(f["rms"]), f["radius"], f["max_dist"]) for f in steps] == al["steps"]
    np.testing.assert_array_equal(r.export_splats().view(np.uint32), al["out"].view(np.uint32))
    r.destroy()
    r = _mk(al["rec0"], 64, 64, 16)
    r.write_state(al["st0"])
    steps = register.align(r, **tr.ALIGN)
    assert [(f["paired"], mr.bits(f["rms"]), f["radius"], f["max_dist"]) for f in steps] == al["steps"]
    np.testing.assert_array_equal(r.export_splats().view(np.uint32), al["out"].view(np.uint32))
    r.destroy()
    q = mk(al["rec0"], 64, 64, 16)
    pos = np.ascontiguousarray(al["rec0"][:, 0:3])
    part, nrm = pr.partner("perm", pos), pp.normals("unit", pos.shape[0])
    assert pp.same(register.pair_plane_moments(q, (0, 0), INF, PIVOTS[1], part, nrm), pp.restate(pos, part, nrm, None, INF, PIVOTS[1]))
    code, msg = code_of(lambda: register.pair_plane_moments(q, mr.THIRD, INF, PIVOTS[0], part, nrm))
    assert code == INV and "GS_FLAG_SPLAT_STATE" in msg and "gs_pair_plane_moments" in msg
    q.destroy()
