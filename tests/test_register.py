"""Registration (gs_abi.h "registration"): gs_pair_moments and gs_pair_moments_host against the restatement of tests/pairs_restate.py,
bit for bit on hi and lo and on both counts; the fit, the step and the loop of gsplat.register."""
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
import xform_restate as xr
from conftest import scene
from support import F, ROOT, SLAB_COLS, TAPS, c_layout, cached, code_of, guarded, is_fill, mk, state_scene, timeless

_mk = functools.partial(mk, state=True)
CSRC = os.path.join(ROOT, "gaussian-splatting-wgpu_amd", "csrc")
SEL, REST = (2, 2), (2, 0)
SIZED = ("scene", "cancel", "far", "spread")
CELLS = [(k, n) for k in SIZED for n in mr.LENGTHS + (1043,)] + [("nonfinite", 1043)]
INF = float("inf")


def positions(kind, n):
    """(n, 3) float32, seeded, once per session.  Every sized kind holds exact duplicates (d2 = +0.0 occurs)."""
    def make():
        if kind == "scene":
            return pr.with_duplicates(scene(10000)[:n, 0:3])
        if kind == "cancel":
            return mr.cancel(n)  # (a period of ten values: duplicates throughout)
        if kind == "far":
            return pr.far(n)
        return pr.spread(n) if kind == "spread" else mr.nonfinite()
    return cached(("pairs_positions", kind, n), make)


def records(pos):
    """scene() records with the given centres."""
    rec = np.array(scene(10000)[:pos.shape[0]], dtype=F, copy=True)
    rec[:, 0:3] = pos
    return np.ascontiguousarray(rec)


def partner(kind, n, pk):
    return cached(("pairs_partner", kind, n, pk), lambda: pr.partner(pk, positions(kind, n)))


def columns(kind, n, pk):
    """The restatement's per-splat terms of one cell and partner kind, computed once and shared by the CPU and the GPU tests."""
    return cached(("pairs_columns", kind, n, pk), lambda: pr.columns(positions(kind, n), partner(kind, n, pk)))


def distances(kind, n):
    """The d2 bounds of the nearest partner kind: 0 (duplicates), the median of the d2 that occur and the float32 below it."""
    valid, d2, _ = columns(kind, n, "nearest")
    if not valid.any():
        return (F(0),)
    med = np.sort(d2[valid])[valid.sum() // 2]
    return (F(0), med, np.nextafter(med, F(-1))) if med > 0 else (F(0),)  # (a median of 0: nothing below it is a valid bound)


def cases(kind, n):
    """[(partner kind, filter, max_d2)]: every partner kind with every filter at +inf; the nearest one also at the finite bounds."""
    out = [(pk, where, F(np.inf)) for pk in pr.PARTNERS for where in mr.FILTERS]
    return out + [("nearest", where, d) for where in mr.FILTERS[:2] for d in distances(kind, n)]


def want_of(kind, n, pk, where, max_d2):
    return pr.record(columns(kind, n, pk), mr.keep_of(where, mr.third(n)), max_d2)


def _host(pos, part, st, where, max_d2):
    """gs_pair_moments_host with max_dist2 given as it is (the Python wrapper squares a distance)."""
    from gsplat import _abi, register
    planes = [np.ascontiguousarray(pos[:, a]) for a in range(3)]
    out = _abi.GsPairMoments()
    _abi.check(_abi.load().gs_pair_moments_host(planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, pos.shape[0], part.ctypes.data,
                                                None if st is None else st.ctypes.data, where[0], where[1], float(max_d2), ctypes.byref(out)))
    return register._result(out)


def _dev(r, where, max_d2, part=None):
    """gs_pair_moments likewise: (the record as a dict, its 352 bytes)."""
    from gsplat import _abi, register
    o = r._state_owner() if hasattr(r, "_state_owner") else r
    out = _abi.GsPairMoments()
    _abi.check(o._L.gs_pair_moments(o._ctx, where[0], where[1], None if part is None else part.ctypes.data, float(max_d2), ctypes.byref(out)))
    return register._result(out), bytes(out)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_register_abi(tmp_path):
    """Both symbols are exported without a GPU and listed; gs_pair_moments is 352 bytes and every offset agrees between the compiled
    header and ctypes; the version is still 3; a null ctx and the host call's bad arguments are refused with the call's name and the
    record untouched; the renderer classes gained no public method."""
    from gsplat import _abi, register, renderer
    L = _abi.load()
    for name in ("gs_pair_moments", "gs_pair_moments_host"):
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    assert L.gs_abi_version() == 3
    fm = [n for n, _ in _abi.GsPairMoments._fields_]
    prog = 'printf("%zu", sizeof(struct gs_pair_moments));'
    prog += "".join('printf(" %%zu", offsetof(struct gs_pair_moments, %s));' % n for n in fm)
    prog += 'printf(" %u", (unsigned)GS_ABI_VERSION);'
    out = c_layout(tmp_path, "pairs_layout", prog)
    assert out[0] == ctypes.sizeof(_abi.GsPairMoments) == 352
    assert out[1:8] == [getattr(_abi.GsPairMoments, n).offset for n in fm] == [0, 8, 16, 64, 112, 256, 304]
    assert out[8] == 3
    rec = guarded(352, np.uint8)
    po = ctypes.cast(rec.ctypes.data, ctypes.POINTER(_abi.GsPairMoments))
    assert L.gs_pair_moments(None, 0, 0, None, 1.0, po) == _abi.GS_ERR_INVALID_ARGUMENT
    assert b"gs_pair_moments" in L.gs_last_error() and b"null ctx" in L.gs_last_error()
    x, ids, st = np.arange(4, dtype=F), np.arange(4, dtype=np.uint32), np.zeros(4, np.uint8)
    X, I, S = x.ctypes.data, ids.ctypes.data, st.ctypes.data
    for args, fragment in (((None, X, X, 4, I, None, 0, 0, 1.0, po), "null position plane"), ((X, X, None, 4, I, None, 0, 0, 1.0, po), "null position plane"),
                           ((X, X, X, 4, None, None, 0, 0, 1.0, po), "null partner"), ((X, X, X, 4, I, None, 4, 4, 1.0, po), "null state"),
                           ((X, X, X, 4, I, S, 0x100, 0, 1.0, po), "does not fit the state byte"), ((X, X, X, 4, I, S, 0, 0, float("nan"), po), "max_dist2"),
                           ((X, X, X, 4, I, S, 0, 0, -1.0, po), "max_dist2"), ((X, X, X, 1 << 31, I, S, 0, 0, 1.0, po), "2^31"),
                           ((X, X, X, 4, I, S, 0, 0, 1.0, None), "null moments")):
        assert L.gs_pair_moments_host(*args) == _abi.GS_ERR_INVALID_ARGUMENT, fragment
        msg = L.gs_last_error().decode()
        assert "gs_pair_moments_host" in msg and fragment in msg, msg
    assert is_fill(rec)
    # n == 0: zeros; -0.0 is a valid bound
    empty = register.host_pair_moments(np.zeros((0, 3), F), np.zeros(0, np.uint32))
    assert pr.same(empty, pr.restate(np.zeros((0, 3), F), np.zeros(0, np.uint32))) and empty["matched"] == 0
    assert _host(np.zeros((2, 3), F), np.array([1, 0], np.uint32), None, (0, 0), -0.0)["paired"] == 2
    import test_abi
    for cname in ("Renderer", "PipelinedRenderer"):
        live = {n for n in vars(getattr(renderer, cname)) if not n.startswith("_") and callable(getattr(getattr(renderer, cname), n))}
        assert live == set(test_abi.PYTHON_HOST_SURFACE[cname]) - {"__init__"}
    import gsplat
    assert gsplat.register is register
    assert "snapshots" in register.align.__doc__ and "pre-alignment" in register.align.__doc__


def test_restatement_is_pinned():
    """The integer columns of pairs_restate against the term-by-term Fraction sum, and the pairing rule at its edges."""
    for kind, n in (("scene", 1025), ("far", 1023), ("spread", 1043), ("nonfinite", 1043), ("cancel", 5)):
        pos, st = positions(kind, n), mr.third(n)
        for pk in ("nearest", "perm", "beyond"):
            keep = mr.keep_of(mr.THIRD, st)
            assert pr.same(pr.record(columns(kind, n, pk), keep), pr.by_fractions(pos, partner(kind, n, pk), keep)), (kind, pk)
    # ids at and past N are unpaired, a non-finite p or q is, j == i is a pair with d2 = 0
    pos = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [3e38, 0, 0], [-3e38, 0, 0]], F)
    got = pr.restate(pos, np.array([1, 5, 0, 4, 4], np.uint32))
    assert (got["matched"], got["paired"]) == (5, 3)  # 0 -> 1, 3 -> 4 (d2 = +inf <= +inf), 4 -> 4
    assert pr.restate(pos, np.array([1, 5, 0, 4, 4], np.uint32), None, F(3e38))["paired"] == 2  # the overflowed d2 passes +inf only
    assert pr.restate(pos, np.array([2, 0, 1, 0, 0], np.uint32), None, F(1))["paired"] == 1  # a NaN partner; 1 -> 0 at d2 = 1 exactly
    assert pr.restate(pos, np.arange(5, dtype=np.uint32), None, F(0))["paired"] == 4
    z = pr.restate(pos, np.full(5, pr.NONE, np.uint32))
    assert z["paired"] == 0 and all(mr.bits(v) == 0 for e in pr.flat(z) for v in e)  # an exact zero is {+0.0, +0.0}


@pytest.mark.parametrize("kind,n", CELLS)
def test_host_pair_moments(kind, n):
    """gs_pair_moments_host on every scene, length, partner kind and filter; the nearest partners also at max_dist2 = 0 (exact
    duplicates), at a d2 that occurs (inclusive) and just below it; with and without a state plane; through the Python wrapper."""
    from gsplat import register
    pos, st = positions(kind, n), mr.third(n)
    for pk, where, d in cases(kind, n):
        got = _host(pos, partner(kind, n, pk), st, where, d)
        assert pr.same(got, want_of(kind, n, pk, where, d)), (kind, n, pk, where, d)
    for pk in ("nearest", "beyond"):
        assert pr.same(_host(pos, partner(kind, n, pk), None, (0, 0), INF), want_of(kind, n, pk, (0, 0), INF))  # no plane at all
        assert pr.same(register.host_pair_moments(pos, partner(kind, n, pk), st, mr.THIRD), want_of(kind, n, pk, mr.THIRD, INF))
    assert want_of(kind, n, "none", (0, 0), INF)["paired"] == 0 == want_of(kind, n, "nearest", mr.NOTHING, INF)["matched"]
    ds = distances(kind, n)
    if n >= 1023 and kind in SIZED:
        assert want_of(kind, n, "nearest", (0, 0), ds[0])["paired"] > 0  # the duplicates, at d2 <= 0
    if len(ds) == 3:
        assert want_of(kind, n, "nearest", (0, 0), ds[1])["paired"] > want_of(kind, n, "nearest", (0, 0), ds[2])["paired"]  # inclusive AT the median
    if kind == "nonfinite":
        full = want_of(kind, n, "self", (0, 0), INF)
        assert full["matched"] - full["paired"] == len(mr.EDGES) and abs(full["sum_p"][0][0]) < 1e5  # the 1e30 beside a NaN is in no sum
    if kind == "spread" and n >= 1023:
        hi = [abs(e[0]) for e in pr.flat(want_of(kind, n, "perm", (0, 0), INF))[6:15]]
        assert max(hi) > 2.0 ** 100 and want_of(kind, n, "perm", (0, 0), INF)["paired"] == n  # products far apart, every d2 finite


def _cloud(kind, n=1500, seed=5):
    rng = np.random.default_rng(seed)
    if kind == "far":
        return (1.0e4 + rng.random((n, 3))).astype(F)
    if kind == "flat":
        return (rng.normal(size=(n, 3)) * np.array([3.0, 2.0, 1.0e-3])).astype(F)
    return (rng.normal(size=(n, 3)) * np.array([3.0, 2.0, 1.0])).astype(F)


R0 = xr.rot_matrix(xr.axis_angle((0.2, 0.9, -0.4), 0.7))
T0 = np.array([0.4, -1.1, 2.2])


def _moved(p, s0=1.0, mirror=False):
    """q = s0 R0 (p - c) + c + T0 in float64, rounded to f32 (mirror: with p's z reflected through c first)."""
    p64 = p.astype(np.float64)
    c = p64.mean(axis=0)
    d = p64 - c
    if mirror:
        d = d * np.array([1.0, 1.0, -1.0])
    return (s0 * d @ R0.T + c + T0).astype(F)


def _paired_scene(p, q):
    """(positions, partner, state): the p's selected, each with its q as partner, the q's behind them."""
    n = p.shape[0]
    return (np.concatenate([p, q]), np.concatenate([np.arange(n, 2 * n), np.full(n, pr.NONE)]).astype(np.uint32),
            np.concatenate([np.full(n, 2), np.zeros(n)]).astype(np.uint8))


def _kabsch64(p, q, scale):
    """An independent float64 Kabsch / Umeyama on the same f32 pairs: centre, SVD."""
    p, q = p.astype(np.float64), q.astype(np.float64)
    pm, qm = p.mean(axis=0), q.mean(axis=0)
    P, Q = p - pm, q - qm
    U, D, Vt = np.linalg.svd(P.T @ Q)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    s = (D[0] + D[1] + d * D[2]) / (P * P).sum() if scale else 1.0
    return R, s, pm, qm - pm, D


def _held(e):
    return Fraction(e[0]) + Fraction(e[1])


def test_fit_against_float64():
    """fit against the independent float64 solution on the same f32 pairs: R to 1e-9 absolute, scale, pivot and translate to 1e-9
    relative -- both are double-precision solutions of one well-conditioned problem (singular values of M within a factor 100, printed)
    and differ by about 1e-15 x condition.  rms equals its Fraction restatement bit for bit.  A reflection-prone flat cloud returns
    det R = +1; fewer than 3 pairs and a collinear cloud raise."""
    from gsplat import register
    for kind in ("near", "far"):
        for scale, s0 in ((False, 1.0), (True, 1.3)):
            p = _cloud(kind)
            q = _moved(p, s0)
            pos, part, st = _paired_scene(p, q)
            m = register.host_pair_moments(pos, part, st, SEL)
            assert pr.same(m, pr.restate(pos, part, st == 2))
            f = register.fit(m, scale)
            R, s, pivot, translate, D = _kabsch64(p, q, scale)
            print(kind, scale, "singular values", f["singular"], "max |R - R64| %.3e" % np.abs(f["R"] - R).max())
            assert f["singular"][0] <= 100 * f["singular"][2] and np.allclose(f["singular"], D, rtol=1e-9)
            assert np.abs(f["R"] - R).max() <= 1e-9 and abs(np.linalg.det(f["R"]) - 1) < 1e-12
            assert abs(f["scale"] - s) <= 1e-9 * s and (scale or f["scale"] == 1.0)
            assert np.all(np.abs(f["pivot"] - pivot) <= 1e-9 * np.abs(pivot))
            assert np.all(np.abs(f["translate"] - translate) <= 1e-9 * np.abs(translate))
            assert np.abs(f["R"] - R0).max() < 1e-3 and f["paired"] == p.shape[0]
            assert np.allclose(np.array(f["rot"]) @ np.array(f["rot"]), 1.0) and np.abs(xr.rot_matrix(f["rot"]) - f["R"]).max() < 1e-12
            # rms: sqrt(RN(sum_a pp + qq - 2 pq_aa) / n) from the restated sums as the record holds them
            w = pr.restate(pos, part, st == 2)
            ssd = float(sum((_held(w["pp"][a]) + _held(w["qq"][a]) - 2 * _held(w["pq"][a][a]) for a in range(3)), Fraction(0)))
            assert mr.bits(f["rms"]) == mr.bits(math.sqrt(ssd / w["paired"]))
            direct = math.sqrt(((p.astype(np.float64) - q.astype(np.float64)) ** 2).sum() / p.shape[0])
            assert abs(f["rms"] - direct) <= 1e-12 * direct
    # a flat cloud whose partners are mirrored through its plane: the best orthogonal map is a reflection, the fit must not return it
    p = _cloud("flat")
    pos, part, st = _paired_scene(p, _moved(p, mirror=True))
    f = register.fit(register.host_pair_moments(pos, part, st, SEL))
    R, _, _, _, _ = _kabsch64(p, pos[p.shape[0]:], False)
    assert abs(np.linalg.det(f["R"]) - 1) < 1e-12 and np.abs(f["R"].T @ f["R"] - np.eye(3)).max() < 1e-12
    assert np.abs(f["R"] - R).max() <= 1e-9
    # too few pairs; pairs on a line
    two = register.host_pair_moments(pos[:4], np.array([2, 3, pr.NONE, pr.NONE], np.uint32))
    assert two["paired"] == 2
    with pytest.raises(ValueError, match="2 pairs"):
        register.fit(two)
    line = (np.arange(40, dtype=np.float64)[:, None] * np.array([1.0, 2.0, 3.0])).astype(F)
    with pytest.raises(ValueError, match="line"):
        register.fit(register.host_pair_moments(*_paired_scene(line, _moved(line))[:2]))


def ulp_of(x):
    return float(np.spacing(F(x)))


def test_xform_of_moves_p_onto_q():
    """xform_of(fit) applied by xform_restate to p, where q = s R0 p + t0 was generated in float64 and rounded to f32: the moved points
    lie within 4 ulp of the largest coordinate magnitude of q, per component.

    The bound.  q is one rounding from the true image: 1/2 ulp.  A row of the transform, ((m0 X + m1 Y) + m2 Z) + m3, is four operations
    deep -- a product, then three adds -- and each rounds by at most 1/2 ulp of a value no larger than the largest coordinate: 2 ulp.
    The fitted map itself, a least-squares mean over 1500 pairs held in double, is off by far less than one ulp.  Together 2.5 ulp of
    the largest coordinate magnitude of q; the bound of 4 leaves 1.5 for the two products beside the chain and for the f32 rounding of
    the twelve matrix entries.  (Measured: 1 to 2 ulp, printed below.)"""
    from gsplat import register
    for kind in ("near", "far"):
        for scale, s0 in ((False, 1.0), (True, 1.3)):
            p = _cloud(kind)
            q = _moved(p, s0)
            pos, part, st = _paired_scene(p, q)
            f = register.fit(register.host_pair_moments(pos, part, st, SEL), scale)
            rec = records(pos)
            out = xr.apply(rec, xr.Xform.from_struct(register.xform_of(f)), st == 2)
            err = np.abs(out[:p.shape[0], 0:3].astype(np.float64) - q.astype(np.float64)).max(axis=0)
            bound = 4 * ulp_of(np.abs(q).max())
            print(kind, scale, "error in ulp of the largest coordinate", err / ulp_of(np.abs(q).max()))
            assert np.all(err <= bound), (kind, scale, err, bound)
            np.testing.assert_array_equal(out[p.shape[0]:].view(np.uint32), rec[p.shape[0]:].view(np.uint32))


def test_sanitized_host_program(tmp_path):
    """tools/pairs_check: gs_pair_host.h compiled alone with -fsanitize=address,undefined and run as its own process; it runs the
    pairing loop over its partner planes (all NONE, ids >= N, every id equal, j == i) in two orders of summation and compares the
    limbs, and prints the record of a file's scene, which must be the restatement's.  Skipped where the sanitizer runtime is not
    installed."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed")
    exe = str(tmp_path / "pairs_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san +
                          ["-I", CSRC, os.path.join(ROOT, "tools", "pairs_check", "main.cpp"), "-o", exe])
    for kind, n, pk in (("nonfinite", 1043, "beyond"), ("spread", 1025, "perm"), ("far", 1023, "nearest")):
        pos, part = positions(kind, n), partner(kind, n, pk)
        path = tmp_path / (kind + ".txt")
        rows = np.column_stack([pos.view(np.uint32), part])
        path.write_text("%d\n" % n + "\n".join(" ".join("%08x" % int(w) for w in row) for row in rows) + "\n")
        out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")
        assert lines[0] == "pairs_check ok"
        want = want_of(kind, n, pk, (0, 0), INF)
        assert lines[1] == "matched %d paired %d" % (want["matched"], want["paired"])
        got = [tuple(int(x, 16) for x in ln.split()) for ln in lines[2:23]]
        assert got == [(mr.bits(hi), mr.bits(lo)) for hi, lo in pr.flat(want)], kind


# ---- the scenes of the step and of the loop: built on the CPU, checked on the CPU ----------------------------------------------------
def _duplicated(base, sel, X):
    """What duplicate_selected(xform) leaves: the records with the copies of `sel` behind them, transformed; the state plane."""
    copies = xr.apply(base[sel], xr.Xform.from_struct(X))
    return np.concatenate([base, copies]), np.concatenate([np.zeros(base.shape[0], np.uint8), np.full(int(sel.sum()), 2, np.uint8)])


def step_scene():
    """2000 splats on a jittered lattice of spacing 1 and a copy of the 700 nearest its centre, turned by 3 degrees about their
    centroid and shifted by a tenth of the spacing: every copy stays nearer to its original than to any other splat."""
    def make():
        from gsplat import _abi
        rng = np.random.default_rng(31)
        g = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), -1).reshape(-1, 3)[:2000].astype(np.float64)
        pos = (g + rng.uniform(-0.05, 0.05, g.shape)).astype(F)
        base = records(pos)
        order = np.argsort(((pos - pos.astype(np.float64).mean(axis=0)) ** 2).sum(axis=1))
        sel = np.zeros(2000, bool)
        sel[order[:700]] = True
        X = _abi.compose_xform(rot=xr.axis_angle((0.3, -0.5, 0.81), np.radians(3.0)), translate=(0.06, -0.05, 0.04),
                               pivot=pos[sel].astype(np.float64).mean(axis=0))
        rec0, st0 = _duplicated(base, sel, X)
        out, f, near = pr.step(rec0, st0, 1.0)
        return dict(base=base, sel=sel, X=X, rec0=rec0, st0=st0, out=out, fit=f, near=near, radius=1.0)
    return cached("register_step_scene", make)


ALIGN = dict(radius=1.0, max_iters=10, tol=1e-3)


def align_scene():
    """40 clusters of 50 splats (sigma 0.05, about 0.03 between neighbours) two units apart, and a copy of 17 splats of each, turned by
    3 degrees and shifted by 0.3 -- ten spacings, so the first pairs are mostly wrong ones within the right cluster."""
    def make():
        from gsplat import _abi
        rng = np.random.default_rng(41)
        g = np.stack(np.meshgrid(np.arange(4), np.arange(5), np.arange(2), indexing="ij"), -1).reshape(-1, 3) * 2.0
        centres = g + rng.uniform(-0.4, 0.4, g.shape)
        pos = (np.repeat(centres, 50, axis=0) + rng.normal(0, 0.05, (2000, 3))).astype(F)
        base = records(pos)
        sel = np.arange(2000) % 50 < 17
        X = _abi.compose_xform(rot=xr.axis_angle((0.3, -0.5, 0.81), np.radians(3.0)), translate=(0.18, -0.192, 0.144),
                               pivot=pos[sel].astype(np.float64).mean(axis=0))
        rec0, st0 = _duplicated(base, sel, X)
        out, steps = pr.align(rec0, st0, **ALIGN)
        return dict(base=base, sel=sel, X=X, rec0=rec0, st0=st0, out=out, steps=steps)
    return cached("register_align_scene", make)


def test_restated_step_and_loop():
    """What the GPU tests rely on, asserted on the restatement alone: the step's move pairs every copy with its original and one step
    brings every copy within the 4-ulp bound of test_xform_of_moves_p_onto_q; the loop needs several steps and ends below 1 % of its
    first rms."""
    sc = step_scene()
    orig = np.flatnonzero(sc["sel"])
    np.testing.assert_array_equal(sc["near"][2000:], orig)
    assert sc["fit"]["paired"] == 700 and (sc["near"][:2000] == pr.NONE).all()
    big = np.abs(sc["base"][orig, 0:3]).max()
    err = np.abs(sc["out"][2000:, 0:3].astype(np.float64) - sc["base"][orig, 0:3].astype(np.float64)).max()
    print("step: largest distance to the original %.3e = %.2f ulp of %g" % (err, err / ulp_of(big), big))
    assert err <= 4 * ulp_of(big)
    al = align_scene()
    rms = [float(np.uint64(b).view(np.float64)) for _, b, _, _ in al["steps"]]
    print("align: rms per step", rms)
    assert len(rms) > 3 and rms[-1] < 0.01 * rms[0]
    assert al["steps"][1][3] == min(ALIGN["radius"], 3.0 * rms[0]) and al["steps"][0][3] == ALIGN["radius"]


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", CELLS)
def test_pair_moments_host_partners(kind, n):
    """gs_pair_moments with a HOST partner array on every scene, length, partner kind, filter and bound of test_host_pair_moments;
    3001 splats also with GS_OPT_PERSISTENT_GRID 1 (several trips per thread), where the 352 bytes do not change."""
    from gsplat import _abi, register
    pos = positions(kind, n)
    r = _mk(records(pos), 64, 64, 16)
    r.write_state(mr.third(n))
    seen = {}
    for grid in ((0, 1) if n == 3001 else (0,)):
        if grid:
            r.set_option(_abi.GS_OPT_PERSISTENT_GRID, grid)
        for pk, where, d in cases(kind, n):
            got, raw = _dev(r, where, d, partner(kind, n, pk))
            assert pr.same(got, want_of(kind, n, pk, where, d)), (kind, n, pk, where, d, grid)
            assert seen.setdefault((pk, where, float(d)), raw) == raw
    assert pr.same(register.pair_moments(r, mr.THIRD, INF, partner(kind, n, "perm")), want_of(kind, n, "perm", mr.THIRD, INF))
    r.destroy()


def _cfg_a():
    def make():
        s, u, W, H = state_scene("cfgA")
        s = np.ascontiguousarray(s[:3001])
        st = mr.third(3001)
        d2 = knn_restate.planes(s, 1, np.inf)[0]
        spacing = float(np.median(np.sqrt(d2.astype(np.float64))))
        lo, hi = s[:, 0:3].min(axis=0), s[:, 0:3].max(axis=0)
        return s, u, W, H, st, 0.5 * spacing, 2.0 * float(np.linalg.norm(hi.astype(np.float64) - lo))
    return cached("register_cfgA", make)


def _plane_want(radius, src, qry, where, max_d2=INF):
    """The restated record over `where` of the nearest plane a search (source src, query qry) at `radius` leaves."""
    def make():
        s, _, _, _, st, _, _ = _cfg_a()
        near = knn_restate.planes(s, 1, radius, src=mr.keep_of(src, st), qry=mr.keep_of(qry, st))[1]
        return pr.restate(s[:, 0:3], near, mr.keep_of(where, st), max_d2), near
    return cached(("register_plane_want", radius, src, qry, where, float(max_d2)), make)


def _own_plane_records(r):
    """The 352 bytes of a few calls on the ctx's own plane after two searches (one cell for the whole scene; most queries NONE), and
    of one with a host array."""
    from gsplat import nearest
    s, _, _, _, st, small, whole = _cfg_a()
    out = []
    for radius in (whole, small):
        nearest.search(r, 1, radius, source=(0, 0), query=mr.THIRD)
        for where in ((0, 0), mr.THIRD):
            out.append(_dev(r, where, INF)[1])
    out.append(_dev(r, mr.THIRD, INF, pr.partner("perm", s[:, 0:3]))[1])
    return out


def _own_plane_want():
    s, _, _, _, st, small, whole = _cfg_a()
    out = [pr.as_bytes(_plane_want(radius, (0, 0), mr.THIRD, where)[0]) for radius in (whole, small) for where in ((0, 0), mr.THIRD)]
    return out + [pr.as_bytes(pr.restate(s[:, 0:3], pr.partner("perm", s[:, 0:3]), mr.keep_of(mr.THIRD, st)))]


@pytest.mark.gpu
def test_pair_moments_own_plane():
    """partner == NULL: all zeros before any search; the restatement of the searched plane at a radius that makes the scene one cell
    and at one that leaves most queries NONE; equal bytes twice in a row; all zeros again after a compaction dropped the plane."""
    from gsplat import nearest
    s, u, W, H, st, small, whole = _cfg_a()
    r = _mk(s, W, H, 16)
    r.write_state(st)
    zero = pr.restate(s[:, 0:3], np.full(3001, pr.NONE, np.uint32), mr.keep_of(mr.THIRD, st))
    got, raw = _dev(r, mr.THIRD, INF)
    assert pr.same(got, zero) and got["matched"] == 1001 and raw[16:] == bytes(336)  # never searched
    want = _own_plane_want()
    assert _own_plane_records(r) == want
    assert _own_plane_records(r) == want
    few, near = _plane_want(small, (0, 0), mr.THIRD, mr.THIRD)
    assert 0 < few["paired"] < 0.5 * few["matched"] and _plane_want(whole, (0, 0), mr.THIRD, mr.THIRD)[0]["paired"] == 1001
    d2, got_near = nearest.read(r)
    np.testing.assert_array_equal(got_near, near)
    # a bound on the plane's own pairs, inclusive at a d2 that occurs
    med = np.sort(d2[np.isfinite(d2)])[np.isfinite(d2).sum() // 2]
    for d in (med, np.nextafter(med, F(-1))):
        assert pr.same(_dev(r, mr.THIRD, d)[0], _plane_want(small, (0, 0), mr.THIRD, mr.THIRD, d)[0])
    kept = r.compact(*mr.THIRD)
    got, raw = _dev(r, (0, 0), INF)
    assert got["matched"] == kept.size == 1001 and got["paired"] == 0 and raw[16:] == bytes(336)
    r.destroy()


@pytest.mark.gpu
def test_slab_borrower_and_pipeline_answer_the_same():
    """A slab context, a borrower of gs_share_splats -- which reads ITS OWN nearest plane: zeros until it has searched -- and a
    pipelined renderer give the owner's bytes."""
    import gsplat
    from gsplat import _abi
    s, u, W, H, st, small, whole = _cfg_a()
    want = _own_plane_want()
    owner = _mk(s, W, H, 16)
    owner.write_state(st)
    assert _own_plane_records(owner) == want
    slab = _mk(s, W, H, 16, cols=SLAB_COLS[16])
    slab.write_state(st)
    assert _own_plane_records(slab) == want
    slab.destroy()
    borrower = _mk(s, W, H, 16, share_with=owner)
    got, raw = _dev(borrower, mr.THIRD, INF)
    assert got["matched"] == 1001 and raw[16:] == bytes(336)  # the owner has searched, the borrower has not
    assert _own_plane_records(borrower) == want
    borrower.destroy()
    p = gsplat.PipelinedRenderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(s), 16, frames_in_flight=2, flags=_abi.GS_FLAG_SPLAT_STATE)
    p.write_state(st)
    p.render_uniforms(u)
    p.render_uniforms(u)
    assert _own_plane_records(p) == want
    p.destroy()
    owner.destroy()


def _taps(r):
    """The last frame's taps and image, read without rendering."""
    from gsplat import _abi
    out = {t: r.read_buffer(getattr(_abi, "GS_BUF_" + t)) for t in TAPS}
    out["rgba8"] = r.read_rgba8()
    out["rgbf"] = r.read_buffer(_abi.GS_BUF_RGB_F32)
    return out


def _same_frame(r, before, stats):
    after = _taps(r)
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    assert timeless(r.stats()) == stats


@pytest.mark.gpu
def test_step_matches_restatement():
    """duplicate_selected builds the step scene; one step equals the host restatement of the same step bit for bit -- the nearest
    plane, the record, positions, quaternions and log-scales of the moved splats, every other float -- and brings every copy within the
    4-ulp bound of its original.  The last frame's taps and the statistics are unchanged by the calls."""
    from gsplat import insert, nearest, register, synth
    sc = step_scene()
    r = _mk(sc["base"], 64, 64, 16)
    r.write_state(sc["sel"].astype(np.uint8) * 2)
    assert insert.duplicate_selected(r, sc["X"]) == (2000, 700)
    np.testing.assert_array_equal(r.export_splats().view(np.uint32), sc["rec0"].view(np.uint32))
    np.testing.assert_array_equal(r.read_state(), sc["st0"])
    r.render_uniforms(synth.orbit_camera(3, 64, 64).uniforms(64, 64))
    r.wait()
    before, stats = _taps(r), timeless(r.stats())
    f = register.step(r, sc["radius"])
    _same_frame(r, before, stats)
    w = sc["fit"]
    assert (f["paired"], f["moved"], f["search"]["queried"], f["search"]["sources"]) == (700, 700, 700, 2000)
    assert mr.bits(f["rms"]) == mr.bits(w["rms"]) and (f["radius"], f["max_dist"]) == (1.0, 1.0)
    for k in ("R", "pivot", "translate", "M"):
        np.testing.assert_array_equal(f[k], w[k], err_msg=k)
    np.testing.assert_array_equal(nearest.read(r)[1], sc["near"])
    got = r.export_splats()
    np.testing.assert_array_equal(got.view(np.uint32), sc["out"].view(np.uint32))
    assert (got[2000:, 0:3] != sc["rec0"][2000:, 0:3]).any() and (got[2000:, 8:12] != sc["rec0"][2000:, 8:12]).any()
    orig = np.flatnonzero(sc["sel"])
    big = np.abs(sc["base"][orig, 0:3]).max()
    assert np.abs(got[2000:, 0:3].astype(np.float64) - sc["base"][orig, 0:3].astype(np.float64)).max() <= 4 * ulp_of(big)
    np.testing.assert_array_equal(r.read_state(), sc["st0"])
    r.destroy()


@pytest.mark.gpu
def test_align_matches_restatement():
    """align on a copy displaced by ten spacings: the list of step records (paired, the rms's bits, radius, max_dist) and the final
    records equal the restated loop's exactly; through a PipelinedRenderer the same."""
    import gsplat
    from gsplat import _abi, register
    al = align_scene()

    def run(r):
        steps = register.align(r, **ALIGN)
        assert [(f["paired"], mr.bits(f["rms"]), f["radius"], f["max_dist"]) for f in steps] == al["steps"]
        o = r._state_owner() if hasattr(r, "_state_owner") else r
        np.testing.assert_array_equal(o.export_splats().view(np.uint32), al["out"].view(np.uint32))

    r = _mk(al["rec0"], 64, 64, 16)
    r.write_state(al["st0"])
    run(r)
    r.destroy()
    p = gsplat.PipelinedRenderer(gsplat.Canvas(64, 64), None, 0, gsplat.PackedGaussians(al["rec0"]), 16, frames_in_flight=2, flags=_abi.GS_FLAG_SPLAT_STATE)
    p.write_state(al["st0"])
    run(p)
    p.destroy()


@pytest.mark.gpu
def test_align_default_radius():
    """radius=None: eight times the median nearest-neighbour distance among the fixed splats, restated from the brute-force plane."""
    from gsplat import register
    al = align_scene()
    fixed = al["st0"] == 0
    d2 = knn_restate.planes(al["rec0"], 1, np.inf, src=fixed, qry=fixed)[0]
    radius = 8.0 * float(np.median(np.sqrt(d2[np.isfinite(d2)].astype(np.float64))))
    r = _mk(al["rec0"], 64, 64, 16)
    r.write_state(al["st0"])
    steps = register.align(r, max_iters=2)
    assert len(steps) == 2 and steps[0]["radius"] == steps[1]["radius"] == radius and steps[0]["max_dist"] == radius
    assert steps[1]["max_dist"] == min(radius, 3.0 * steps[0]["rms"])
    _, want = pr.align(al["rec0"], al["st0"], radius, max_iters=2)
    assert [(f["paired"], mr.bits(f["rms"])) for f in steps] == [(a, b) for a, b, _, _ in want]
    r.destroy()


@pytest.mark.gpu
def test_refusals_and_a_refused_fit():
    """GS_ERR_NO_SCENE before an upload, zeros for N == 0; a NaN or negative max_dist2, a null record and a filter that does not fit
    are refused with the call's name and the record untouched; a ctx without the state plane takes (0, 0) only; a step whose fit is
    refused (2 pairs) leaves every plane of the scene byte-equal, and the frame as it was."""
    from gsplat import _abi, nearest, register, synth
    L = _abi.load()
    s, u, W, H, st, small, whole = _cfg_a()
    INV = _abi.GS_ERR_INVALID_ARGUMENT
    out = guarded(352, np.uint8)
    po = ctypes.cast(out.ctypes.data, ctypes.POINTER(_abi.GsPairMoments))
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(_abi.GsConfig), W, H, 16, _abi.GS_FLAG_SPLAT_STATE
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    assert L.gs_pair_moments(ctx, 0, 0, None, 1.0, po) == _abi.GS_ERR_NO_SCENE
    assert is_fill(out)
    _abi.check(L.gs_upload_splats(ctx, None, 0))
    _abi.check(L.gs_pair_moments(ctx, 0, 0, None, 1.0, po))
    assert not out.any()
    L.gs_destroy(ctx)
    out.fill(0xA5)
    r = _mk(s, W, H, 16)
    r.write_state(st)
    for call, fragment in ((lambda: L.gs_pair_moments(r._ctx, 0, 0, None, float("nan"), po), "max_dist2"),
                           (lambda: L.gs_pair_moments(r._ctx, 0, 0, None, -1.0, po), "max_dist2"),
                           (lambda: L.gs_pair_moments(r._ctx, 0, 0, None, 1.0, None), "null moments"),
                           (lambda: L.gs_pair_moments(r._ctx, 0x100, 0, None, 1.0, po), "does not fit the state byte")):
        assert call() == INV, fragment
        msg = L.gs_last_error().decode()
        assert "gs_pair_moments" in msg and fragment in msg, msg
    assert is_fill(out)
    with pytest.raises(ValueError):
        register.pair_moments(r, partner=np.zeros(5, np.uint32))
    # two selected splats: the fit is refused before anything moves
    state = np.zeros(3001, np.uint8)
    state[[10, 2000]] = 2
    r.write_state(state)
    r.render_uniforms(u)
    r.wait()
    before, stats, rec = _taps(r), timeless(r.stats()), r.export_splats()
    with pytest.raises(ValueError, match="2 pairs"):
        register.step(r, whole)
    assert register.align(r, whole) == []
    assert register.pair_moments(r)["paired"] == 2
    np.testing.assert_array_equal(r.export_splats().view(np.uint32), rec.view(np.uint32))
    np.testing.assert_array_equal(r.read_state(), state)
    _same_frame(r, before, stats)
    r.destroy()
    q = mk(s, W, H, 16)
    part = pr.partner("perm", s[:, 0:3])
    assert pr.same(register.pair_moments(q, (0, 0), INF, part), pr.restate(s[:, 0:3], part))
    code, msg = code_of(lambda: register.pair_moments(q, mr.THIRD, INF, part))
    assert code == INV and "GS_FLAG_SPLAT_STATE" in msg and "gs_pair_moments" in msg
    q.destroy()
