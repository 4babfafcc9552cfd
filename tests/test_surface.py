"""Surface: per-splat normals and shape from neighbourhood covariance (include/gsplat/gs_abi.h "surface").

Two references.  tests/surface_restate.py brute-forces all pairs in numpy f32 and adds integers: count, sums and info are held to it
BIT FOR BIT, by the host twin (CPU tests, through surface.host_estimate) and by the device (GPU tests).  Its float64 model
(numpy.linalg.eigh on the exact covariance) holds the finishing within two DERIVED bounds:
    eigenvalues   |l_k - m_k| <= 2^-23 |m_k| + 1e-12 m_0        one f32 rounding (relative 2^-24, doubled for the f32 denormal-free
                                                                range it is used in) plus a thousand times the float64 solvers' error
                                                                of a few 1e-16 m_0
    normal        |n . n_model| >= 1 - 1e-6 where (m_1 - m_2) / m_0 >= 1e-2
                                                                rounding a unit vector to f32 costs at most 1.1e-7 of the dot product,
                                                                the eigenvector's own error is 1e-14 at that gap, a wrong column gives ~0
The device's normal and eig are compared with the host twin's bit for bit: both run the same header in IEEE float64 without
contraction.  Hand pins (a lattice, one of its layers, pairs, triples, lines) fix what the model cannot: exact ties.
"""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import state_restate as sr
import surface_restate as su
from support import F, ROOT, SLAB_COLS, c_layout, cached, code_of, frame_taps, host_sources, mk, state_scene, timeless
from test_nearest import lattice_pos, records, special_pos

_mk = functools.partial(mk, state=True)
CSRC = os.path.join(ROOT, "gaussian-splatting-wgpu_amd", "csrc")
OPS = (sr.SET, sr.CLEAR, sr.TOGGLE, sr.ASSIGN)
INF = float("inf")
BICYCLE_RADIUS = 1.0137261


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bicycle1000():
    from gsplat import synth
    return np.array(synth.bicycle_like(3001)[:1000, 0:3], dtype=F, copy=True)


def sheet_pos():
    """The tilted sheet: 1500 points on a 2 x 2 square with 0.002 of noise across it, rotated and moved; radius 0.25."""
    rng = np.random.default_rng(5)
    sheet = np.c_[rng.uniform(0, 2, 1500), rng.uniform(0, 2, 1500), 0.002 * rng.standard_normal(1500)]
    R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    return (sheet @ R.T + [3, -1, 2]).astype(np.float32)


def knot_pos():
    """The lattice, a knot of 200 splats within 0.01 (whole waves whose queries share a cell, next to waves that straddle cells) and
    two far ends that push the grid past 2^24 cells at the lattice's radii (test_nearest.test_blocked_table's construction)."""
    ends = np.array([[-120, -121, -122], [123, 122, 121]], F)
    knot = (F(5.0) + np.random.default_rng(11).uniform(-0.005, 0.005, (200, 3))).astype(F)
    return np.concatenate([lattice_pos(), knot, ends])


def masks(st, source, query):
    return (st & source[0]) == source[1], (st & query[0]) == query[1]


def want(key, pos, radius, st=None, source=(0, 0), query=(0, 0)):
    """The restatement's (count, sums, info), once per key and session; the key names the positions and the state plane."""
    def make():
        sm, qm = (None, None) if st is None else masks(st, source, query)
        return su.sums(pos, radius, sm, qm)
    return cached(("surface", key, float(radius), tuple(source), tuple(query)), make)


def host(key, pos, radius, st=None, source=(0, 0), query=(0, 0), toward=None):
    from gsplat import surface
    return cached(("surface_host", key, float(radius), tuple(source), tuple(query), None if toward is None else tuple(toward)),
                  lambda: surface.host_estimate(pos, radius, state=st, source=source, query=query, toward=toward))


def nan6(normal, eig, where):
    return bool((bits(normal)[where] == su.NAN_BITS).all() and (bits(eig)[where] == su.NAN_BITS).all())


LINES = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1), "xy": (1, 1, 0), "xyz": (1, 2, 3)}


def line_pos(direction):
    """Four collinear points 0.125 apart along an integer direction from (1, 2, 3): every coordinate and difference exact in f32."""
    return (np.array([1, 2, 3], F)[None, :] + np.arange(4, dtype=F)[:, None] * F(0.125) * np.array(direction, F)[None, :]).astype(F)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def check_lattice(estimate):
    """The hand pins; estimate(pos, radius, toward) -> (normal, eig, count, sums)."""
    p = lattice_pos()
    assert su.scale(0.25)[:2] == (-1, F(2.0 ** 17))
    normal, eig, count, sums = estimate(p, 0.25, None)
    inner = [36 * a + 6 * b + c for a in range(1, 5) for b in range(1, 5) for c in range(1, 5)]
    assert (count[inner] == 6).all() and (sums[inner, 0] == 6).all() and (sums[inner, 1:4] == 0).all()
    assert (sums[inner][:, [4, 7, 9]] == 2 ** 31).all() and (sums[inner][:, [5, 6, 8]] == 0).all()  # two face neighbours of q = +-2^15 per axis
    assert (bits(eig)[inner] == bits(np.array([1 / 48], F))[0]).all()  # 2 (2^15)^2 / 6 * 2^-34 = 1/48, three times, exactly
    corner = 0
    assert count[corner] == 3 and not nan6(normal, eig, [corner]) and count.min() == 3
    layer = p[p[:, 2] == F(3.75)]  # z index 3
    assert layer.shape == (36, 3)
    normal, eig, count, sums = estimate(layer, 0.36, None)
    inner = [6 * a + b for a in range(1, 5) for b in range(1, 5)]
    assert (count[inner] == 8).all() and (sums[:, 9] == 0).all() and (sums[:, [6, 8]] == 0).all()
    assert (bits(eig)[:, 2] == 0).all() and (eig[inner, 0] == eig[inner, 1]).all()
    assert (bits(normal) == bits(np.tile(np.array([0, 0, 1], F), (36, 1)))).all()  # (0, 0, 1) bit for bit
    down, _, _, _ = estimate(layer, 0.36, (3.5, 3.5, 0.0))
    assert (down == np.array([0, 0, -1], F)).all()  # negated: below the layer
    up, _, _, _ = estimate(layer, 0.36, (3.5, 3.5, 9.0))
    assert (bits(up) == bits(normal)).all()
    level, _, _, _ = estimate(layer, 0.36, (3.5, 3.5, 3.75))  # t == 0 keeps the normal
    assert (bits(level) == bits(normal)).all()
    # a pair and a triple: count < 3 reads NaN with these bits and keeps its count
    tri = np.array([[1, 1, 1], [1.125, 1, 1], [1, 1.25, 1]], F)
    for pts, cnt in ((tri[:2], [1, 1]), (tri, [2, 2, 2])):
        normal, eig, count, sums = estimate(pts, 0.5, None)
        assert count.tolist() == cnt == sums[:, 0].tolist() and nan6(normal, eig, slice(None))
    normal, eig, count, sums = estimate(tri[:2], 0.5, None)
    assert sums[0].tolist() == [1, 2 ** 13, 0, 0, 2 ** 26, 0, 0, 0, 0, 0] and sums[1].tolist() == [1, -2 ** 13, 0, 0, 2 ** 26, 0, 0, 0, 0, 0]  # E = 0, s = 2^16
    # collinear triples: l1 = l2 = 0; the normal is whatever the rule gives (a unit vector across the line), the same everywhere
    out = {}
    for name, direction in LINES.items():
        normal, eig, count, sums = estimate(line_pos(direction), 0.5 * float(np.linalg.norm(direction)), None)
        assert count.tolist() == [3, 3, 3, 3], name
        if name == "xyz":  # a general direction: the covariance has rank 1 but is no diagonal, and the sweeps leave rounding dust
            assert (eig[:, 0] > 0).all() and (eig[:, 1:] <= 1e-15 * eig[:, :1]).all(), (name, eig)  # a few float64 roundings of l0
        else:
            assert (eig[:, 0] > 0).all() and (bits(eig)[:, 1:] == 0).all(), (name, eig)
        d = np.array(direction, np.float64) / np.linalg.norm(direction)
        assert np.abs(normal.astype(np.float64) @ d).max() < 1e-7 and np.abs((normal.astype(np.float64) ** 2).sum(1) - 1).max() < 1e-6, name
        out[name] = normal
    return out


def test_hand_pins_host():
    """The lattice at 0.25 (count 6, S = 0, M = diag 2^31, eig 1/48 three times), its z = 3 layer at 0.36 (count 8, M_zz = 0, l2 = 0,
    the normal (0, 0, 1) bit for bit, (0, 0, -1) towards a point below), a pair and a triple (NaN bits, the count kept), collinear
    triples -- through the host twin AND through the restatement's sums."""
    from gsplat import surface

    def estimate(pos, radius, toward):
        normal, eig, count, sums, info = surface.host_estimate(pos, radius, toward=toward)
        c, s, i = su.sums(pos, radius)
        assert np.array_equal(s, sums) and np.array_equal(c, count) and sums.dtype == np.int64 and count.dtype == np.uint32
        assert (info["queried"], info["sources"], info["unresolved"]) == (i["queried"], i["sources"], i["unresolved"])
        assert normal.dtype == eig.dtype == F and normal.shape == eig.shape == (pos.shape[0], 3)
        return normal, eig, count, sums
    check_lattice(estimate)


def test_quantisation_bound():
    """A neighbour at exactly the radius along one axis is accepted and |q| <= 2^16 + 1 for every accepted pair, at radii on both
    sides of a change of E: 0.25 and the float below (E = -1, -2), 1.0 and the float above (E = 1, 1); the scale changes where E does."""
    from gsplat import surface
    below, above = float(np.nextafter(F(0.25), F(0))), float(np.nextafter(F(1.0), F(2)))
    assert [su.scale(r)[:2] for r in (0.25, below, 1.0, above)] == [(-1, F(2.0 ** 17)), (-2, F(2.0 ** 18)), (1, F(2.0 ** 15)), (1, F(2.0 ** 15))]
    rng = np.random.default_rng(3)
    for radius, q_at_r in ((0.25, 2 ** 15), (below, 2 ** 16), (1.0, 2 ** 15), (above, 2 ** 15)):
        r32 = F(radius)
        for axis in range(3):
            e = np.zeros(3, F)
            e[axis] = r32
            cloud = (rng.uniform(-1, 1, (60, 3)) * float(r32)).astype(F)  # differences up to twice the radius: most pairs near the bound
            pos = np.concatenate([np.zeros((1, 3), F), e[None, :], -e[None, :], cloud])
            normal, eig, count, sums, info = surface.host_estimate(pos, radius, source=(0, 0), query=(0, 0))
            c, s, _ = su.sums(pos, radius)
            assert np.array_equal(s, sums) and np.array_equal(c, count)
            assert su.max_abs_q(pos, radius) <= 2 ** 16 + 1
            pair = pos[:2]
            _, _, cp, sp, _ = surface.host_estimate(pair, radius)
            assert cp.tolist() == [1, 1]  # exactly at the radius: inclusive
            assert sp[0, 1 + axis] == q_at_r == -sp[1, 1 + axis] and sp[0, (4, 7, 9)[axis]] == q_at_r ** 2, (radius, axis, sp)
            assert abs(int(sp[0, 1 + axis])) <= 2 ** 16 + 1
            assert (sums[:, 4] <= int(count.max()) * (2 ** 32 + 2 ** 18 + 1)).all()


SCENES = {"special": (special_pos, 0.5), "bicycle": (bicycle1000, BICYCLE_RADIUS), "sheet": (sheet_pos, 0.25)}
FILTERS = (((0, 0), (0, 0)), ((3, 1), (3, 2)))  # everyone; disjoint: a query that is no source


@pytest.mark.parametrize("name", list(SCENES))
def test_host_sums_bit_for_bit(name):
    """Sums, count and info of the host twin equal the restatement bit for bit, unfiltered and with disjoint sources and queries."""
    from gsplat import surface
    make, radius = SCENES[name]
    pos = make()
    st = (np.arange(pos.shape[0]) % 3).astype(np.uint8)
    for source, query in FILTERS:
        c, s, i = want(name, pos, radius, st, source, query)
        normal, eig, count, sums, info = host(name, pos, radius, st, source, query)
        assert np.array_equal(sums, s) and np.array_equal(count, c), (name, source, int((sums != s).any(axis=1).sum()))
        assert (info["queried"], info["sources"], info["unresolved"]) == (i["queried"], i["sources"], i["unresolved"])
        qm = masks(st, source, query)[1]
        assert (count[~qm] == 0).all() and (sums[~qm] == 0).all() and nan6(normal, eig, ~qm | (count < 3))
        assert np.isfinite(normal[qm & (count >= 3)]).all() and np.isfinite(eig[qm & (count >= 3)]).all()
    if name == "special":
        c, _, i = want(name, pos, radius, st)
        assert (c[[10, 20, 30, 70, 71]] == 0).all() and i["unresolved"] >= 5  # non-finite: no neighbours, nobody's, unresolved


def check_model(normal, eig, count, sums, radius, expect_queries, min_gap):
    """Eigenvalues and normals against the float64 model within the module's two bounds; the gap rule may leave out no query."""
    me, mn = su.model(sums, radius)
    ok = count >= 3
    assert int(ok.sum()) == expect_queries
    l, m = eig[ok].astype(np.float64), me[ok]
    assert (l[:, 0] >= l[:, 1]).all() and (l[:, 1] >= l[:, 2]).all() and (l[:, 2] >= 0).all()
    err, bound = np.abs(l - m), 2.0 ** -23 * np.abs(m) + 1e-12 * m[:, :1]
    print("eigenvalues: worst error / bound %.3g" % float((err / bound).max()))
    assert (err <= bound).all()
    gap = (m[:, 1] - m[:, 2]) / m[:, 0]
    print("smallest relative gap %.4g, mean count %.3g" % (float(gap.min()), float(count[ok].mean())))
    assert gap.min() >= min_gap >= 1e-2  # no query is left out
    dot = (normal[ok].astype(np.float64) * mn[ok]).sum(axis=1)
    print("normals: smallest |n . n_model| = 1 - %.3g" % float(1 - np.abs(dot).min()))
    assert (np.abs(dot) >= 1 - 1e-6).all()
    big = np.argmax(np.abs(normal[ok]), axis=1)
    assert (normal[ok][np.arange(big.size), big] > 0).all()  # the sign rule


@pytest.mark.parametrize("name,queries,min_gap", [("bicycle", 677, 0.017), ("sheet", 1500, 0.144)])
def test_host_finishing_against_model(name, queries, min_gap):
    make, radius = SCENES[name]
    pos = make()
    normal, eig, count, sums, _ = host(name, pos, radius, (np.arange(pos.shape[0]) % 3).astype(np.uint8))
    check_model(normal, eig, count, sums, radius, queries, min_gap)
    if name == "sheet":  # a sheet is planar: the feature an editor selects by
        assert np.median(su.feature("planarity", normal, eig, count)) > 0.5 and np.median(su.feature("variation", normal, eig, count)) < 1e-3


def test_orient_restated_host():
    """GS_SURFACE_ORIENT is the f32 rule on the unoriented planes, bit for bit; eigenvalues, count and sums do not change."""
    pos = sheet_pos()
    plain = host("sheet", pos, 0.25, (np.arange(1500) % 3).astype(np.uint8))
    for toward in ((0.0, 0.0, 0.0), (3.0, -1.0, 20.0), (float("nan"), 0.0, 0.0)):
        got = host("sheet", pos, 0.25, (np.arange(1500) % 3).astype(np.uint8), toward=toward)
        assert np.array_equal(bits(got[0]), bits(su.orient(plain[0], pos, toward))), toward
        assert np.array_equal(bits(got[1]), bits(plain[1])) and np.array_equal(got[2], plain[2]) and np.array_equal(got[3], plain[3])
    flipped = su.orient(plain[0], pos, (0.0, 0.0, 0.0))
    assert 0 < (bits(flipped) != bits(plain[0])).any(axis=1).sum()


def test_surface_abi(tmp_path):
    """The five symbols are exported and listed; the three structs have the same size and offsets in the compiled header and in
    ctypes; the constants agree; GS_ABI_VERSION is still 3; the header states the definition; a null context and every bad argument of
    the host twin are refused by name with a message that names the number; no Renderer methods, no Node exports."""
    import gsplat
    from gsplat import _abi, surface
    L = _abi.load()
    names = ("gs_surface_estimate", "gs_surface_read", "gs_surface_read_sums", "gs_state_surface", "gs_surface_host")
    for name in names:
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    layouts = (("gs_surface", _abi.GsSurface, 56, [0, 4, 8, 12, 16, 20, 24, 28, 40, 48]),
               ("gs_surface_info", _abi.GsSurfaceInfo, 48, [0, 8, 16, 24, 32, 44]),
               ("gs_surface_range", _abi.GsSurfaceRange, 32, [0, 4, 8, 12, 16, 20]))
    prog = 'printf("%d", GS_ABI_VERSION);'
    for cname, cls, _, _ in layouts:
        prog += 'printf(" %%zu", sizeof(%s));' % cname + "".join('printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f, _ in cls._fields_)
    prog += ('printf(" %u %u %u %u %u %u %u %u %u %u", GS_SURFACE_ORIENT, GS_SURFACE_KEEP_SUMS, GS_SURFACE_SUM_WORDS, GS_SURFACE_VARIATION, GS_SURFACE_PLANARITY,'
             "GS_SURFACE_LINEARITY, GS_SURFACE_SPHERICITY, GS_SURFACE_FACING, GS_SURFACE_FACING_SIGNED, GS_SURFACE_COUNT);")
    out = c_layout(tmp_path, "surface_layout", prog)
    assert out[0] == 3 and L.gs_abi_version() == 3
    at = 1
    for cname, cls, size, offsets in layouts:
        k = len(cls._fields_)
        assert out[at] == size == ctypes.sizeof(cls), cname
        assert out[at + 1:at + 1 + k] == offsets == [getattr(cls, f).offset for f, _ in cls._fields_], cname
        at += 1 + k
    assert out[at:] == [1, 2, 10, 0, 1, 2, 3, 4, 5, 6]
    assert (_abi.GS_SURFACE_ORIENT, _abi.GS_SURFACE_KEEP_SUMS, _abi.GS_SURFACE_SUM_WORDS) == (1, 2, 10) == (1, 2, surface.SUM_WORDS)
    assert [surface.KINDS[k] for k in su.KINDS] == list(range(7)) == [getattr(_abi, "GS_SURFACE_" + k.upper()) for k in su.KINDS]
    rjs, idx, dts, napi, hdr = host_sources()
    for name in names:
        assert name + "(" in hdr and name not in napi  # no Node exports: the N-API surface is pinned
    assert hdr.index("---- cell merge") < hdr.index("---- surface") < hdr.index("Tuning / profiling knobs")
    sec = hdr[hdr.index("---- surface"):hdr.index("Tuning / profiling knobs")]
    for text in ("d2 = (dx dx + dy dy) + dz dz", "d = p_j - p_i", "r2 = radius * radius", "INCLUSIVE", "frexpf(radius)", "s = 2^(16 - E)",
                 "q_a = (int32) rintf(d_a * s)", "ONE quantisation", "|q_a| <= 2^16 + 1", "2^32 + 2^18 + 1", "2^63", "no wrap and no saturation",
                 "mu_a = (double)S_a / n", "C_ab = (double)M_ab / n - mu_a * mu_b", "Jacobi", "l0 >= l1 >= l2", "l >= 0 ? l : 0", "2^(2 (E - 16))",
                 "largest magnitude is positive", "the lowest axis", "t = (nx ex + ny ey) + nz ez", "0x7FC00000", "count < 3", "DROPPED", "gs_upload_*",
                 "gs_share_splats", "gs_compact", "as they were", "GS_ERR_CAPACITY", "l2 / ((l0 + l1) + l2)", "(l1 - l2) / l0", "(l0 - l1) / l0", "l2 / l0",
                 "fabsf((nx ax + ny ay) + nz az)", "16 - E > 127"):
        assert text in sec, text
    q, info, n, rg = _abi.GsSurface(), _abi.GsSurfaceInfo(), ctypes.c_uint64(), _abi.GsSurfaceRange()
    calls = {"gs_surface_estimate": lambda: L.gs_surface_estimate(None, ctypes.byref(q), ctypes.byref(info)),
             "gs_surface_read": lambda: L.gs_surface_read(None, None, None, None, 0, ctypes.byref(n)),
             "gs_surface_read_sums": lambda: L.gs_surface_read_sums(None, None, 0, ctypes.byref(n)),
             "gs_state_surface": lambda: L.gs_state_surface(None, ctypes.byref(rg), 0, 0, 1, 2, None)}
    for name, call in calls.items():
        assert call() == _abi.GS_ERR_INVALID_ARGUMENT
        msg = L.gs_last_error()
        assert name.encode() in msg and b"null ctx" in msg
    # the host twin's refusals are the estimate's: the code, the call's name and the number
    pos = lattice_pos()
    good = surface.host_estimate(pos, 0.25)
    for kw, fragments in ((dict(radius=float("nan")), ("radius nan",)), (dict(radius=float("inf")), ("radius inf",)), (dict(radius=-0.5), ("radius -0.5",)),
                          (dict(radius=0.0), ("radius 0", "not above 0")), (dict(radius=2e19), ("radius 2e+19", "squared")),
                          (dict(radius=1e-36), ("radius 1e-36", "2^135")), (dict(radius=1e-40), ("2^148",)),
                          (dict(source=(0x100, 0)), ("0x100", "does not fit the state byte")), (dict(query=(1, 0x1FF)), ("0x1ff", "does not fit the state byte")),
                          (dict(source=(1, 1)), ("null state",))):
        args = dict(radius=0.25)
        args.update(kw)
        code, msg = code_of(lambda: surface.host_estimate(pos, args.pop("radius"), **args))
        assert code == _abi.GS_ERR_INVALID_ARGUMENT and "gs_surface_host" in msg and all(f in msg for f in fragments), msg

    def raw(**kw):
        qq = surface._query(0.25, (0, 0), (0, 0), None, False, 0)
        for k, v in kw.items():
            setattr(qq, k, v)
        nv, ev, cnt = np.zeros((216, 3), F), np.zeros((216, 3), F), np.zeros(216, np.uint32)
        rc = L.gs_surface_host(pos.ctypes.data, None, 216, ctypes.byref(qq), nv.ctypes.data, ev.ctypes.data, cnt.ctypes.data, None, None)
        return rc, L.gs_last_error().decode(), cnt
    for kw, fragment in ((dict(struct_size=48), "struct_size 48"), (dict(flags=6), "flags 0x4"), (dict(flags=8), "flags 0x8"), (dict(reserved=5), "reserved 5")):
        rc, msg, cnt = raw(**kw)
        assert rc == _abi.GS_ERR_INVALID_ARGUMENT and "gs_surface_host" in msg and fragment in msg and not cnt.any(), msg
    rc, _, cnt = raw(flags=_abi.GS_SURFACE_KEEP_SUMS)  # sums and info may be null; the flag needs no plane here
    assert rc == 0 and np.array_equal(cnt, good[2])
    assert L.gs_surface_host(None, None, 0, ctypes.byref(surface._query(0.25, (0, 0), (0, 0), None, False, 0)), None, None, None, None, ctypes.byref(info)) == 0
    assert (info.queried, info.sources, info.candidates, info.unresolved) == (0, 0, 0, 0)
    assert gsplat.surface is surface
    for fn in ("estimate", "read", "read_sums", "select", "host_estimate", "radius_for", "select_planar", "select_facing", "select_fuzzy"):
        assert callable(getattr(surface, fn))
    for cls in (gsplat.Renderer, gsplat.PipelinedRenderer):
        assert not [m for m in dir(cls) if not m.startswith("_") and ("surface" in m.lower() or "normal" in m.lower() or "planar" in m.lower())]


def test_surface_check_sanitized(tmp_path):
    """tools/surface_check: gs_surface_math.h compiled alone with -fsanitize=address,undefined and run as its own process.  Skipped
    where the sanitizer runtime is not installed."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed")
    exe = str(tmp_path / "surface_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san +
                          ["-I", CSRC, os.path.join(ROOT, "tools", "surface_check", "main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout == "surface_check ok\n", out.stdout[-2000:] + out.stderr[-2000:]
    # a file of positions: its sums are the restatement's
    pos = special_pos()[:300]
    path = tmp_path / "pos.bin"
    pos.tofile(path)
    out = subprocess.run([exe, str(path), repr(0.5)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = np.array([int(x) for x in out.stdout.split()], np.int64).reshape(-1, 10)
    assert np.array_equal(got, su.sums(pos, 0.5)[1])


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def check_estimate(r, key, pos, radius, st=None, source=(0, 0), query=(0, 0), toward=None, cells=None):
    """estimate(keep_sums=True) + read + read_sums: sums, count and info against the restatement, normal and eig against the host twin,
    all bit for bit; the count plane equals neighbours.count's.  Returns (normal, eig, count, sums, info)."""
    from gsplat import neighbours, surface
    n = pos.shape[0]
    c, s, i = want(key, pos, radius, st, source, query)
    hn, he, hc, hs, _ = host(key, pos, radius, st, source, query, toward)
    info = surface.estimate(r, radius, source=source, query=query, toward=toward, keep_sums=True)
    normal, eig, count = surface.read(r)
    sums = surface.read_sums(r)
    assert normal.dtype == eig.dtype == F and count.dtype == np.uint32 and sums.dtype == np.int64
    assert normal.shape == eig.shape == (n, 3) and count.shape == (n,) and sums.shape == (n, 10)
    cell = (key, radius, source, query)
    assert np.array_equal(sums, s), (cell, int((sums != s).any(axis=1).sum()))
    assert np.array_equal(count, c) and np.array_equal(count, hc), cell
    assert (info["queried"], info["sources"], info["unresolved"]) == (i["queried"], i["sources"], i["unresolved"]), (cell, info, i)
    assert np.array_equal(bits(eig), bits(he)), (cell, int((bits(eig) != bits(he)).any(axis=1).sum()))
    assert np.array_equal(bits(normal), bits(hn)), (cell, int((bits(normal) != bits(hn)).any(axis=1).sum()))
    if i["queried"] and i["sources"] and np.isfinite(pos).all():
        assert info["cell_edge"] >= 1.001 * radius
    if cells is not None:
        assert cells(info["cells"]), (cell, info)
    neighbours.count(r, radius, source=source, query=query)
    assert np.array_equal(neighbours.read(r), c), cell
    print("%s radius %g: unresolved %d, cells %s, candidates %d, largest count %d" % (key, radius, info["unresolved"], info["cells"], info["candidates"], int(c.max(initial=0))))
    return normal, eig, count, sums, info


@pytest.mark.gpu
def test_lattice_and_lines():
    """The CPU test's hand pins on the device; the collinear triples' normals equal the host twin's bit for bit."""
    from gsplat import surface

    def estimate(pos, radius, toward):
        r = _mk(records(pos), 64, 64, 16)
        normal, eig, count = surface.read(r)  # before any estimate
        assert nan6(normal, eig, slice(None)) and not count.any()
        surface.estimate(r, radius, toward=toward, keep_sums=True)
        normal, eig, count = surface.read(r)
        sums = surface.read_sums(r)
        hn, he, hc, hs, _ = surface.host_estimate(pos, radius, toward=toward)
        assert np.array_equal(bits(normal), bits(hn)) and np.array_equal(bits(eig), bits(he)) and np.array_equal(sums, hs) and np.array_equal(count, hc)
        r.destroy()
        return normal, eig, count, sums
    check_lattice(estimate)
    p = lattice_pos()
    r = _mk(records(p), 64, 64, 16)
    for radius in (0.25, float(np.nextafter(F(0.25), F(0))), 0.36, 0.5):
        check_estimate(r, "lattice", p, radius)
    r.destroy()


@pytest.mark.gpu
def test_special_floats():
    """NaN, infinities, -0.0, a denormal and duplicates among the coordinates, with and without a far outlier that coarsens the grid."""
    from gsplat import surface
    p = special_pos()
    n = p.shape[0]
    far = np.concatenate([p, np.array([[1e6, 1e6, -1e6]], F)])
    r, rf = _mk(records(p), 64, 64, 16), _mk(records(far), 64, 64, 16)
    for radius in (0.5, 0.1, 1e-30, 100.0):
        normal, eig, count, sums, info = check_estimate(r, "special", p, radius)
        surface.estimate(rf, radius, keep_sums=True)
        fn, fe, fc = surface.read(rf)
        assert np.array_equal(bits(fn)[:n], bits(normal)) and np.array_equal(bits(fe)[:n], bits(eig)) and np.array_equal(fc[:n], count)
        assert np.array_equal(surface.read_sums(rf)[:n], sums) and fc[n] == 0 and nan6(fn, fe, [n])
        assert (count[[10, 20, 30, 70, 71]] == 0).all() and nan6(normal, eig, [10, 20, 30, 70, 71])
    r.destroy()
    rf.destroy()


@pytest.mark.gpu
def test_ragged_scene_many_cells_and_one():
    """bicycle_like(3001)[:1000] at the radius of the finishing test (many cells: per-lane walks), at 1e3 (ONE cell: uniform waves,
    every count 999) and at a radius with a few cells; the device's finishing is also held to the model."""
    pos = bicycle1000()
    r = _mk(records(pos), 64, 64, 16)
    normal, eig, count, sums, _ = check_estimate(r, "bicycle", pos, BICYCLE_RADIUS, cells=lambda c: min(c) > 1)
    check_model(normal, eig, count, sums, BICYCLE_RADIUS, 677, 0.017)
    _, _, count, _, _ = check_estimate(r, "bicycle", pos, 1e3, cells=lambda c: c == (1, 1, 1))
    assert (count == 999).all()
    check_estimate(r, "bicycle", pos, 6.0, cells=lambda c: 1 < max(c) < 12)
    r.destroy()
    pos = sheet_pos()
    r = _mk(records(pos), 64, 64, 16)
    normal, eig, count, sums, _ = check_estimate(r, "sheet", pos, 0.25)
    check_model(normal, eig, count, sums, 0.25, 1500, 0.144)
    r.destroy()


@pytest.mark.gpu
def test_blocked_table_and_dense_cell():
    """More than 2^24 cells (the table indexed by blocks, a cell's run found by binary search) with a knot of 200 splats in one cell --
    whole waves whose queries share a cell -- next to waves that straddle cells; the same scene without the far ends."""
    p = knot_pos()
    r = _mk(records(p), 64, 64, 16)
    for radius in (0.25, 0.36):
        _, _, count, _, _ = check_estimate(r, "knot", p, radius, cells=lambda c: min(c) > 256 and c[0] * c[1] * c[2] > 2 ** 24)
        assert (count[216:416] == 199).all()
    r.destroy()
    p = p[:-2]
    r = _mk(records(p), 64, 64, 16)
    _, _, count, _, _ = check_estimate(r, "knot_near", p, 0.25, cells=lambda c: c[0] * c[1] * c[2] < 2 ** 24)
    assert (count[216:416] == 199).all()
    r.destroy()


@pytest.mark.gpu
def test_tiny_scenes():
    """N = 0, 1, 2, 3, 4 (the first with three neighbours) and 257 queries: no multiple of 64 or 256."""
    from gsplat import _abi, surface
    L = _abi.load()
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(_abi.GsConfig), 64, 64, 16, _abi.GS_FLAG_SPLAT_STATE
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    q, info, nn, m = surface._query(0.5, (0, 0), (0, 0), None, True, 0), _abi.GsSurfaceInfo(), ctypes.c_uint64(9), ctypes.c_uint64(77)
    rg = _abi.GsSurfaceRange()
    rg.struct_size, rg.kind, rg.lo, rg.hi, rg.inside = ctypes.sizeof(rg), 0, 0.0, 1.0, 1
    assert L.gs_surface_estimate(ctx, ctypes.byref(q), ctypes.byref(info)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_surface_read(ctx, None, None, None, 0, ctypes.byref(nn)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_surface_read_sums(ctx, None, 0, ctypes.byref(nn)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_state_surface(ctx, ctypes.byref(rg), 0, 0, 1, 2, None) == _abi.GS_ERR_NO_SCENE
    _abi.check(L.gs_upload_splats(ctx, None, 0))
    info.queried = info.candidates = info.unresolved = 9
    _abi.check(L.gs_surface_estimate(ctx, ctypes.byref(q), ctypes.byref(info)))
    assert (info.queried, info.sources, info.candidates, info.unresolved) == (0, 0, 0, 0)
    _abi.check(L.gs_surface_estimate(ctx, ctypes.byref(q), None))
    _abi.check(L.gs_surface_read(ctx, None, None, None, 0, ctypes.byref(nn)))
    assert nn.value == 0
    nn.value = 9
    _abi.check(L.gs_surface_read_sums(ctx, None, 0, ctypes.byref(nn)))
    assert nn.value == 0
    _abi.check(L.gs_state_surface(ctx, ctypes.byref(rg), 0, 0, 1, 2, ctypes.byref(m)))
    assert m.value == 0
    L.gs_destroy(ctx)
    tet = np.array([[1, 1, 1], [1.25, 1, 1], [1, 1.25, 1], [1, 1, 1.25], [1.125, 1.125, 1.125]], F)
    for k in (1, 2, 3, 4, 5):
        r = _mk(records(tet[:k]), 64, 64, 16)
        normal, eig, count, _, info = check_estimate(r, "tet%d" % k, tet[:k], 0.5)
        assert (count == k - 1).all() and info["unresolved"] == (k if k < 4 else 0) and nan6(normal, eig, slice(None)) == (k < 4)
        r.destroy()
    pos = bicycle1000()[:257]
    r = _mk(records(pos), 64, 64, 16)
    check_estimate(r, "bicycle257", pos, 2.0)
    check_estimate(r, "bicycle257", pos, 1e3, cells=lambda c: c == (1, 1, 1))
    r.destroy()


@pytest.mark.gpu
def test_filters():
    """Disjoint, overlapping and equal sources and queries, none of either; non-queries read NaN, count 0 and zero sums; (0, 0) on a
    ctx without the state plane."""
    from gsplat import surface
    pos = bicycle1000()
    n = pos.shape[0]
    st = (np.arange(n) % 5).astype(np.uint8)
    r = _mk(records(pos), 64, 64, 16)
    r.write_state(st)
    for radius in (BICYCLE_RADIUS, 1e3):
        for source, query in (((7, 1), (7, 2)), ((1, 0), (1, 0)), ((1, 0), (4, 0)), ((0, 0), (7, 3))):
            normal, eig, count, sums, info = check_estimate(r, "bicycle5", pos, radius, st, source, query)
            qm = masks(st, source, query)[1]
            assert nan6(normal, eig, ~qm) and not count[~qm].any() and not sums[~qm].any()
    info = surface.estimate(r, 0.5, source=(0xFF, 0xEE), keep_sums=True)
    normal, eig, count = surface.read(r)
    assert info["sources"] == 0 and info["queried"] == info["unresolved"] == n and nan6(normal, eig, slice(None)) and not count.any()
    assert not surface.read_sums(r).any()
    info = surface.estimate(r, 0.5, query=(0xFF, 0xEE))
    normal, eig, count = surface.read(r)
    assert info["queried"] == info["unresolved"] == 0 and nan6(normal, eig, slice(None)) and not count.any()
    np.testing.assert_array_equal(r.read_state(), st)
    r.destroy()
    q = mk(records(pos), 64, 64, 16)  # without GS_FLAG_SPLAT_STATE
    check_estimate(q, "bicycle", pos, BICYCLE_RADIUS)
    before = surface.read(q)
    for fn in (lambda: surface.estimate(q, 0.5, source=(1, 0)), lambda: surface.estimate(q, 0.5, query=(1, 1)), lambda: surface.select(q, "count", 0, 1)):
        code, msg = code_of(fn)
        assert code == -1 and "GS_FLAG_SPLAT_STATE" in msg
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(surface.read(q), before))
    q.destroy()


@pytest.mark.gpu
def test_orient_restated():
    """GS_SURFACE_ORIENT restated from the unoriented planes bit for bit; eig and count unchanged."""
    from gsplat import surface
    pos = sheet_pos()
    r = _mk(records(pos), 64, 64, 16)
    surface.estimate(r, 0.25)
    plain = surface.read(r)
    for toward in ((0.0, 0.0, 0.0), (3.0, -1.0, 20.0), (float("nan"), 0.0, 0.0)):
        surface.estimate(r, 0.25, toward=toward)
        got = surface.read(r)
        assert np.array_equal(bits(got[0]), bits(su.orient(plain[0], pos, toward))), toward
        assert np.array_equal(bits(got[1]), bits(plain[1])) and np.array_equal(got[2], plain[2])
    r.destroy()


@pytest.mark.gpu
def test_runs_slab_and_borrower_agree():
    """Two runs, an estimate without kept sums (the slice's scratch), a slab ctx and a borrower of gs_share_splats agree bit for bit."""
    from gsplat import surface
    pos = bicycle1000()
    rec = records(pos)
    owner = _mk(rec, 64, 64, 16)
    first = check_estimate(owner, "bicycle", pos, BICYCLE_RADIUS)
    again = check_estimate(owner, "bicycle", pos, BICYCLE_RADIUS)
    surface.estimate(owner, BICYCLE_RADIUS)  # no kept sums: another addressing of the same words
    plain = surface.read(owner)
    for a, b, c in zip(first[:3], again[:3], plain):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    slab = _mk(rec, 256, 256, 16, cols=SLAB_COLS[16])
    check_estimate(slab, "bicycle", pos, BICYCLE_RADIUS)
    slab.destroy()
    borrower = _mk(rec, 64, 64, 16, share_with=owner)
    normal, eig, count = surface.read(borrower)
    assert nan6(normal, eig, slice(None)) and not count.any()  # the borrower keeps its own planes
    check_estimate(borrower, "bicycle", pos, 1e3)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(surface.read(owner), plain))
    borrower.destroy()
    owner.destroy()


@pytest.mark.gpu
def test_state_surface():
    """Every kind x op against the restatement of the READ planes, matched included: inside 0 and 1, a where filter, infinite bounds,
    the NaN splats in no range, the empty range."""
    from gsplat import surface
    pos = bicycle1000()
    n = pos.shape[0]
    qm = np.arange(n) % 4 != 0
    st0 = np.where(qm, 0, 0x40).astype(np.uint8)
    st = (np.random.default_rng(7).integers(0, 256, n) & 0xBF).astype(np.uint8) | st0
    r = _mk(records(pos), 64, 64, 16)
    r.write_state(st0)
    surface.estimate(r, BICYCLE_RADIUS, query=(0x40, 0))
    normal, eig, count = surface.read(r)
    assert nan6(normal, eig, ~qm) and 0 < int((count >= 3).sum()) < int(qm.sum())
    axis = (0.6, -0.48, 0.64)
    for ki, kind in enumerate(su.KINDS):
        v = su.feature(kind, normal, eig, count, axis)
        fin = v[np.isfinite(v)]
        assert fin.size > 100
        med = float(np.median(fin))
        ranges = [(float(fin.min()), med), (med, INF), (-INF, INF), (med, float(fin.min()) - 1.0), (float(np.nextafter(F(med), F(INF))), 3.0e38)]
        for k, (lo, hi) in enumerate(ranges):
            for inside in (True, False):
                for op in OPS:
                    b = (0x02, 0xA4)[(k + op) % 2]
                    where = ((0, 0), (0x0C, 0x04), (0x30, 0x10))[(k + op + int(inside) + ki) % 3]
                    r.write_state(st)
                    member = su.member(v, lo, hi, inside)
                    new, matched = sr.apply_region(st, member, op, b, where)
                    cell = (kind, lo, hi, inside, op, b, where)
                    assert surface.select(r, kind, lo, hi, inside, axis, where, op, b) == matched, cell
                    np.testing.assert_array_equal(r.read_state(), new, err_msg=str(cell))
                    if inside and kind != "count":
                        assert not member[np.isnan(v)].any() and not member[~qm].any()  # a NaN is in no range
                    if lo > hi:
                        assert member.sum() == (0 if inside else n)
    got = surface.read(r)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, (normal, eig, count)))  # the selection only reads the planes
    # the verbs: planar splats of a sheet, the ones facing its normal, nothing fuzzy
    r.destroy()
    pos = sheet_pos()
    r = _mk(records(pos), 64, 64, 16)
    hn, he, hc, _, _ = host("sheet", pos, 0.25, (np.arange(1500) % 3).astype(np.uint8))
    assert surface.select_planar(r, 0.25, 0.5) == int(su.member(su.feature("planarity", hn, he, hc), 0.5, INF).sum()) > 1000
    up = np.median(hn, axis=0).astype(np.float64)
    a32 = (up / math.sqrt(float((up * up).sum()))).astype(F)
    cos = F(math.cos(math.radians(5.0)))
    r.clear_selection()
    assert surface.select_facing(r, up, 5.0) == int(su.member(su.feature("facing", hn, he, hc, a32), cos, INF).sum()) > 1000
    r.clear_selection()
    assert surface.select_facing(r, -up, 5.0, signed=True) == int(su.member(su.feature("facing_signed", hn, he, hc, -a32), cos, INF).sum())
    r.clear_selection()
    assert surface.select_fuzzy(r, 0.25, 0.1) == int(su.member(su.feature("variation", hn, he, hc), 0.1, INF).sum()) == 0
    assert surface.select_fuzzy(r, 0.25, 1e-4) == int(su.member(su.feature("variation", hn, he, hc), 1e-4, INF).sum()) > 100
    rad = surface.radius_for(r, 30)
    assert 0.1 < rad < 0.4  # 1500 points on 4 square units: 30 neighbours within sqrt(30 * 4 / (1500 pi)) = 0.16
    r.destroy()


@pytest.mark.gpu
def test_lifecycle():
    """The planes read NaN / 0 before the first estimate and after an upload, compact and share_splats, and the kept sums go with them
    and with the next estimate without the flag; state calls and translate_selected leave them; the other features' planes are
    unchanged by an estimate and the estimate's by them."""
    from gsplat import _abi, clusters, nearest, neighbours, surface
    pos = bicycle1000()
    rec = records(pos)
    n = pos.shape[0]

    def blank(r, m):
        normal, eig, count = surface.read(r)
        code, msg = code_of(lambda: surface.read_sums(r))
        return normal.shape == eig.shape == (m, 3) and nan6(normal, eig, slice(None)) and not count.any() and code == -1 and "GS_SURFACE_KEEP_SUMS" in msg

    def same(r, ref):
        return all(np.array_equal(bits(a), bits(b)) for a, b in zip(surface.read(r), ref[:3]))
    owner = _mk(rec, 64, 64, 16)
    assert blank(owner, n)
    ref = check_estimate(owner, "bicycle", pos, BICYCLE_RADIUS)
    borrower = _mk(rec, 64, 64, 16, share_with=owner)
    assert blank(borrower, n)
    check_estimate(borrower, "bicycle", pos, BICYCLE_RADIUS)
    _abi.check(borrower._L.gs_share_splats(borrower._ctx, owner._ctx))  # sharing again drops the borrower's planes and sums ...
    assert blank(borrower, n) and same(owner, ref) and np.array_equal(surface.read_sums(owner), ref[3])  # ... and not the owner's
    borrower.destroy()
    # an estimate without the flag drops the sums, and only the sums
    surface.estimate(owner, BICYCLE_RADIUS)
    code, msg = code_of(lambda: surface.read_sums(owner))
    assert code == -1 and "gs_surface_read_sums" in msg and "0x2" in msg and same(owner, ref)
    surface.estimate(owner, BICYCLE_RADIUS, keep_sums=True)
    # the other planes are unchanged by an estimate, and vice versa
    neighbours.count(owner, 0.5)
    clusters.label(owner, 0.5)
    nearest.search(owner, 3, 0.5)
    others = (neighbours.read(owner),) + clusters.read(owner) + nearest.read(owner)
    assert same(owner, ref) and np.array_equal(surface.read_sums(owner), ref[3])
    surface.estimate(owner, 2.0)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((neighbours.read(owner),) + clusters.read(owner) + nearest.read(owner), others))
    surface.estimate(owner, BICYCLE_RADIUS, keep_sums=True)
    # state calls and transforms leave the planes; a new estimate sees the moved splats
    assert owner.select_sphere((0, 0, 0), 1.5) > 0
    owner.translate_selected((0.3, -0.2, 0.1))
    assert same(owner, ref) and np.array_equal(surface.read_sums(owner), ref[3])
    moved = np.ascontiguousarray(owner.export_splats()[:, 0:3])
    assert not np.array_equal(moved, pos)
    check_estimate(owner, "bicycle_moved", moved, BICYCLE_RADIUS)
    # compact and a re-upload drop the planes and the sums
    st = (np.arange(n) % 3 == 0).astype(np.uint8) * 4
    owner.write_state(st)
    kept = owner.compact(4, 4)
    assert kept.size == int((st == 4).sum()) and blank(owner, kept.size)
    check_estimate(owner, "bicycle_kept", np.ascontiguousarray(moved[kept]), BICYCLE_RADIUS)
    arr = np.ascontiguousarray(rec[:600])
    _abi.check(owner._L.gs_upload_splats(owner._ctx, arr.ctypes.data, 600))
    assert blank(owner, 600)
    owner.destroy()


@pytest.mark.gpu
def test_estimate_disturbs_no_frame():
    """A frame rendered before and after an estimate and a selection that changes nothing is byte-identical in every tap, and the
    statistics are unchanged."""
    from gsplat import surface
    s, u, W, H = state_scene("ragged")
    a, b = _mk(s, W, H, 8), _mk(s, W, H, 8)
    before = frame_taps(a, u, False)
    frame_taps(b, u, False)
    for _ in range(3):  # three frames in flight on both; no wait: the estimate drains the ring
        a.render_uniforms(u)
        b.render_uniforms(u)
    info = surface.estimate(a, 0.5, toward=(0, 0, 0), keep_sums=True)
    assert info["queried"] == s.shape[0] and surface.read_sums(a).any()
    assert surface.select(a, "planarity", 5.0, 1.0, op=sr.SET, bits=sr.HIDDEN) == 0  # the empty range
    ta, tb = frame_taps(a, u, False), frame_taps(b, u, False)
    for k in ta:
        np.testing.assert_array_equal(ta[k], tb[k], err_msg=k)
        np.testing.assert_array_equal(ta[k], before[k], err_msg=k)
    assert timeless(a.stats()) == timeless(b.stats())
    a.destroy()
    b.destroy()


@pytest.mark.gpu
def test_budget_and_refusals():
    """max_candidates below info["candidates"] gives GS_ERR_CAPACITY with both numbers in the message, the planes and the kept sums as
    they were and info still written; every refusal leaves them as they were."""
    from gsplat import _abi, surface
    L = _abi.load()
    INV = _abi.GS_ERR_INVALID_ARGUMENT
    pos = bicycle1000()
    n = pos.shape[0]
    r = _mk(records(pos), 64, 64, 16)
    st = (np.arange(n) % 5).astype(np.uint8)
    r.write_state(st)
    ref = check_estimate(r, "bicycle", pos, BICYCLE_RADIUS)
    done = ref[4]
    info, nn, m = _abi.GsSurfaceInfo(), ctypes.c_uint64(), ctypes.c_uint64(77)

    def untouched():
        return all(np.array_equal(bits(a), bits(b)) for a, b in zip(surface.read(r), ref[:3])) and np.array_equal(surface.read_sums(r), ref[3])
    for keep in (False, True):
        code, msg = code_of(lambda: surface.estimate(r, BICYCLE_RADIUS, keep_sums=keep, max_candidates=done["candidates"] - 1))
        assert code == _abi.GS_ERR_CAPACITY and "gs_surface_estimate" in msg and str(done["candidates"]) in msg and str(done["candidates"] - 1) in msg
        assert untouched()
    q = surface._query(BICYCLE_RADIUS, (0, 0), (0, 0), None, False, 1)
    assert L.gs_surface_estimate(r._ctx, ctypes.byref(q), ctypes.byref(info)) == _abi.GS_ERR_CAPACITY
    assert (info.candidates, info.sources, info.queried) == (done["candidates"], n, n) and tuple(info.cells) == done["cells"] and untouched()
    assert surface.estimate(r, BICYCLE_RADIUS, keep_sums=True, max_candidates=done["candidates"])["candidates"] == done["candidates"]

    def refused(name, call, *fragments, code=INV):
        assert call() == code, name
        msg = L.gs_last_error().decode()
        assert name in msg and all(f in msg for f in fragments), msg
        assert untouched()
        np.testing.assert_array_equal(r.read_state(), st)

    def query(**kw):
        qq = surface._query(0.5, (0, 0), (0, 0), None, False, 0)
        for k, v in kw.items():
            setattr(qq, k, v)
        return qq
    est = lambda qq: (lambda: L.gs_surface_estimate(r._ctx, ctypes.byref(qq) if qq is not None else None, ctypes.byref(info)))
    refused("gs_surface_estimate", est(None), "null query")
    refused("gs_surface_estimate", est(query(struct_size=48)), "struct_size 48")
    refused("gs_surface_estimate", est(query(radius=float("nan"))), "radius nan")
    refused("gs_surface_estimate", est(query(radius=float("inf"))), "radius inf")
    refused("gs_surface_estimate", est(query(radius=-0.5)), "radius -0.5")
    refused("gs_surface_estimate", est(query(radius=0.0)), "radius 0", "not above 0")
    refused("gs_surface_estimate", est(query(radius=2e19)), "radius 2e+19", "squared")
    refused("gs_surface_estimate", est(query(radius=1e-36)), "radius 1e-36", "2^135")
    refused("gs_surface_estimate", est(query(flags=4)), "flags 0x4")
    refused("gs_surface_estimate", est(query(flags=11)), "flags 0x8")
    refused("gs_surface_estimate", est(query(reserved=5)), "reserved 5")
    refused("gs_surface_estimate", est(query(src_mask=0x100)), "0x100", "does not fit the state byte")
    refused("gs_surface_estimate", est(query(qry_value=0x1FF)), "0x1ff", "does not fit the state byte")
    refused("gs_surface_read", lambda: L.gs_surface_read(r._ctx, None, None, None, 0, None), "null n")
    bn, be, bc = np.full((n, 3), 0xA5A5A5A5, np.uint32), np.full((n, 3), 0xA5A5A5A5, np.uint32), np.full(n, 0xA5A5A5A5, np.uint32)
    refused("gs_surface_read", lambda: L.gs_surface_read(r._ctx, bn.ctypes.data, be.ctypes.data, bc.ctypes.data, n - 1, ctypes.byref(nn)), "%d splats per plane needed" % n)
    assert nn.value == n and (bn == 0xA5A5A5A5).all() and (be == 0xA5A5A5A5).all() and (bc == 0xA5A5A5A5).all()
    _abi.check(L.gs_surface_read(r._ctx, None, be.ctypes.data, None, n, ctypes.byref(nn)))  # each pointer may be null
    assert np.array_equal(be, bits(ref[1])) and (bn == 0xA5A5A5A5).all() and (bc == 0xA5A5A5A5).all()
    _abi.check(L.gs_surface_read(r._ctx, bn.ctypes.data, None, bc.ctypes.data, n, ctypes.byref(nn)))
    assert np.array_equal(bn, bits(ref[0])) and np.array_equal(bc, ref[2])
    bs = np.full((n, 10), -7, np.int64)
    refused("gs_surface_read_sums", lambda: L.gs_surface_read_sums(r._ctx, bs.ctypes.data, n - 1, ctypes.byref(nn)), "%d splats needed" % n)
    refused("gs_surface_read_sums", lambda: L.gs_surface_read_sums(r._ctx, None, 0, None), "null n")
    assert (bs == -7).all()
    # gs_state_surface's own: nothing is applied
    def sel(op=1, b=2, wm=0, **kw):
        rg = _abi.GsSurfaceRange()
        rg.struct_size, rg.kind, rg.lo, rg.hi, rg.inside = ctypes.sizeof(rg), 0, 0.0, 5.0, 1
        for k, v in kw.items():
            setattr(rg, k, v)
        return lambda: L.gs_state_surface(r._ctx, ctypes.byref(rg), wm, 0, op, b, ctypes.byref(m))
    refused("gs_state_surface", lambda: L.gs_state_surface(r._ctx, None, 0, 0, 1, 2, ctypes.byref(m)), "null range")
    refused("gs_state_surface", sel(struct_size=28), "struct_size 28")
    refused("gs_state_surface", sel(kind=7), "unknown kind 7")
    refused("gs_state_surface", sel(op=0), "unknown op 0")
    refused("gs_state_surface", sel(op=5), "unknown op 5")
    refused("gs_state_surface", sel(b=0x100), "0x100")
    refused("gs_state_surface", sel(wm=0x100), "where_mask 0x100")
    refused("gs_state_surface", sel(lo=float("nan")), "not a number")
    refused("gs_state_surface", sel(hi=float("nan")), "not a number")
    assert m.value == 77
    r.destroy()
