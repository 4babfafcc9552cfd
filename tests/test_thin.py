"""Thinning: a blue-noise subsample of resident splats by rank and radius (include/gsplat/gs_abi.h "thinning").

The reference every answer is held to is tests/thin_restate.py: all pairs with the header's f32 expression, the rank as Python
integers, the sequential greedy.  The CPU tests pin the restatement by hand (a lattice whose links sit exactly on the radius, special
floats, duplicates, the hash, the priority key), hold gs_thin_host -- another algorithm, a hashed grid of the kept members -- to it
over scenes x radii x orders x priorities x a filter, and check the ABI.  The GPU tests compare with np.array_equal on uint32 --
there is no tolerance anywhere -- over grids of many cells, of one and of more than 2^24, per-lane and wave-uniform walks, chains
4096 rounds long and the round cap, priorities read from the attribute kernels, placement, the selection, the verbs, the planes'
lifecycle, the work budget and the refusals.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import state_restate as sr
import thin_restate as tr
from conftest import scene
from support import F, ROOT, SLAB_COLS, c_layout, cached, code_of, frame_taps, host_sources, mk, state_scene, timeless

_mk = functools.partial(mk, state=True)
NONE = tr.NONE
OPS = (sr.SET, sr.CLEAR, sr.TOGGLE, sr.ASSIGN)
BELOW = float(np.nextafter(F(0.25), F(0)))
CSRC = os.path.join(ROOT, "gaussian-splatting-wgpu_amd", "csrc")
ORDERS = {"hash0": ("hash", 0), "hash1": ("hash", 12345), "index": ("index", 0)}
RADII = (0.5, 0.1, 100.0, 0.0, 1e-30)


def lattice_pos():
    """6 x 6 x 6 points, spacing 0.25, offset 3.0: every coordinate and every difference is exact in f32.  Index = 36 a + 6 b + c."""
    k = np.arange(6, dtype=F) * F(0.25) + F(3.0)
    return np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3).astype(F)


def records(pos):
    """Records of the synthetic scene with their centres replaced by `pos`."""
    pos = np.asarray(pos, F)
    rec = np.array(scene(10000)[:pos.shape[0]], dtype=F, copy=True)
    rec[:, 0:3] = pos
    return np.ascontiguousarray(rec)


def ragged():
    from gsplat import synth
    return cached("ragged_records", lambda: synth.bicycle_like(3001))


def special_pos():
    """1000 centres of the ragged scene with a NaN, +inf and -inf coordinate, -0.0, a denormal coordinate, a pair and a triple of
    exact duplicates and a pair of duplicates of non-finite splats (which are linked to nobody)."""
    p = np.array(ragged()[:1000, 0:3], dtype=F, copy=True)
    p[10, 0] = np.nan
    p[20, 1] = np.inf
    p[30, 2] = -np.inf
    p[40, 0] = -0.0
    p[50, 1] = 1e-45
    p[60] = p[61]
    p[70] = p[71] = (np.nan, 0.0, 0.0)
    p[80] = p[81] = p[82]
    return p


NONFINITE = (10, 20, 30, 70, 71)


def knot_pos():
    """The lattice, a knot of 200 splats within 0.01 (whole waves whose members share a cell, next to waves that straddle cells) and
    two far ends that push the grid past 2^24 cells at the lattice's radii."""
    ends = np.array([[-120, -121, -122], [123, 122, 121]], F)
    knot = (F(5.0) + np.random.default_rng(11).uniform(-0.005, 0.005, (200, 3))).astype(F)
    return np.concatenate([lattice_pos(), knot, ends])


def chain_pos():
    """x = 0.25 k, k < 4096: every value and every difference exact in f32."""
    p = np.zeros((4096, 3), F)
    p[:, 0] = np.arange(4096, dtype=F) * F(0.25)
    return p


def tied_priority(n):
    """Priority values with ties, NaNs of both signs, both zeros and both infinities."""
    v = (np.arange(n) % 5).astype(F) - F(2.0)
    rng = np.random.default_rng(5)
    v[rng.integers(0, n, max(n // 20, 1))] = np.nan
    if n > 8:
        v[1], v[2], v[3], v[4], v[5] = -np.nan, -0.0, 0.0, np.inf, -np.inf
    return v


def flags_of(order, ascending=False):
    return (tr.ORDER_INDEX if order == "index" else 0) | (tr.ASCENDING if ascending else 0)


def adj_of(key, pos, radius):
    return cached(("thin_adj", key, float(radius)), lambda: tr.links(pos, radius))


def want(key, pos, radius, members=None, priority=None, ascending=False, order="hash", seed=0, mkey=None, pkey=None):
    """The restatement, once per session; key names pos, mkey the members, pkey the priority values."""
    assert (members is None) == (mkey is None) and (priority is None) == (pkey is None)
    return cached(("thin", key, float(radius), mkey, pkey, ascending, order, seed),
                  lambda: tr.sample(pos, radius, members, priority, flags_of(order, ascending), seed, adj=adj_of(key, pos, radius)))


SCENES = {"lattice": lattice_pos, "special": special_pos, "ragged1000": lambda: np.ascontiguousarray(ragged()[:1000, 0:3])}


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def both(pos, radius, **kw):
    """(keeper, covers) of the restatement and of gs_thin_host, which must agree; returns one."""
    from gsplat import thin
    k, c = tr.sample(pos, radius, None, None, flags_of(kw.get("order", "hash")), kw.get("seed", 0))
    hk, hc, info = thin.host_sample(pos, radius, **kw)
    assert np.array_equal(k, hk) and np.array_equal(c, hc)
    assert (info["members"], info["kept"], info["dropped"], info["largest"]) == tr.info_counts(k, c)
    return k, c


def test_restatement_and_host_are_pinned():
    p = lattice_pos()
    a, b, c = np.unravel_index(np.arange(216), (6, 6, 6))
    even = (a + b + c) % 2 == 0
    k, cov = both(p, 0.25, order="index")
    assert k.dtype == cov.dtype == np.uint32
    assert np.array_equal(k == np.arange(216), even) and int(even.sum()) == 108  # kept: exactly the even points
    for i in np.flatnonzero(~even):  # a dropped point's keeper: its smallest-index kept face neighbour
        ai, bi, ci = a[i], b[i], c[i]
        face = [36 * x + 6 * y + z for x, y, z in ((ai - 1, bi, ci), (ai + 1, bi, ci), (ai, bi - 1, ci), (ai, bi + 1, ci), (ai, bi, ci - 1), (ai, bi, ci + 1))
                if 0 <= x < 6 and 0 <= y < 6 and 0 <= z < 6]
        assert k[i] == min(face), i
    assert cov.sum() == 216 and not cov[~even].any() and (cov[even] >= 1).all()
    k, cov = both(p, BELOW, order="index")
    assert np.array_equal(k, np.arange(216)) and (cov == 1).all()  # at the float below 0.25 everything is kept
    assert np.array_equal(tr.fixpoint(p, 0.25, flags=tr.ORDER_INDEX), even)
    # special floats
    s = special_pos()
    k, cov = both(s, 100.0)
    kept = np.flatnonzero(k == np.arange(1000))
    fin = np.setdiff1d(kept, NONFINITE)
    assert fin.size == 1 and sorted(set(kept) - set(fin)) == list(NONFINITE)  # one finite member plus exactly the non-finite ones
    assert cov[fin[0]] == 1000 - len(NONFINITE) and all(cov[i] == 1 for i in NONFINITE) and cov.sum() == 1000
    best = max(set(range(1000)) - set(NONFINITE), key=lambda i: tr.hash32(i))
    assert fin[0] == best  # ... the one with the largest hash
    for radius in (0.0, 1e-30):  # (1e-30: its square is 0)
        k, cov = both(s, radius)
        assert int((k[[60, 61]] == np.array([60, 61])).sum()) == 1 and int((k[[80, 81, 82]] == np.array([80, 81, 82])).sum()) == 1
        assert sorted(cov[[60, 61]].tolist()) == [0, 2] and sorted(cov[[80, 81, 82]].tolist()) == [0, 0, 3]
        assert int((k == np.arange(1000)).sum()) == 997 and k[70] == 70 and k[71] == 71  # duplicates of non-finite splats stay apart
        ki, _ = both(s, radius, order="index")
        assert ki[61] == 60 and ki[81] == ki[82] == 80  # index order: the lower index survives
    # the hash is a bijection on 0 .. 2^20 (vectorised; the scalar form is the header's text)
    h = tr.hash32_array(np.arange(1 << 20))
    assert np.unique(h).size == 1 << 20 and [int(v) for v in h[:50]] == [tr.hash32(i) for i in range(50)]
    assert np.unique(tr.hash32_array(np.arange(1 << 20), 12345)).size == 1 << 20 and int(tr.hash32_array([7], 12345)[0]) == tr.hash32(7, 12345)
    # a NaN priority never wins, in either direction; -0 < +0 in the key
    for nan in (np.nan, -np.nan, np.array([0x7F800001], np.uint32).view(F)[0]):
        assert tr.pkey(nan) == 0 and tr.pkey(nan, True) == 0
    for v in (-np.inf, -1.0, -0.0, 0.0, 1e-45, np.inf):
        assert tr.pkey(v) > 0 and tr.pkey(v, True) > 0
    assert tr.pkey(-0.0) < tr.pkey(0.0) and tr.pkey(-0.0, True) > tr.pkey(0.0, True) and tr.pkey(-np.inf) < tr.pkey(-1.0) < tr.pkey(1e-45) < tr.pkey(np.inf)
    two = np.array([[0, 0, 0], [0.5, 0, 0]], F)
    from gsplat import thin
    for ascending in (False, True):
        worst = np.inf if ascending else -np.inf
        for prio in ([np.nan, worst], [worst, -np.nan]):
            pr = np.array(prio, F)
            k, _ = tr.sample(two, 1.0, None, pr, flags_of("hash", ascending))
            hk, _, _ = thin.host_sample(two, 1.0, priority=pr, ascending=ascending)
            win = int(np.flatnonzero(~np.isnan(pr))[0])
            assert k.tolist() == hk.tolist() == [win, win], (ascending, prio)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_host_twin_equals_restatement(name):
    """gs_thin_host against the restatement: radii x {hash with two seeds, index} x {no priority, ties and NaNs, ascending} x a
    member filter; the iteration of the two fixpoint rules agrees with both on a part of them."""
    from gsplat import thin
    pos = SCENES[name]()
    n = pos.shape[0]
    prio = tied_priority(n)
    st = (4 * (np.arange(n) % 3 == 1) + 8 * (np.arange(n) % 2)).astype(np.uint8)  # bit 2 is the filter's; bit 3 is noise it must ignore
    mem = (st & 4) == 0
    for radius in RADII:
        adj = adj_of(name, pos, radius)
        for oname, (order, seed) in ORDERS.items():
            for pcase in ("none", "ties", "ascending"):
                pr, asc = (None if pcase == "none" else prio), pcase == "ascending"
                for filtered in (False, True):
                    cell = (name, radius, oname, pcase, filtered)
                    k, c = tr.sample(pos, radius, mem if filtered else None, pr, flags_of(order, asc), seed, adj=adj)
                    hk, hc, info = thin.host_sample(pos, radius, state=st if filtered else None, where=(4, 0) if filtered else (0, 0), priority=pr,
                                                    ascending=asc, order=order, seed=seed)
                    assert np.array_equal(hk, k), (cell, int((hk != k).sum()))
                    assert np.array_equal(hc, c), cell
                    assert (info["members"], info["kept"], info["dropped"], info["largest"]) == tr.info_counts(k, c), cell
                    assert int(c.sum()) == info["members"] == (int(mem.sum()) if filtered else n)
                    if oname != "hash1" and radius in (0.5, 0.0):
                        kept = tr.fixpoint(pos, radius, mem if filtered else None, pr, flags_of(order, asc), seed, adj=adj)
                        assert np.array_equal(kept, k == np.arange(n)), cell


def test_thin_abi(tmp_path):
    """The four symbols are exported and listed; gs_thin is 72 bytes and gs_thin_info 64 with the same offsets in the compiled header
    and in ctypes; the header states the definition; every refusal names its number; the Python host is a module and no method."""
    import gsplat
    from gsplat import _abi, thin
    L = _abi.load()
    names = ("gs_thin_sample", "gs_thin_read", "gs_state_thin", "gs_thin_host")
    for name in names:
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    q_fields = [n for n, _ in _abi.GsThin._fields_]
    i_fields = [n for n, _ in _abi.GsThinInfo._fields_]
    assert q_fields == ["struct_size", "radius", "mask", "value", "flags", "seed", "max_rounds", "reserved0", "max_candidates", "priority", "reserved"]
    assert i_fields == ["members", "kept", "dropped", "largest", "candidates", "rounds", "cells", "cell_edge", "reserved"]
    prog = 'printf("%d %d %zu %zu", GS_ABI_VERSION, (int)GS_ATTR_COUNT, sizeof(gs_thin), sizeof(gs_thin_info));'
    prog += "".join('printf(" %%zu", offsetof(gs_thin, %s));' % n for n in q_fields)
    prog += "".join('printf(" %%zu", offsetof(gs_thin_info, %s));' % n for n in i_fields)
    prog += 'printf(" %u %u %u %u %u", GS_THIN_NONE == 0xFFFFFFFFu, GS_THIN_NO_PRIORITY == 0xFFFFFFFFu, GS_THIN_ORDER_INDEX, GS_THIN_ASCENDING, GS_THIN_DEFAULT_ROUNDS);'
    out = c_layout(tmp_path, "thin_layout", prog)
    assert out[0] == 3 and L.gs_abi_version() == 3 and out[1] == 16 == _abi.GS_ATTR_COUNT
    assert out[2] == 72 == ctypes.sizeof(_abi.GsThin) and out[3] == 64 == ctypes.sizeof(_abi.GsThinInfo)
    assert out[4:15] == [getattr(_abi.GsThin, n).offset for n in q_fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 64]
    assert out[15:24] == [getattr(_abi.GsThinInfo, n).offset for n in i_fields] == [0, 8, 16, 24, 32, 40, 44, 56, 60]
    assert out[24:] == [1, 1, _abi.GS_THIN_ORDER_INDEX, _abi.GS_THIN_ASCENDING, _abi.GS_THIN_DEFAULT_ROUNDS]
    assert (_abi.GS_THIN_ORDER_INDEX, _abi.GS_THIN_ASCENDING) == (tr.ORDER_INDEX, tr.ASCENDING) and _abi.GS_THIN_NONE == NONE == thin.NONE
    hdr = host_sources().hdr
    for name in names:
        assert re.search(r"int32_t %s\(" % name, hdr)
    assert hdr.index("---- surface") < hdr.index("---- thinning") < hdr.index("Tuning / profiling knobs")
    sec = hdr[hdr.index("---- thinning"):hdr.index("Tuning / profiling knobs")]
    for text in ("d2 = (dx dx + dy dy) + dz dz", "d = p_j - p_i", "r2 = radius * radius", "INCLUSIVE", "R_i = (P_i << 32) | H_i", "OUTRANKS", "0x9E3779B9",
                 "0x7FEB352D", "0x846CA68B", "GS_THIN_NONE", "DROPPED", "gs_upload_*", "gs_share_splats", "gs_compact", "GS_ERR_CAPACITY",
                 "GS_THIN_DEFAULT_ROUNDS", "lexicographically first maximal independent set", "missing data never wins"):
        assert text in sec, text
    # every refusal of the host twin names its number; the device call refuses a null context by name
    x = np.zeros(2, F)
    k, c = np.full(2, 9, np.uint32), np.full(2, 9, np.uint32)

    def host(prio=None, **kw):
        q = thin._query(kw.pop("radius", 0.5), (kw.pop("mask", 0), kw.pop("value", 0)), None, False, "hash", 0, 0, 0, host=True)
        for name, v in kw.items():
            setattr(q, name, v)
        pr = None if prio is None else prio.ctypes.data
        return L.gs_thin_host(x.ctypes.data, x.ctypes.data, x.ctypes.data, 2, None, pr, ctypes.byref(q), k.ctypes.data, c.ctypes.data, None)

    cases = [(dict(struct_size=40), "struct_size 40"), (dict(radius=float("nan")), "radius nan"), (dict(radius=-0.5), "radius -0.5"),
             (dict(radius=float("inf")), "radius inf"), (dict(radius=2e19), "squared"), (dict(flags=4), "unknown flags 0x4"),
             (dict(flags=2), "GS_THIN_ASCENDING without a priority"), (dict(reserved0=5), "reserved0 = 5"),
             (dict(reserved=(ctypes.c_uint32 * 2)(0, 6)), "reserved[1] = 6"), (dict(mask=0x100), "0x100"), (dict(value=0x1FF), "0x1ff")]
    for kw, text in cases:
        assert host(**kw) == _abi.GS_ERR_INVALID_ARGUMENT, kw
        msg = L.gs_last_error().decode()
        assert "gs_thin_host:" in msg and text in msg, msg
        assert (k == 9).all() and (c == 9).all()
    wk, wc = tr.sample(np.zeros((2, 3), F), 0.5, priority=np.zeros(2, F), flags=2)
    assert host(np.zeros(2, F), flags=2) == 0 and k.tolist() == wk.tolist() and c.tolist() == wc.tolist() and sorted(wc.tolist()) == [0, 2]  # ascending WITH a priority
    q, info, n = thin._query(0.5, (0, 0), None, False, "hash", 0, 0, 0), _abi.GsThinInfo(), ctypes.c_uint64()
    calls = {"gs_thin_sample": lambda: L.gs_thin_sample(None, ctypes.byref(q), ctypes.byref(info)),
             "gs_thin_read": lambda: L.gs_thin_read(None, None, None, 0, ctypes.byref(n)),
             "gs_state_thin": lambda: L.gs_state_thin(None, 0, 1, 1, 0, 0, 1, 2, None)}
    for name, call in calls.items():
        assert call() == _abi.GS_ERR_INVALID_ARGUMENT
        msg = L.gs_last_error()
        assert (name + ":").encode() in msg and b"null ctx" in msg
    assert gsplat.thin is thin
    for fn in ("sample", "read", "select", "host_sample", "select_kept", "select_dropped", "decimate", "decimate_to", "dedupe", "spread"):
        assert callable(getattr(thin, fn))
    for cls in (gsplat.Renderer, gsplat.PipelinedRenderer):
        assert not [m for m in dir(cls) if "thin" in m.lower() or "decimate" in m.lower() or "dedupe" in m.lower()]


def test_thin_check_sanitized(tmp_path):
    """tools/thin_check: gs_thin_math.h compiled alone with -fsanitize=address,undefined and run as its own process.  Skipped where
    the sanitizer runtime is not installed."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed")
    exe = str(tmp_path / "thin_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san +
                          ["-I", CSRC, os.path.join(ROOT, "tools", "thin_check", "main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout == "thin_check ok\n", out.stdout[-2000:] + out.stderr[-2000:]
    # a file of positions: its planes are the restatement's
    pos = special_pos()[:300]
    path = tmp_path / "pos.bin"
    pos.tofile(path)
    for flags, seed in ((0, 0), (0, 12345), (1, 0)):
        out = subprocess.run([exe, str(path), repr(0.5), str(flags), str(seed)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        got = np.array([int(v) for v in out.stdout.split()], np.uint32).reshape(-1, 2)
        k, c = tr.sample(pos, 0.5, flags=flags, seed=seed)
        assert np.array_equal(got[:, 0], k) and np.array_equal(got[:, 1], c)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def check_sample(r, key, pos, radius, members=None, filt=(0, 0), mkey=None, priority=None, pvals=None, pkey=None, ascending=False, order="hash", seed=0,
                 many=None, max_rounds=0):
    """sample + read against the restatement, and the info numbers; priority: the GsAttr, pvals: its values as the restatement takes
    them; many: whether the grid must have more than one cell on every axis (True), exactly one (False), or either.  Returns the info."""
    from gsplat import thin
    wk, wc = want(key, pos, radius, members, pvals, ascending, order, seed, mkey, pkey)
    info = thin.sample(r, radius, filt, priority, ascending, order, seed, max_rounds)
    k, c = thin.read(r)
    print("%s radius %g %s/%d %s: %s" % (key, radius, order, seed, pkey, info))
    assert k.dtype == c.dtype == np.uint32
    assert np.array_equal(k, wk), (key, radius, order, int((k != wk).sum()))
    assert np.array_equal(c, wc), (key, radius, order, int((c != wc).sum()))
    assert (info["members"], info["kept"], info["dropped"], info["largest"]) == tr.info_counts(wk, wc), info
    assert int(c.sum()) == info["members"] and info["kept"] + info["dropped"] == info["members"]
    fin = np.isfinite(np.asarray(pos, F)).all(axis=1) & (np.ones(len(pos), bool) if members is None else np.asarray(members, bool))
    assert (info["rounds"] >= 1) == bool(fin.any()), info
    assert info["candidates"] >= int(fin.sum()), info  # every finite member had itself as a candidate
    if many is not None:
        assert (min(info["cells"]) > 1) if many else (info["cells"] == (1, 1, 1)), info
    if fin.any():
        assert info["cell_edge"] >= 1.001 * radius
    return info


@pytest.mark.gpu
@pytest.mark.parametrize("far", [False, True])
def test_lattice_and_special_floats(far):
    """The lattice (links exactly one radius long, across cell borders) and the special floats, with and without a far outlier that
    coarsens the grid: planes and info equal the restatement for hash and index order; the outlier changes nothing of the others."""
    from gsplat import thin
    out = np.array([[1e6, 1e6, -1e6]], F)
    for name, radii in (("lattice", (0.25, BELOW, 0.36)), ("special", (0.1, 100.0, 0.0, 1e-30))):
        base = SCENES[name]()
        n = base.shape[0]
        p = np.concatenate([base, out]) if far else base
        key = name + ("_far" if far else "")
        r = _mk(records(p), 64, 64, 16)
        k, c = thin.read(r)  # before any sample
        assert k.shape == c.shape == (p.shape[0],) and (k == NONE).all() and not c.any()
        for radius in radii:
            for order, seed in ORDERS.values():
                check_sample(r, key, p, radius, order=order, seed=seed)
                k, c = thin.read(r)
                wk, wc = want(name, base, radius, order=order, seed=seed)
                if far:  # the outlier is linked to nobody and a rank does not depend on N: the others' planes are those without it
                    assert np.array_equal(k[:n], wk) and np.array_equal(c[:n], wc) and (k[n], c[n]) == (n, 1)
                if name == "special":
                    assert all((k[i], c[i]) == (i, 1) for i in NONFINITE)
        if name == "lattice":
            check_sample(r, key, p, 0.25, order="index")
            k, _ = thin.read(r)
            a, b, c3 = np.unravel_index(np.arange(216), (6, 6, 6))
            assert np.array_equal(k[:216] == np.arange(216), (a + b + c3) % 2 == 0)
        r.destroy()
    q = np.full((5, 3), np.nan, F)  # nothing but non-finite members: no grid, all kept all the same
    r = _mk(records(q), 64, 64, 16)
    info = thin.sample(r, 0.5)
    k, c = thin.read(r)
    assert k.tolist() == [0, 1, 2, 3, 4] and c.tolist() == [1] * 5 and (info["members"], info["kept"], info["largest"], info["rounds"]) == (5, 5, 1, 0)
    r.destroy()


@pytest.mark.gpu
def test_ragged_radii_and_priorities():
    """synth.bicycle_like(3001)[:1000] at a many-cell radius (per-lane walks), 1e3 (ONE cell, wave-uniform walks, one finite member
    kept) and a few-cell radius; without a priority, with COVER_SUM after an accumulate_coverage, with OPACITY_LOGIT, and ascending:
    the device's priority values are the attribute kernels', the restatement takes them as read back."""
    from gsplat import _abi, attributes, thin
    s, u, W, H = state_scene("ragged")
    rec = np.ascontiguousarray(s[:1000])
    pos = np.ascontiguousarray(rec[:, 0:3])
    r = _mk(rec, W, H, 8)
    r.render_uniforms(u)
    r.wait()
    r.accumulate_coverage()
    cover, logit = attributes.attr(_abi.GS_ATTR_COVER_SUM), attributes.attr(_abi.GS_ATTR_OPACITY_LOGIT)
    cv, lv = attributes.values(r, cover), attributes.values(r, logit)
    assert cv.shape == lv.shape == (1000,) and (cv > 0).any() and (cv == 0).any()  # ties among the unseen
    st = (np.arange(1000) % 3).astype(np.uint8)
    r.write_state(st)
    for radius, many in ((0.1, True), (1e3, False), (2.0, None)):
        for order, seed in ORDERS.values():
            info = check_sample(r, "ragged1000", pos, radius, order=order, seed=seed, many=many)
            if radius == 1e3:
                assert (info["kept"], info["largest"], info["candidates"]) == (1, 1000, 10**6)
        check_sample(r, "ragged1000", pos, radius, priority=cover, pvals=cv, pkey="cover", many=many)
        check_sample(r, "ragged1000", pos, radius, priority=logit, pvals=lv, pkey="logit", order="index", many=many)
        check_sample(r, "ragged1000", pos, radius, priority=logit, pvals=lv, pkey="logit", ascending=True, seed=3, many=many)
        check_sample(r, "ragged1000", pos, radius, members=st == 1, filt=(3, 1), mkey="mod3", priority=cover, pvals=cv, pkey="cover", ascending=True)
    k, _ = thin.read(r)
    assert (k[st != 1] == NONE).all()
    # the most seen splat of the scene is kept whenever coverage ranks
    thin.sample(r, 1e3, priority=cover)
    k, c = thin.read(r)
    top = int(np.flatnonzero(cv == cv.max())[np.argmax([tr.hash32(int(i)) for i in np.flatnonzero(cv == cv.max())])])
    assert (k == top).all() and c[top] == 1000
    np.testing.assert_array_equal(r.read_state(), st)
    r.destroy()


@pytest.mark.gpu
def test_knot_and_blocked_table():
    """More than 2^24 cells (the table indexed by blocks, a cell's run found by binary search) with a knot of 200 splats in one cell --
    whole waves on the uniform path -- next to waves that straddle cells; radius above and below the knot's diameter."""
    p = knot_pos()
    r = _mk(records(p), 64, 64, 16)
    for radius in (0.25, 0.36, 0.004):
        for order, seed in ORDERS.values():
            info = check_sample(r, "knot", p, radius, order=order, seed=seed)
            assert min(info["cells"]) > 256 and info["cells"][0] * info["cells"][1] * info["cells"][2] > 2**24, info
        wk, _ = want("knot", p, radius)
        in_knot = int((wk[216:416] == np.arange(216, 416)).sum())
        assert (in_knot == 1) if radius >= 0.25 else (in_knot > 10), (radius, in_knot)  # above the diameter one survives, below it many
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 257])
def test_tiny_scenes(n):
    from gsplat import thin
    from gsplat import _abi
    if n == 0:  # an EMPTY scene: zero results, GS_OK
        L = _abi.load()
        cfg = _abi.GsConfig()
        cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(_abi.GsConfig), 64, 64, 16, _abi.GS_FLAG_SPLAT_STATE
        ctx, info, nn, m = ctypes.c_void_p(), _abi.GsThinInfo(), ctypes.c_uint64(9), ctypes.c_uint64(9)
        _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
        _abi.check(L.gs_upload_splats(ctx, None, 0))
        for radius in (0.0, 0.05, 1e3):
            for order, seed in ORDERS.values():
                q = thin._query(radius, (0, 0), None, False, order, seed, 0, 0)
                info.members = info.rounds = 9
                _abi.check(L.gs_thin_sample(ctx, ctypes.byref(q), ctypes.byref(info)))
                assert (info.members, info.kept, info.dropped, info.largest, info.candidates, info.rounds) == (0, 0, 0, 0, 0, 0)
        _abi.check(L.gs_thin_read(ctx, None, None, 0, ctypes.byref(nn)))
        _abi.check(L.gs_state_thin(ctx, 1, NONE, 1, 0, 0, 1, 2, ctypes.byref(m)))
        assert nn.value == 0 and m.value == 0
        L.gs_destroy(ctx)
        return
    pos = np.ascontiguousarray(ragged()[:n, 0:3]) * F(0.1)
    r = _mk(records(pos), 64, 64, 16)
    for radius in (0.0, 0.05, 1e3):
        for order, seed in ORDERS.values():
            check_sample(r, "tiny%d" % n, pos, radius, order=order, seed=seed)
    assert thin.select_kept(r) == 1 and thin.select_dropped(r) == n - 1  # radius 1e3: one survivor
    r.destroy()


@pytest.mark.gpu
def test_chain_and_round_cap():
    """A line of 4096 points at spacing 0.25, radius 0.25, index order: point k waits for point k - 1, so it takes 4096 rounds and the
    default cap refuses it; the result is the restatement's (alternating).  max_rounds = rounds - 1: GS_ERR_CAPACITY with the rounds
    and the undecided members in the message, and the planes of the previous sample bit for bit.  The hash order needs a few rounds."""
    from gsplat import _abi, thin
    p = chain_pos()
    r = _mk(records(p), 64, 64, 16)
    info = check_sample(r, "chain", p, 0.25, order="hash")
    assert 2 <= info["rounds"] <= 24, info
    hk, hc = thin.read(r)
    code, msg = code_of(lambda: thin.sample(r, 0.25, order="index"))  # the default cap
    assert code == _abi.GS_ERR_CAPACITY and "gs_thin_sample" in msg and "after %d rounds" % _abi.GS_THIN_DEFAULT_ROUNDS in msg, msg
    k, c = thin.read(r)
    assert np.array_equal(k, hk) and np.array_equal(c, hc)
    info = check_sample(r, "chain", p, 0.25, order="index", max_rounds=1 << 20)
    k, c = thin.read(r)
    even = np.arange(4096) % 2 == 0
    assert np.array_equal(k == np.arange(4096), even) and np.array_equal(k[~even], np.arange(4096)[~even] - 1)
    assert (c[even] == 2).all() and not c[~even].any()  # an odd point's keeper is the lower of its two kept neighbours
    rounds = info["rounds"]
    assert rounds >= 2 and rounds == 4096, info  # (a round reads the decisions of earlier rounds only: the count is the inputs')
    check_sample(r, "chain", p, 0.25, order="hash", seed=12345)
    hk, hc = thin.read(r)
    code, msg = code_of(lambda: thin.sample(r, 0.25, order="index", max_rounds=rounds - 1))
    assert code == _abi.GS_ERR_CAPACITY and "after %d rounds" % (rounds - 1) in msg and re.search(r"\b1 members are still undecided", msg), msg
    k, c = thin.read(r)
    assert np.array_equal(k, hk) and np.array_equal(c, hc)  # left as they were
    assert thin.sample(r, 0.25, order="index", max_rounds=rounds)["rounds"] == rounds
    assert thin.sample(r, BELOW, order="index")["kept"] == 4096
    r.destroy()


@pytest.mark.gpu
def test_determinism_and_placement():
    """Two samples agree; a slab context, a borrower and a PipelinedRenderer give a fresh whole-canvas context's planes."""
    import gsplat
    from gsplat import _abi, thin
    rec = ragged()
    pos = np.ascontiguousarray(rec[:, 0:3])
    wk, wc = want("ragged", pos, 0.5)
    owner = _mk(rec, 64, 64, 16)
    infos = []
    for _ in range(2):
        infos.append(thin.sample(owner, 0.5))
        k, c = thin.read(owner)
        assert np.array_equal(k, wk) and np.array_equal(c, wc)
    assert infos[0] == infos[1]
    slab = _mk(rec, 256, 256, 16, cols=SLAB_COLS[16])
    assert check_sample(slab, "ragged", pos, 0.5) == infos[0]
    slab.destroy()
    borrower = _mk(rec, 64, 64, 16, share_with=owner)
    k, c = thin.read(borrower)
    assert (k == NONE).all() and not c.any()  # the borrower keeps its own planes
    check_sample(borrower, "ragged", pos, 0.3, order="index", max_rounds=4096)
    k, c = thin.read(owner)
    assert np.array_equal(k, wk) and np.array_equal(c, wc)
    borrower.destroy()
    owner.destroy()
    p = gsplat.PipelinedRenderer(gsplat.Canvas(64, 64), None, 0, gsplat.PackedGaussians(rec), 16, frames_in_flight=2, flags=_abi.GS_FLAG_SPLAT_STATE)
    p.render_uniforms(state_scene("ragged")[1])  # in flight when the call comes
    assert check_sample(p, "ragged", pos, 0.5) == infos[0]
    assert thin.select_kept(p) == infos[0]["kept"]
    ids = thin.spread(p, 0.5)
    assert np.array_equal(ids, np.flatnonzero(wk == np.arange(wk.size)))
    p.destroy()


@pytest.mark.gpu
def test_state_thin():
    """matched and the plane against state_restate for every op, inside 0 and 1, where filters and the empty range; kept and dropped
    partition the members."""
    from gsplat import thin
    rec = ragged()
    n = rec.shape[0]
    pos = np.ascontiguousarray(rec[:, 0:3])
    st = np.random.default_rng(7).integers(0, 256, n).astype(np.uint8)
    mem = (st & 0x40) == 0
    wk, wc = want("ragged", pos, 0.5, members=mem, mkey="bit6")
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    thin.sample(r, 0.5, where=(0x40, 0))
    ranges = [(0, 0), (1, 1), (1, NONE), (2, 9), (10, NONE), (0, NONE), (4, 1), (int(wc.max()), int(wc.max()))]
    for k, (lo, hi) in enumerate(ranges):
        for inside in (True, False):
            for op in OPS:
                bits = (0x02, 0xA4)[(k + op) % 2]
                where = ((0, 0), (0x0C, 0x04), (0x30, 0x10))[(k + op + int(inside)) % 3]
                r.write_state(st)
                member = tr.member(wc, lo, hi, inside)
                new, matched = sr.apply_region(st, member, op, bits, where)
                cell = (lo, hi, inside, op, bits, where)
                assert thin.select(r, lo, hi, inside, where, op, bits) == matched, cell
                np.testing.assert_array_equal(r.read_state(), new, err_msg=str(cell))
    r.write_state(st)
    kept = thin.select_kept(r, where=(0x40, 0), op=sr.SET, bits=0x80)  # (bit 7: no where filter here reads it)
    dropped = thin.select_dropped(r, where=(0x40, 0), op=sr.CLEAR, bits=0x80)
    assert kept == int((wk == np.arange(n)).sum()) and dropped == int(mem.sum()) - kept and kept + dropped == int(mem.sum())
    np.testing.assert_array_equal(r.read_state(), np.where(mem, np.where(wk == np.arange(n), st | 0x80, st & 0x7F), st).astype(np.uint8))
    assert thin.select_dropped(r, op=sr.CLEAR, bits=0x80) == n - kept  # without the member filter a non-member's 0 takes part
    k, c = thin.read(r)
    assert np.array_equal(k, wk) and np.array_equal(c, wc)  # the selection only reads the planes
    r.destroy()


@pytest.mark.gpu
def test_decimate():
    """decimate on a state scene: the id map is the kept members and the non-members in order, the states are carried, and an EXACT
    frame afterwards is a fresh context's of those records bit for bit; dedupe keeps the lower index; the tag is refused when taken."""
    from gsplat import _abi, attributes, thin
    s, u, W, H = state_scene("ragged")
    n = s.shape[0]
    pos = np.ascontiguousarray(s[:, 0:3])
    st = (np.arange(n) % 4 == 1).astype(np.uint8) * 4  # bit 2: no member
    mem = st == 0
    r = _mk(s, W, H, 8, exact=True)
    r.write_state(st)
    logit = attributes.attr(_abi.GS_ATTR_OPACITY_LOGIT)
    lv = attributes.values(r, logit)
    wk, wc = want("ragged", pos, 0.3, members=mem, mkey="mod4", priority=lv, pkey="logit")
    info, ids = thin.decimate(r, 0.3, where=(4, 0), priority=logit)
    stay = ~mem | (wk == np.arange(n))
    assert np.array_equal(ids, np.flatnonzero(stay)) and r.numGaussians == int(stay.sum()) == n - info["dropped"]
    assert (info["members"], info["kept"], info["dropped"], info["largest"]) == tr.info_counts(wk, wc) and info["dropped"] > 500
    np.testing.assert_array_equal(r.read_state(), st[stay])  # no tag left
    np.testing.assert_array_equal(r.export_splats()[:, :59], s[stay][:, :59])
    k, c = thin.read(r)
    assert (k == NONE).all() and not c.any()  # a compaction drops the planes
    fresh = _mk(np.ascontiguousarray(s[stay]), W, H, 8, exact=True)
    fresh.write_state(st[stay])
    ta, tb = frame_taps(r, u, False), frame_taps(fresh, u, False)
    for name in ta:
        np.testing.assert_array_equal(ta[name], tb[name], err_msg=name)
    fresh.destroy()
    # no link left among the members: a second decimation at the radius drops nothing and returns the identity
    info2, ids2 = thin.decimate(r, 0.3, where=(4, 0), priority=logit)
    assert info2["dropped"] == 0 and np.array_equal(ids2, np.arange(r.numGaussians))
    r.write_state(np.full(r.numGaussians, 0x80, np.uint8))
    with pytest.raises(ValueError):
        thin.decimate(r, 0.3)
    r.destroy()
    # dedupe: the resident, lower-index copy survives
    two = np.concatenate([s[:500], s[:500]])
    two[700, 0:3] += F(1e-3)
    r = _mk(two, W, H, 8)
    info, ids = thin.dedupe(r, 0.0)
    assert info["dropped"] == 499 and np.array_equal(ids, np.r_[np.arange(500), 700])
    r.destroy()


@pytest.mark.gpu
def test_decimate_to():
    """decimate_to stays within its rule: at most 24 probes, the kept count does not exceed the target and is the nearest to it among
    the radii probed (here: within a few percent), the splats left are the non-members plus the kept."""
    from gsplat import thin
    rec = ragged()
    n = rec.shape[0]
    for target in (1500, 300):
        r = _mk(rec, 64, 64, 16)
        out = thin.decimate_to(r, target)
        print(target, {k: v for k, v in out.items() if k != "ids"})
        assert out["probes"] <= 24 and out["kept"] <= target and out["kept"] >= int(0.9 * target), out["kept"]
        assert out["splats"] == r.numGaussians == out["kept"] == out["ids"].size and out["info"]["members"] == n
        wk, _ = tr.sample(rec[:, 0:3], out["radius"])
        assert np.array_equal(out["ids"], np.flatnonzero(wk == np.arange(n)))
        r.destroy()
    r = _mk(rec, 64, 64, 16)
    out = thin.decimate_to(r, 0)  # one finite member is always kept: no probe reaches 0
    assert out["ids"] is None and out["radius"] is None and r.numGaussians == n and out["probes"] <= 24
    out = thin.decimate_to(r, n)  # radius 0 already fits: one probe, only exact duplicates could go
    assert out["probes"] == 1 and out["radius"] == 0.0 and r.numGaussians == out["kept"] == int((tr.sample(rec[:, 0:3], 0.0)[0] == np.arange(n)).sum())
    r.destroy()


@pytest.mark.gpu
def test_lifecycle():
    """NONE / 0 before any sample and after upload, compact and share_splats; state calls, a transform, a frame, a count and a
    labelling leave the planes."""
    from gsplat import _abi, clusters, neighbours, thin
    s, u, W, H = state_scene("ragged")
    n = s.shape[0]
    wk, wc = want("ragged", np.ascontiguousarray(s[:, 0:3]), 0.5)

    def initial(r, m):
        k, c = thin.read(r)
        return k.shape == c.shape == (m,) and bool((k == NONE).all()) and not c.any()

    def sampled(r):
        k, c = thin.read(r)
        return np.array_equal(k, wk) and np.array_equal(c, wc)

    r = _mk(s, W, H, 8)
    other = _mk(np.ascontiguousarray(s[:1500]), W, H, 8)
    assert initial(r, n)
    thin.sample(r, 0.5)
    assert sampled(r)
    assert r.select_sphere((0, 0, 0), 1.5) > 100
    r.translate_selected((0.3, -0.2, 0.1))
    r.hide_selected()
    r.render_uniforms(u)
    r.wait()
    r.accumulate_coverage()
    neighbours.count(r, 0.3)
    clusters.label(r, 0.3)
    assert sampled(r)  # they describe the positions and states at the time of the sample
    st = (np.arange(n) % 3 == 0).astype(np.uint8) * 4
    r.write_state(st)
    kept = r.compact(4, 4)
    assert initial(r, kept.size)
    moved = r.export_splats()
    info = thin.sample(r, 0.5, order="index", max_rounds=4096)
    mk_, mc = tr.sample(moved[:, 0:3], 0.5, flags=tr.ORDER_INDEX)
    k, c = thin.read(r)
    assert np.array_equal(k, mk_) and np.array_equal(c, mc) and info["kept"] == int((mk_ == np.arange(kept.size)).sum())
    arr = np.ascontiguousarray(s[:2000])
    _abi.check(r._L.gs_upload_splats(r._ctx, arr.ctypes.data, 2000))
    assert initial(r, 2000)
    thin.sample(r, 0.5)
    assert not initial(r, 2000)
    _abi.check(r._L.gs_share_splats(r._ctx, other._ctx))
    assert initial(r, 1500)
    r.destroy()
    other.destroy()


@pytest.mark.gpu
def test_sample_disturbs_no_frame():
    """A frame rendered before and after a sample and a selection that changes nothing is byte-identical in every tap, and the
    statistics are unchanged."""
    from gsplat import thin
    s, u, W, H = state_scene("ragged")
    a, b = _mk(s, W, H, 8), _mk(s, W, H, 8)
    wk, wc = want("ragged", np.ascontiguousarray(s[:, 0:3]), 0.5)
    before = frame_taps(a, u, False)
    frame_taps(b, u, False)
    for _ in range(3):  # three frames in flight on both; no wait: the sample drains the ring
        a.render_uniforms(u)
        b.render_uniforms(u)
    thin.sample(a, 0.5)
    k, c = thin.read(a)
    assert np.array_equal(k, wk) and np.array_equal(c, wc)
    assert thin.select(a, 5, 1, op=sr.SET, bits=sr.HIDDEN) == 0  # the empty range
    ta, tb = frame_taps(a, u, False), frame_taps(b, u, False)
    for name in ta:
        np.testing.assert_array_equal(ta[name], tb[name], err_msg=name)
        np.testing.assert_array_equal(ta[name], before[name], err_msg=name)
    assert timeless(a.stats()) == timeless(b.stats())
    a.destroy()
    b.destroy()


@pytest.mark.gpu
def test_budget_and_refusals():
    """max_candidates = 1 at radius 1e3 is refused with GS_ERR_CAPACITY, both numbers in the message, info written and the planes as
    they were; every refused argument names its number and leaves planes and states as they were; a context without the state plane
    takes (0, 0) only."""
    from gsplat import _abi, attributes, thin
    L = _abi.load()
    INV = _abi.GS_ERR_INVALID_ARGUMENT
    rec = ragged()
    n = rec.shape[0]
    pos = np.ascontiguousarray(rec[:, 0:3])
    wk, wc = want("ragged", pos, 0.5)
    info, nn, m = _abi.GsThinInfo(), ctypes.c_uint64(), ctypes.c_uint64(77)

    def query(**kw):
        q = thin._query(kw.pop("radius", 0.5), (kw.pop("mask", 0), kw.pop("value", 0)), kw.pop("priority", None), False, "hash", 0, 0, 0)
        for name, v in kw.items():
            setattr(q, name, v)
        return q

    # before any upload: GS_ERR_NO_SCENE; N == 0: zero results, GS_OK
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(_abi.GsConfig), 64, 64, 16, _abi.GS_FLAG_SPLAT_STATE
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    q = query()
    assert L.gs_thin_sample(ctx, ctypes.byref(q), ctypes.byref(info)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_thin_read(ctx, None, None, 0, ctypes.byref(nn)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_state_thin(ctx, 0, 1, 1, 0, 0, 1, 2, None) == _abi.GS_ERR_NO_SCENE
    _abi.check(L.gs_upload_splats(ctx, None, 0))
    info.members = info.candidates = 9
    _abi.check(L.gs_thin_sample(ctx, ctypes.byref(q), ctypes.byref(info)))
    assert (info.members, info.kept, info.dropped, info.largest, info.candidates, info.rounds) == (0, 0, 0, 0, 0, 0)
    _abi.check(L.gs_thin_sample(ctx, ctypes.byref(q), None))
    nn.value = 9
    _abi.check(L.gs_thin_read(ctx, None, None, 0, ctypes.byref(nn)))
    assert nn.value == 0
    _abi.check(L.gs_state_thin(ctx, 0, 1, 1, 0, 0, 1, 2, ctypes.byref(m)))
    assert m.value == 0
    L.gs_destroy(ctx)

    r = _mk(rec, 64, 64, 16)
    st = (np.arange(n) % 5).astype(np.uint8)
    r.write_state(st)
    thin.sample(r, 0.5)
    # the budget: info written, planes as they were
    q = query(radius=1e3, max_candidates=1)
    assert L.gs_thin_sample(r._ctx, ctypes.byref(q), ctypes.byref(info)) == _abi.GS_ERR_CAPACITY
    msg = L.gs_last_error().decode()
    assert info.candidates == 3001 * 3001 and info.members == 3001 and tuple(info.cells) == (1, 1, 1) and info.cell_edge >= 1001.0
    assert "gs_thin_sample" in msg and str(3001 * 3001) in msg and "max_candidates = 1 " in msg + " ", msg
    k, c = thin.read(r)
    assert np.array_equal(k, wk) and np.array_equal(c, wc)
    code, msg = code_of(lambda: thin.sample(r, 1e3, max_candidates=3001 * 3001 - 1))
    assert code == _abi.GS_ERR_CAPACITY and str(3001 * 3001) in msg and str(3001 * 3001 - 1) in msg
    assert thin.sample(r, 1e3, max_candidates=3001 * 3001)["kept"] == 1
    thin.sample(r, 0.5)

    def refused(name, call, *fragments, code=INV):
        assert call() == code, name
        msg = L.gs_last_error().decode()
        assert name + ":" in msg and all(f in msg for f in fragments), msg
        k, c = thin.read(r)
        assert np.array_equal(k, wk) and np.array_equal(c, wc)
        np.testing.assert_array_equal(r.read_state(), st)

    run = lambda q: (lambda: L.gs_thin_sample(r._ctx, ctypes.byref(q) if q is not None else None, ctypes.byref(info)))
    refused("gs_thin_sample", run(None), "null query")
    refused("gs_thin_sample", run(query(struct_size=40)), "struct_size 40")
    refused("gs_thin_sample", run(query(radius=float("nan"))), "radius nan")
    refused("gs_thin_sample", run(query(radius=float("inf"))), "radius inf")
    refused("gs_thin_sample", run(query(radius=-0.5)), "radius -0.5")
    refused("gs_thin_sample", run(query(radius=2e19)), "radius 2e+19", "squared")
    refused("gs_thin_sample", run(query(flags=4)), "unknown flags 0x4")
    refused("gs_thin_sample", run(query(flags=0x80000001)), "unknown flags 0x80000000")
    refused("gs_thin_sample", run(query(flags=_abi.GS_THIN_ASCENDING)), "GS_THIN_ASCENDING without a priority")
    refused("gs_thin_sample", run(query(reserved0=5)), "reserved0 = 5")
    refused("gs_thin_sample", run(query(reserved=(ctypes.c_uint32 * 2)(5, 0))), "reserved[0] = 5")
    refused("gs_thin_sample", run(query(reserved=(ctypes.c_uint32 * 2)(0, 6))), "reserved[1] = 6")
    refused("gs_thin_sample", run(query(mask=0x100)), "0x100", "does not fit the state byte")
    refused("gs_thin_sample", run(query(value=0x1FF)), "0x1ff", "does not fit the state byte")
    refused("gs_thin_sample", run(query(priority=attributes.attr(_abi.GS_ATTR_COUNT))), "unknown attribute kind 16")
    bad = attributes.attr(_abi.GS_ATTR_OPACITY_LOGIT)
    bad.struct_size = 20
    refused("gs_thin_sample", run(query(priority=bad)), "struct_size 20")
    refused("gs_thin_sample", run(query(priority=attributes.attr(_abi.GS_ATTR_DIST2, (np.nan, 0, 0)))), "gs_thin_sample")
    # the read's conventions are gs_cluster_read's
    refused("gs_thin_read", lambda: L.gs_thin_read(r._ctx, None, None, 0, None), "null n")
    a, b = np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, 0xA5A5A5A5, np.uint32)
    refused("gs_thin_read", lambda: L.gs_thin_read(r._ctx, a.ctypes.data, b.ctypes.data, n - 1, ctypes.byref(nn)), "%d words per plane needed" % n)
    assert nn.value == n and (a == 0xA5A5A5A5).all() and (b == 0xA5A5A5A5).all()
    _abi.check(L.gs_thin_read(r._ctx, a.ctypes.data, None, n, ctypes.byref(nn)))  # either plane alone
    assert np.array_equal(a, wk) and (b == 0xA5A5A5A5).all()
    _abi.check(L.gs_thin_read(r._ctx, None, b.ctypes.data, n, ctypes.byref(nn)))
    assert np.array_equal(b, wc)
    # the state call's own: nothing is applied
    sel = lambda op, bits, wm=0: (lambda: L.gs_state_thin(r._ctx, 0, 5, 1, wm, 0, op, bits, ctypes.byref(m)))
    m.value = 77
    refused("gs_state_thin", sel(0, 2), "unknown op 0")
    refused("gs_state_thin", sel(5, 2), "unknown op 5")
    refused("gs_state_thin", sel(1, 0x100), "0x100")
    refused("gs_state_thin", sel(1, 2, 0x100), "where_mask 0x100")
    assert m.value == 77
    r.destroy()
    # a context without the state plane: (0, 0) works, any other filter and the state call are refused
    q = mk(rec, 64, 64, 16)
    check_sample(q, "ragged", pos, 0.5)
    for fn in (lambda: thin.sample(q, 0.5, where=(1, 0)), lambda: thin.select(q, 0, 1), lambda: thin.decimate(q, 0.5)):
        code, msg = code_of(fn)
        assert code == INV and "GS_FLAG_SPLAT_STATE" in msg
    ids = thin.spread(q, 0.5)  # without the plane the list comes from the planes
    assert np.array_equal(ids, np.flatnonzero(wk == np.arange(n)))
    k, c = thin.read(q)
    assert np.array_equal(k, wk) and np.array_equal(c, wc)
    q.destroy()
