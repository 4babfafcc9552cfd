"""Cell merge and gsplat.simplify (gs_abi.h "cell merge"): the symbols, layouts and refusals; gs_cell_merge_host against the numpy
restatement bit for bit (group_of, counts, every sum) and against its independent f64 finishing model by a margin; the invariants of the
definition; and on the GPU the device entry points against both, on whole, slab and borrowing contexts, and the simplify verbs.

THE MARGIN of the finishing.  The yardstick is the f64 model's own record rounded to f32; the library's largest relative Frobenius
error of R(q) diag(exp(2 s)) R(q)^T against the model's covariance, and its largest relative error of sigmoid(logit) against the
model's alpha, may each be at most 4 x the yardstick's (Jacobi against LAPACK and libraries that differ in the last place of log and
sqrt must not fail; a wrong formula misses by orders of magnitude).  Every comparison prints both maxima; profiles/simplify.txt
records them.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import export_restate as er
import merge_restate as ms
from support import F, ROOT, SLAB_COLS, TAPS, c_layout, cached, code_of, frame_taps, guarded, is_fill, mk, raw_export, special_records, state_scene

_mk = functools.partial(mk, state=True)
CSRC = os.path.join(ROOT, "gaussian-splatting-wgpu_amd", "csrc")
H = 0.25                                          # the planted scenes' cell edge: a power of two, so a face is hit exactly
RUNS = (1, 2, 3, 63, 64, 65, 127, 129, 257)       # the lane, wave and prefetch boundaries of the member loop
SIZES = (1, 2, 3, 5, 63, 64, 65, 1023, 1025, 3001)
TINY = 1e-6                                       # an edge that the 1024-cell clamp raises
TAG = 0x80
HALF, NOBODY, ONE = (0x04, 0x04), (TAG, TAG), (0x40, 0x40)
FILTERS = {"all": (0, 0), "half": HALF, "nobody": NOBODY, "one": ONE}


def scene_of(n):
    """(records float32[n, 80], state uint8[n]) of support.special_records(n).  From 1023 splats on the positions are planted: an
    anchor at the origin, runs of RUNS members in every other cell of the row y = z = 0 with their ids interleaved, members on and
    next to a cell face, three and two exact copies of one position, everyone else in cells no planted splat uses (a coordinate
    that was not finite stays so).  Bit 7 is clear everywhere, bit 6 set on one splat, bit 2 on about half."""
    def make():
        rec = np.array(special_records(n), F, copy=True)
        rng = np.random.default_rng(1000 + n)
        st = (rng.integers(0, 64, n, dtype=np.uint8)).astype(np.uint8)
        st[n // 2] |= 0x40
        if n < 1023:
            return np.ascontiguousarray(rec), st
        h = F(H)
        pos = np.stack([rng.uniform(0, 64, n), rng.uniform(2, 10, n), rng.uniform(0, 8, n)], 1).astype(F) * h
        rows = 100 + rng.permutation(sum(RUNS))
        at = 0
        for j, length in enumerate(RUNS):
            i = rows[at:at + length]
            at += length
            u = rng.uniform(0.1, 0.9, (length, 3)).astype(F)
            pos[i] = (u + np.array([2 * j + 2, 0, 0], F)) * h
        pos[99] = 0.0
        face = F(40.0) * h
        pos[820:823] = [[face, 1.5 * H, 0.5 * H], [np.nextafter(face, F(0)), 1.5 * H, 0.5 * H], [face + F(0.5) * h, 1.5 * H, 0.5 * H]]
        pos[830:833] = [60.3 * H, 1.5 * H, 0.5 * H]
        pos[833:835] = [62.3 * H, 1.5 * H, 0.5 * H]
        keep = np.ones(n, bool)
        keep[99:835] = False
        old = rec[:, 0:3].copy()
        rec[:, 0:3] = np.where(np.isfinite(old) | ~keep[:, None], pos, old)
        rec[830:833, 3:] = rec[830, 3:]   # exact copies of one splat
        rec[833:835, 3:] = rec[833, 3:]
        return np.ascontiguousarray(rec), st
    return cached(("simplify_scene", n), make)


def edges_of(n):
    return (H if n >= 1023 else 0.5, TINY)


def want(n, cell, filt="all", min_members=2):
    """The restatement of one merge, its finishing model and the yardstick's margins, once per session."""
    def make():
        rec, st = scene_of(n)
        w = ms.merge(rec, st, cell, *FILTERS[filt], min_members=min_members)
        w["model"] = ms.model(w["sums"])
        w["yard"] = tuple(float(e.max()) if e.size else 0.0 for e in ms.finish_errors(w["model"]["rec"], w["model"]))
        return w
    return cached(("simplify_want", n, cell, filt, min_members), make)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=what)


def held_to_model(rec, w, what):
    """The finishing of `rec` against the model of the restated sums: the margin, position and SH within one f32 step, zero padding."""
    if not len(rec):
        return (0.0, 0.0)
    cov, opa = ms.finish_errors(rec, w["model"])
    got = (float(cov.max()), float(opa.max()))
    print("%s: covariance %.3e (yardstick %.3e), opacity %.3e (yardstick %.3e)" % (what, got[0], w["yard"][0], got[1], w["yard"][1]))
    assert got[0] <= 4.0 * w["yard"][0] and got[1] <= 4.0 * w["yard"][1], what
    yard = w["model"]["rec"]
    assert ms.ulps(rec[:, 0:3], yard[:, 0:3]).max() <= 1 and ms.ulps(rec[:, ms.SH_COLS], yard[:, ms.SH_COLS]).max() <= 1, what
    assert not rec[:, ms.PAD_COLS].view(np.uint32).any(), what
    q = rec[:, 8:12].astype(np.float64)
    assert (rec[:, 8] >= 0).all() and np.abs(np.linalg.norm(q, axis=1) - 1.0).max() < 1e-6, what
    assert (rec[:, 4] >= rec[:, 5]).all() and (rec[:, 5] >= rec[:, 6]).all(), what
    return got


def pinned(info, extra, w, what):
    assert info == w["info"], what
    same_bits(extra["group_of"], w["group_of"], what + " group_of")
    same_bits(extra["sums"].reshape(-1, 64), w["sums"].reshape(-1, 64), what + " sums")


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_merge_abi(tmp_path):
    """The three symbols are exported without a GPU and listed; the version is still 3; the struct layouts in the compiled header are
    the ctypes mirrors'; the refusals name the call and write nothing; the renderer classes gained no method."""
    from gsplat import _abi, renderer, simplify
    L = _abi.load()
    for name in ("gs_cell_merge", "gs_cell_merge_device", "gs_cell_merge_host"):
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    assert L.gs_abi_version() == 3
    got = c_layout(tmp_path, "merge_layout",
                   'printf("%u %u %u %u %u %u ", (unsigned)GS_ABI_VERSION, (unsigned)sizeof(gs_merge), (unsigned)offsetof(gs_merge, cell),'
                   '(unsigned)offsetof(gs_merge, min_members), (unsigned)offsetof(gs_merge, op), (unsigned)offsetof(gs_merge, bits));'
                   'printf("%u %u %u %u %u ", (unsigned)sizeof(gs_merge_info), (unsigned)offsetof(gs_merge_info, members),'
                   '(unsigned)offsetof(gs_merge_info, largest), (unsigned)offsetof(gs_merge_info, cells), (unsigned)offsetof(gs_merge_info, cell_edge));'
                   'printf("%u %u %u", (unsigned)GS_MERGE_SUM_DOUBLES, (unsigned)(GS_MERGE_NONE == 0xFFFFFFFFu), (unsigned)GS_MERGE_DEFAULT_MAX_MEMBERS);')
    M, I = _abi.GsMerge, _abi.GsMergeInfo
    assert got == [3, ctypes.sizeof(M), M.cell.offset, M.min_members.offset, M.op.offset, M.bits.offset, ctypes.sizeof(I), I.members.offset,
                   I.largest.offset, I.cells.offset, I.cell_edge.offset, _abi.GS_MERGE_SUM_DOUBLES, 1, _abi.GS_MERGE_DEFAULT_MAX_MEMBERS]
    assert got[1] == 32 and got[6] == 48
    rec, st = scene_of(65)
    out, sums, gof, info = guarded((66, 80), F), guarded((66, 64), np.float64), guarded(65, np.uint32), guarded(48, np.uint8)
    INV = _abi.GS_ERR_INVALID_ARGUMENT

    def call(fn, lead, p, records=out.ctypes.data, cap=66):
        return fn(*lead, ctypes.byref(p), records, cap, sums.ctypes.data, gof.ctypes.data, ctypes.cast(info.ctypes.data, ctypes.POINTER(I)))
    good = dict(cell=0.5, mask=0, value=0, min_members=2, max_members=0, op=0, bits=0)
    host = (rec.ctypes.data, st.ctypes.data, 65)
    for change, fragment in ((dict(struct_size=28), "struct_size"), (dict(cell=0.0), "cell"), (dict(cell=-1.0), "cell"),
                             (dict(cell=float("nan")), "cell"), (dict(cell=float("inf")), "cell"), (dict(min_members=1), "min_members"),
                             (dict(min_members=0), "min_members"), (dict(op=5), "op"), (dict(op=1, bits=0x100), "bits"),
                             (dict(op=0, bits=4), "bits without an op"), (dict(mask=0x100), "state byte"), (dict(value=0x1FF), "state byte")):
        p = simplify._params(**{k: v for k, v in dict(good, **change).items() if k != "struct_size"})
        p.struct_size = change.get("struct_size", p.struct_size)
        for fn, lead, name in ((L.gs_cell_merge_host, host, "gs_cell_merge_host"), (L.gs_cell_merge, (None,), "gs_cell_merge"),
                               (L.gs_cell_merge_device, (None,), "gs_cell_merge_device")):
            assert call(fn, lead, p) == INV, (name, change)  # (the parameters are refused before the context is looked at)
            msg = L.gs_last_error().decode()
            assert name in msg and fragment in msg, msg
    p = simplify._params(**good)
    for fn, name in ((L.gs_cell_merge, "gs_cell_merge"), (L.gs_cell_merge_device, "gs_cell_merge_device")):
        assert call(fn, (None,), p) == INV and name in L.gs_last_error().decode() and "null ctx" in L.gs_last_error().decode()
    assert call(L.gs_cell_merge_host, (None, None, 65), p) == INV and "null records" in L.gs_last_error().decode()
    assert call(L.gs_cell_merge_host, host, p, records=None, cap=3) == INV and "null records with cap_records 3" in L.gs_last_error().decode()
    for change in (dict(mask=4, value=4), dict(op=1, bits=TAG)):
        p2 = simplify._params(**dict(good, **change))
        assert call(L.gs_cell_merge_host, (rec.ctypes.data, None, 65), p2) == INV and "null state" in L.gs_last_error().decode()
    assert is_fill(out) and is_fill(sums) and is_fill(gof) and is_fill(info)
    # n == 0: zeros, GS_OK
    assert call(L.gs_cell_merge_host, (None, None, 0), p) == 0 and not info.any() and is_fill(out) and is_fill(sums)
    import test_abi
    for cname in ("Renderer", "PipelinedRenderer"):
        live = {n for n in vars(getattr(renderer, cname)) if not n.startswith("_") and callable(getattr(getattr(renderer, cname), n))}
        assert live == set(test_abi.PYTHON_HOST_SURFACE[cname]) - {"__init__"}
    import gsplat
    assert gsplat.simplify is simplify
    for fn in ("merge_cells", "count", "host_merge", "simplify", "simplify_to"):
        assert callable(getattr(simplify, fn))


def test_planted_scene_holds_the_boundary_runs():
    """A SELF-CHECK OF THE FIXTURE, not of the library (it runs the numpy restatement alone and passes without the feature): the
    planted scenes hold runs of exactly the lengths of RUNS, the face members on their own sides, and the copies together; the tiny
    edge is raised by the clamp to at most 1024 cells -- what the tests below rely on when they say they cover those cases."""
    for n in (1023, 1025, 3001):
        rec, st = scene_of(n)
        w = want(n, H, "all", 1)  # min_members 1: every run
        lens = set(w["lens"].tolist())
        assert set(RUNS) <= lens, sorted(lens)
        g = w["group_of"]
        assert g[820] == g[822] != g[821] and g[830] == g[831] == g[832] != g[833] == g[834]
        assert w["info"]["cell_edge"] == H and w["info"]["eligible"] < n  # (the special floats make some splats ineligible)
        t = want(n, TINY)
        assert max(t["info"]["cells"]) == 1024 and t["info"]["cell_edge"] > TINY and t["info"]["groups"] >= 2
        one = want(n, H, "one")
        assert one["info"]["eligible"] == 1 and one["info"]["groups"] == 0
        assert want(n, H, "nobody")["info"] == {"eligible": 0, "groups": 0, "members": 0, "largest": 0, "cells": (0, 0, 0), "cell_edge": 0.0}


@pytest.mark.parametrize("filt", ["all", "half", "nobody", "one"])
@pytest.mark.parametrize("n", SIZES)
def test_host_twin_is_the_restatement(n, filt):
    """gs_cell_merge_host: group_of, the counts and every sum bit for bit; the records against the model by the margin; op marks
    exactly the members, in place, and nothing else changes."""
    from gsplat import _abi, simplify
    rec, st = scene_of(n)
    for cell in edges_of(n) + (1.0e4,):  # (the last: everything in one cell)
        w = want(n, cell, filt)
        what = "host n=%d cell=%g %s" % (n, cell, filt)
        state = st.copy()
        before = rec.copy()
        got, info, extra = simplify.host_merge(rec, state, cell, *FILTERS[filt], op=_abi.GS_STATE_SET, bits=TAG)
        pinned(info, extra, w, what)
        held_to_model(got, w, what)
        same_bits(state, ms.marked(st, w["members"], 1, TAG), what + " state")
        same_bits(rec, before, what + " records untouched")
        assert simplify.host_merge(rec, st.copy(), cell, *FILTERS[filt], count_only=True)[1] == w["info"]


def test_copies_merge_into_the_splat():
    """k exact copies of a splat (k = 2, 3, 200) merge into that splat with opacity min(0.99, k a), within the margin; its scales come
    back sorted, its orientation as the same covariance."""
    from gsplat import simplify
    base = np.array(scene_of(3001)[0][1500:1503], F, copy=True)
    base[:, 12] = [-3.0, -1.0, 2.0]  # k a below, around and above the cap
    w1, sig = ms.per_splat(base)
    for k in (2, 3, 200):
        for j in range(3):
            rec = np.repeat(base[j:j + 1], k, 0)
            got, info, extra = simplify.host_merge(rec, None, 0.5)
            assert (info["groups"], info["members"], info["largest"]) == (1, k, k)
            w = ms.merge(rec, None, 0.5)
            w["model"] = ms.model(w["sums"])
            w["yard"] = tuple(float(e.max()) for e in ms.finish_errors(w["model"]["rec"], w["model"]))
            pinned(info, extra, w, "copies")
            held_to_model(got, w, "copies k=%d splat %d" % (k, j))
            a = 1.0 / (1.0 + np.exp(-float(base[j, 12])))
            alpha = 1.0 / (1.0 + np.exp(-float(got[0, 12])))
            assert abs(alpha - min(0.99, k * a)) <= 1e-5 * min(0.99, k * a)
            same_bits(got[0, 0:3], base[j, 0:3], "position")
            S = np.array([[sig[j, 0], sig[j, 1], sig[j, 2]], [sig[j, 1], sig[j, 3], sig[j, 4]], [sig[j, 2], sig[j, 4], sig[j, 5]]], np.float64)
            Rm = ms.rotation_of(got[0, 8:12])
            back = Rm @ np.diag(np.exp(2.0 * got[0, 4:7].astype(np.float64))) @ Rm.T
            assert np.linalg.norm(back - S) <= 2e-6 * np.linalg.norm(S)
            assert ms.ulps(got[0, ms.SH_COLS], base[j, ms.SH_COLS]).max() <= 1


def test_ineligible_and_single_splats_are_left_alone():
    """NaN and infinite positions, a NaN logit, logit -200 (a = 0), a +inf log-scale and a zero quaternion are never grouped or
    marked, whatever shares their cell; neither is a cell's only eligible splat."""
    from gsplat import _abi, simplify
    rec = np.repeat(np.array(scene_of(3001)[0][2000:2001], F, copy=True), 12, 0)
    rec[:, 0:3] = [1.0, 2.0, 3.0]
    rec[0, 0], rec[1, 1], rec[2, 2] = np.nan, np.inf, -np.inf
    rec[3, 12], rec[4, 12], rec[5, 5] = np.nan, -200.0, np.inf
    rec[6, 8:12] = 0.0
    rec[11, 0:3] = [50.0, 2.0, 3.0]  # alone in its cell
    for cell in (0.5, 1.0e4):
        st = np.zeros(12, np.uint8)
        got, info, extra = simplify.host_merge(rec, st, cell, op=_abi.GS_STATE_SET, bits=TAG)
        w = ms.merge(rec, st, cell)
        pinned(info, extra, w, "ineligible")
        members = 4 if cell == 0.5 else 5
        assert (info["eligible"], info["groups"], info["members"]) == (5, 1, members)
        assert (extra["group_of"][:7] == ms.NONE).all() and (st[:7] == 0).all() and (st[7:11] == TAG).all() and st[11] == (TAG if members == 5 else 0)


def test_capacity_count_only_and_max_members():
    """Count-only fills info and writes nothing; a capacity of G - 1 writes and marks nothing; max_members = 4 accepts a run of 4
    and refuses a run of 5 before anything is written."""
    from gsplat import _abi, simplify
    rec, st = scene_of(1025)
    w = want(1025, H)
    G = w["info"]["groups"]
    assert G > 3
    L = _abi.load()
    state = st.copy()
    p, info = simplify._params(H, 0, 0, 2, 0, _abi.GS_STATE_SET, TAG), _abi.GsMergeInfo()
    out, sums, gof = guarded((G, 80), F), guarded((G, 64), np.float64), guarded(1025, np.uint32)
    rc = L.gs_cell_merge_host(rec.ctypes.data, state.ctypes.data, 1025, ctypes.byref(p), out.ctypes.data, G - 1, sums.ctypes.data, gof.ctypes.data, ctypes.byref(info))
    msg = L.gs_last_error().decode()
    assert rc == _abi.GS_ERR_INVALID_ARGUMENT and "gs_cell_merge_host" in msg and "%d records needed, the buffer holds %d" % (G, G - 1) in msg
    assert simplify._info(info) == w["info"] and is_fill(out) and is_fill(sums) and is_fill(gof) and (state == st).all()
    rc = L.gs_cell_merge_host(rec.ctypes.data, state.ctypes.data, 1025, ctypes.byref(p), None, 0, sums.ctypes.data, gof.ctypes.data, ctypes.byref(info))
    assert rc == 0 and simplify._info(info) == w["info"] and is_fill(sums) and is_fill(gof) and (state == st).all()
    # runs of 4 and 5
    five = np.repeat(np.array(rec[200:201], F, copy=True), 9, 0)
    five[4:, 0] += 10.0
    four = five[:8]
    got, i4, _ = simplify.host_merge(four, None, 1.0, max_members=4)
    assert (i4["groups"], i4["largest"]) == (2, 4) and len(got) == 2
    p5, info5 = simplify._params(1.0, 0, 0, 2, 4, 0, 0), _abi.GsMergeInfo()
    rc = L.gs_cell_merge_host(five.ctypes.data, None, 9, ctypes.byref(p5), out.ctypes.data, G, sums.ctypes.data, gof.ctypes.data, ctypes.byref(info5))
    msg = L.gs_last_error().decode()
    assert rc == _abi.GS_ERR_CAPACITY and "gs_cell_merge_host" in msg and "max_members = 4" in msg and "cell edge 1" in msg
    assert info5.largest == 5 and is_fill(out) and is_fill(sums) and is_fill(gof)


def test_sanitized_host_program(tmp_path):
    """tools/merge_check: gs_merge_math.h compiled alone with -fsanitize=address,undefined and run as its own process over scenes of its
    own, and over a file of this module's planted scene, whose info, group numbering and sums must be the restatement's.  Skipped where
    the sanitizer runtime is not installed."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed")
    exe = str(tmp_path / "merge_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san +
                          ["-I", CSRC, os.path.join(ROOT, "tools", "merge_check", "main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout == "merge_check ok\n", out.stdout[-2000:] + out.stderr[-2000:]
    rec, st = scene_of(1025)
    path = tmp_path / "scene.bin"
    rec.tofile(path)
    for cell in (H, TINY):
        w = want(1025, cell)
        out = subprocess.run([exe, str(path), repr(float(cell))], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")
        i = w["info"]
        assert lines[0] == "eligible %d groups %d members %d largest %d cells %d %d %d" % ((i["eligible"], i["groups"], i["members"], i["largest"]) + i["cells"])
        sums = np.array([int(x, 16) for x in " ".join(lines[1:1 + i["groups"]]).split()], np.uint64).reshape(-1, 64)
        same_bits(sums, w["sums"].view(np.uint64), "sums of the sanitized program")


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def twin(n, cell, filt):
    """gs_cell_merge_host's records of one merge, once per session."""
    def make():
        from gsplat import simplify
        rec, st = scene_of(n)
        return simplify.host_merge(rec, st.copy(), cell, *FILTERS[filt])[0]
    return cached(("simplify_twin", n, cell, filt), make)


def held_to_twin(got, n, cell, filt, w, what):
    """Device records against the host twin's, directly.  Both are within 4 yardsticks of the model in each measure, so they are
    within 8 of each other (the triangle inequality); position and SH are one f32 rounding of an f64 quotient of the same sums, which
    two division routines can only move by one step."""
    t = twin(n, cell, filt)
    assert t.shape == got.shape, what
    if not len(got):
        return
    cov, opa = ms.record_distance(got, t, w["model"])
    steps = ms.ulps(got[:, ms.CARRIED], t[:, ms.CARRIED]).max()
    print("%s against the host twin: covariance %.3e, opacity %.3e (yardsticks %.3e, %.3e), at most %d f32 steps in any float"
          % (what, cov.max(), opa.max(), w["yard"][0], w["yard"][1], steps))
    assert cov.max() <= 8.0 * w["yard"][0] and opa.max() <= 8.0 * w["yard"][1], what
    assert ms.ulps(got[:, 0:3], t[:, 0:3]).max() <= 1 and ms.ulps(got[:, ms.SH_COLS], t[:, ms.SH_COLS]).max() <= 1, what


def _device_merges(r, n, what, edges=None, filters=("all", "half"), plane=None):
    """Both entry points at every edge and filter against the restatement (bit for bit), its model (the margin) and the host twin's
    records; the device-record call sets TAG on the members and the state plane is compared.  plane: the context through which the
    state plane is seeded and read (a borrower's owner); r itself otherwise."""
    from gsplat import _abi, simplify
    rec, st = scene_of(n)
    plane = plane or r
    for cell in edges or edges_of(n):
        for filt in filters:
            w = want(n, cell, filt)
            for device in (False, True):
                tag = "%s n=%d cell=%g %s %s" % (what, n, cell, filt, "device" if device else "host")
                op = _abi.GS_STATE_SET if device else 0
                plane.write_state(st)
                got, info, extra = simplify.merge_cells(r, cell, *FILTERS[filt], op=op, bits=TAG if op else 0, device=device, sums=True, group_of=True)
                got = got.cpu().numpy() if device else got
                pinned(info, extra, w, tag)
                held_to_model(got, w, tag)
                held_to_twin(got, n, cell, filt, w, tag)
                same_bits(plane.read_state(), ms.marked(st, w["members"], 1, TAG) if op else st, tag + " state")
                assert simplify.count(r, cell, *FILTERS[filt]) == w["info"], tag


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_device_is_the_restatement(n):
    """gs_cell_merge and gs_cell_merge_device on a whole context: sums, group_of, info and the state plane bit for bit at both edges
    (one of them raised by the 1024-cell clamp) with and without a filter; the records within the margin; the scene untouched."""
    rec, st = scene_of(n)
    r = _mk(rec, 64, 64, 16)
    before = raw_export(r, 0, 0, False)[0]
    _device_merges(r, n, "whole", filters=("all", "half", "nobody", "one") if n in (5, 1025) else ("all", "half"))
    same_bits(raw_export(r, 0, 0, False)[0], before, "the scene is not changed")
    if n >= 1023:
        _device_merges(r, n, "one cell", edges=(1.0e4,), filters=("all",))
    r.destroy()


@pytest.mark.gpu
def test_slab_and_borrower():
    """A slab context and a borrower of gs_share_splats answer what the whole context answers; an op given to the borrower marks the
    members in the owner's plane (gs_state_region's rules), which both then read."""
    rec, st = scene_of(1025)
    owner = _mk(rec, 256, 256, 16)
    owner.write_state(st)
    slab = _mk(rec, 256, 256, 16, cols=SLAB_COLS[16])
    _device_merges(slab, 1025, "slab")
    slab.destroy()
    borrower = _mk(rec, 256, 256, 16, share_with=owner)
    _device_merges(borrower, 1025, "borrower", plane=owner)
    same_bits(borrower.read_state(), owner.read_state(), "the borrower reads the owner's plane")
    borrower.destroy()
    owner.destroy()


@pytest.mark.gpu
def test_device_refusals_and_modes():
    """Count-only fills info and marks nothing; a capacity of G - 1 writes and marks nothing; max_members refuses before anything is
    written; an op or a filter on a context without the state plane is refused by name."""
    from gsplat import _abi, simplify
    rec, st = scene_of(1025)
    w = want(1025, H)
    G = w["info"]["groups"]
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    L = r._L
    p, info = simplify._params(H, 0, 0, 2, 0, _abi.GS_STATE_SET, TAG), _abi.GsMergeInfo()
    out, sums, gof = guarded((G, 80), F), guarded((G, 64), np.float64), guarded(1025, np.uint32)
    rc = L.gs_cell_merge(r._ctx, ctypes.byref(p), out.ctypes.data, G - 1, sums.ctypes.data, gof.ctypes.data, ctypes.byref(info))
    assert rc == _abi.GS_ERR_INVALID_ARGUMENT and "gs_cell_merge" in L.gs_last_error().decode() and "%d records needed" % G in L.gs_last_error().decode()
    assert simplify._info(info) == w["info"] and is_fill(out) and is_fill(sums) and is_fill(gof)
    rc = L.gs_cell_merge(r._ctx, ctypes.byref(p), None, 0, sums.ctypes.data, gof.ctypes.data, ctypes.byref(info))
    assert rc == 0 and simplify._info(info) == w["info"] and is_fill(sums) and is_fill(gof)
    p.max_members = 100
    rc = L.gs_cell_merge(r._ctx, ctypes.byref(p), out.ctypes.data, G, sums.ctypes.data, gof.ctypes.data, ctypes.byref(info))
    msg = L.gs_last_error().decode()
    assert rc == _abi.GS_ERR_CAPACITY and "gs_cell_merge" in msg and "max_members = 100" in msg and "cell edge 0.25" in msg
    assert info.largest == 257 and is_fill(out) and is_fill(sums) and is_fill(gof)
    same_bits(r.read_state(), st, "nothing is marked")
    r.destroy()
    plain = mk(rec, 64, 64, 16)
    assert simplify.count(plain, H) == w["info"]  # the (0, 0) filter needs no plane
    code, msg = code_of(lambda: simplify.count(plain, H, *HALF))
    assert code == _abi.GS_ERR_INVALID_ARGUMENT and "gs_cell_merge" in msg and "GS_FLAG_SPLAT_STATE" in msg
    code, msg = code_of(lambda: simplify.merge_cells(plain, H, op=_abi.GS_STATE_SET, bits=TAG))
    assert code == _abi.GS_ERR_INVALID_ARGUMENT and "GS_FLAG_SPLAT_STATE" in msg
    plain.destroy()


@pytest.mark.gpu
def test_simplify_is_kept_plus_merged(monkeypatch):
    """simplify(): the context then holds exactly the splats of no merged group, in order, followed by the records merge_cells
    returned; the state plane and the id map are the restatement's; an EXACT frame (both binnings, every tap) is a fresh context's of
    those records bit for bit; the tag is gone and a second simplify is not refused."""
    from gsplat import simplify
    s, u, W, Hh = state_scene("ragged")
    n = s.shape[0]
    st = (np.arange(n) * 5 % 64).astype(np.uint8)
    cell, new_state = 0.5, 0x22
    w = ms.merge(s, st, cell, *HALF)
    assert w["info"]["groups"] > 100
    r = _mk(s, W, Hh, 8, exact=True)
    r.write_state(st)
    frame_taps(r, u, False)
    records, info = simplify.merge_cells(r, cell, *HALF, device=True)
    records = records.cpu().numpy()
    assert info == w["info"]
    assert r.state_count(TAG, TAG) == 0
    # an insertion that fails leaves no tag behind and changes nothing else
    def no_room(*a, **kw):
        raise MemoryError("no room")
    monkeypatch.setattr(simplify.insert, "append", no_room)
    with pytest.raises(MemoryError):
        simplify.simplify(r, cell, *HALF, tag=TAG, new_state=new_state)
    monkeypatch.undo()
    same_bits(r.read_state(), st, "the tag is cleared after a failure")
    assert r.numGaussians == n
    info2, ids = simplify.simplify(r, cell, *HALF, tag=TAG, new_state=new_state, groups=info["groups"])  # (sized by the count above)
    want_rec, want_st, want_ids = ms.simplified(er.zero_padding(s), st, records, w["members"], new_state)
    assert info2 == w["info"] and r.numGaussians == n - info["members"] + info["groups"] == len(want_rec)
    same_bits(ids, want_ids, "id map")
    same_bits(raw_export(r, 0, 0, False)[0], want_rec, "kept old ++ merged records")
    same_bits(r.read_state(), want_st, "state plane")
    assert r.state_count(TAG, TAG) == 0
    fresh = _mk(want_rec, W, Hh, 8, exact=True)
    fresh.write_state(want_st)
    for debug in (False, True):
        a, b = frame_taps(r, u, debug), frame_taps(fresh, u, debug)
        for t in TAPS + ("rgba8", "rgbf"):
            np.testing.assert_array_equal(a[t], b[t], err_msg="%s debug=%s" % (t, debug))
    assert a["rgba8"][..., :3].any()
    fresh.destroy()
    info3, ids3 = simplify.simplify(r, cell)  # not refused: the tag bit is gone
    assert r.numGaussians == len(want_rec) - info3["members"] + info3["groups"] == len(ids3)
    # a splat that carries the tag refuses the verb before anything changes
    r.state_ids([0], 1, TAG)
    with pytest.raises(ValueError):
        simplify.simplify(r, cell)
    r.destroy()


@pytest.mark.gpu
def test_simplify_to_lands_at_or_below_its_target():
    from gsplat import simplify
    rec, st = scene_of(3001)
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    out = simplify.simplify_to(r, 1500)
    assert out["ids"] is not None and out["splats"] <= 1500 and out["splats"] == r.numGaussians and 2 <= out["probes"] <= 24
    assert out["edge"] == out["info"]["cell_edge"] > 0
    w = ms.merge(rec, st, out["edge"])
    assert out["info"] == w["info"] and out["splats"] == 3001 - w["info"]["members"] + w["info"]["groups"]
    same_bits(out["ids"], ms.simplified(rec, st, np.zeros((w["info"]["groups"], 80), F), w["members"], 0)[2], "id map")
    assert r.state_count(TAG, TAG) == 0
    none = simplify.simplify_to(r, 0)  # unreachable: at least one splat stays
    assert none["ids"] is None and none["splats"] == r.numGaussians
    r.destroy()
