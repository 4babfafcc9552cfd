"""Splat attributes: summarise, histogram, read and select resident splats by value (include/gsplat/gs_abi.h "splat attributes").

The reference every GPU answer is held to is tests/attr_restate.py: a numpy restatement of the value, the summary's key order, the
histogram's bin rule and the selection's membership.  The CPU tests pin the ABI, pin the restatement to what already exists (the
upload's smax expression, state_restate's projection depth and SPHERE membership) and walk the bin rule's edges by hand.  The GPU
tests compare bit for bit -- apart from the header's two exceptions, a NaN's payload and the sign of a zero fminf / fmaxf chose --
every kind, dense and filtered, at the quad and workgroup edges; and cover the frame after a selection, the ring, slabs and
borrowers, the lifecycle, the refusals, the editor's verbs and the Node host.
"""
import ctypes
import functools
import re

import numpy as np
import pytest

import attr_restate as ar
import state_restate as sr
from conftest import scene
from support import (F, NODE, SLAB_COLS, c_layout, code_of, frame_taps, guarded, host_sources, is_fill, mk, run_node, special_records, state_ref,
                     state_scene, timeless)

_mk = functools.partial(mk, state=True)
LENGTHS = (1, 3, 4, 5, 1023, 1024, 1025, 3001)  # the quad tail and the workgroup edges (1024 splats = 256 quads)
THIRD = (0x04, 0x04)                              # the filter of the plane _third makes
P_DIST2 = (0.5, 0.2, -0.3)
INF = float("inf")


def _third(n):
    """A plane with host bit 0x04 on every third splat and junk in bits 0, 1, 4, 5 and 6, which the filter must ignore (bits 3 and 7 stay
    clear for the tests that need a filter of their own)."""
    st = ((np.arange(n) * 7) & 0x73).astype(np.uint8)
    st[np.arange(n) % 3 == 0] |= 0x04
    return st


def _p(kind):
    if kind == ar.DIST2:
        return P_DIST2
    if kind == ar.PLANE:
        u = state_scene("cfgA")[1]
        return (u[2], u[6], u[10], u[14])
    return (0, 0, 0, 0)


def _attr(kind):
    from gsplat import attributes
    return attributes.attr(kind, _p(kind))


def hand_records():
    """About 40 hand-made records repeated into a scene of 1043 (N = 3 mod 4): all three log-scales NaN; log-scales that mix -0 and
    +0; +-inf positions and logits; and positions / logits exactly on the bounds the range tests use (-0.5 and 0.75)."""
    base = np.array(scene(10000)[:40], dtype=F, copy=True)
    w = base.view(np.uint32)
    base[0, 4:7] = np.nan
    w[1, 4:7] = 0x7FA12345                       # ... as payload NaNs
    base[2, 4:7] = (0.0, -0.0, 0.0)
    base[3, 4:7] = (-0.0, 0.0, -0.0)
    base[4, 4:7] = (-0.0, -0.0, -0.0)
    base[5, 4:7] = (0.0, -0.0, -1.0)
    base[6, 4:7] = (np.nan, 0.25, -0.0)
    base[7, 0], base[8, 1], base[9, 2] = np.inf, -np.inf, np.inf
    base[10, 12], base[11, 12] = np.inf, -np.inf
    base[12, 0], base[13, 0] = -0.5, 0.75
    base[14, 12], base[15, 12] = -0.5, 0.75
    base[16, 0], base[17, 0] = np.nextafter(F(-0.5), F(-1)), np.nextafter(F(0.75), F(0))
    base[18, 0], base[19, 0] = 0.0, -0.0
    base[20, 16:19] = (np.nan, -0.5, 0.75)
    base[21, 12] = np.nan
    return np.ascontiguousarray(np.concatenate([base] * 26 + [base[:3]]))


def _raw_read(r, a, where, with_ids):
    """gs_attr_read into buffers one entry longer than needed, pre-filled with 0xA5: (values, ids or None) after checking the guards."""
    from gsplat import _abi
    L = _abi.load()
    n = ctypes.c_uint64()
    _abi.check(L.gs_attr_read(r._ctx, ctypes.byref(a), where[0], where[1], None, 0, ctypes.byref(n), None))
    m = n.value
    dst, ids = guarded(m + 1, F), guarded(m + 1, np.uint32)
    n2 = ctypes.c_uint64()
    _abi.check(L.gs_attr_read(r._ctx, ctypes.byref(a), where[0], where[1], dst.ctypes.data, m + 1, ctypes.byref(n2), ids.ctypes.data if with_ids else None))
    assert n2.value == m
    assert is_fill(dst[m:]) and is_fill(ids[m:])
    if not with_ids:
        assert is_fill(ids)
    return dst[:m], (ids[:m] if with_ids else None)


def _same_summary(got, want, kind, cell=""):
    assert got["matched"] == want["matched"] and got["nan"] == want["nan"], (cell, got, want)
    for k in ("min", "max"):
        assert ar.same_values([got[k]], [want[k]], kind), (cell, k, got, want)


def _range_on_values(v):
    """(lo, hi) that ARE values of v (so some lie exactly on both ends) with values below and above: the 20 % and 80 % order
    statistics of the distinct finite values."""
    d = np.unique(v[np.isfinite(v)])
    assert d.size >= 5
    return F(d[d.size // 5]), F(d[(4 * d.size) // 5])


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_attr_abi(tmp_path):
    """The four symbols are exported and listed; gs_attr and gs_attr_summary are 24 bytes with the same offsets in the compiled
    header and in ctypes; the kind constants agree between the header, _abi and the Node ATTR table; GS_ABI_VERSION is still 3; a
    null context is refused by each call with a message that names it; the two renderer classes gained no public method."""
    import gsplat
    from gsplat import _abi
    L = _abi.load()
    names = ("gs_attr_summary", "gs_attr_histogram", "gs_attr_read", "gs_state_attr")
    for name in names:
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    a_fields = [n for n, _ in _abi.GsAttr._fields_]
    s_fields = [n for n, _ in _abi.GsAttrSummary._fields_]
    assert a_fields == ["struct_size", "kind", "p"] and s_fields == ["matched", "nan", "min", "max"]
    kinds = ["GS_ATTR_" + n for n in _abi.GS_ATTR_NAMES] + ["GS_ATTR_COUNT"]
    prog = 'printf("%d %zu %zu", GS_ABI_VERSION, sizeof(gs_attr), sizeof(struct gs_attr_summary));'
    prog += "".join('printf(" %%zu", offsetof(gs_attr, %s));' % n for n in a_fields)
    prog += "".join('printf(" %%zu", offsetof(struct gs_attr_summary, %s));' % n for n in s_fields)
    prog += "".join('printf(" %%d", (int)%s);' % k for k in kinds)
    out = c_layout(tmp_path, "attr_layout", prog)
    assert out[0] == 3 and L.gs_abi_version() == 3
    assert out[1] == 24 == ctypes.sizeof(_abi.GsAttr) and out[2] == 24 == ctypes.sizeof(_abi.GsAttrSummary)
    assert out[3:6] == [getattr(_abi.GsAttr, n).offset for n in a_fields] == [0, 4, 8]
    assert out[6:10] == [getattr(_abi.GsAttrSummary, n).offset for n in s_fields] == [0, 8, 16, 20]
    assert out[10:] == [getattr(_abi, k) for k in kinds] == list(range(17))
    assert [getattr(ar, n) for n in _abi.GS_ATTR_NAMES] == list(range(16)) and ar.COUNT == 16
    rjs, idx, dts, napi, hdr = host_sources()
    assert re.search(r"#define GS_ABI_VERSION 3\b", hdr)
    for name in names:
        assert re.search(r"int32_t %s\(gs_ctx\*" % name, hdr)
    m = re.search(r"const ATTR = \{([^}]*)\}", idx)
    assert [(k, int(v)) for k, v in re.findall(r"(\w+):\s*(\d+)", m.group(1))] == [(n, i) for i, n in enumerate(_abi.GS_ATTR_NAMES)]
    m = re.search(r"ATTR: \{([^}]*)\}", dts)
    assert [(k, int(v)) for k, v in re.findall(r"(\w+):\s*(\d+)", m.group(1))] == [(n, i) for i, n in enumerate(_abi.GS_ATTR_NAMES)]
    for fn in ("attrSummary", "attrHistogram", "attrValues", "stateAttr"):
        assert re.search(r"\b%s\(" % fn, dts) and re.search(r"\b%s\(" % fn, rjs) and '{"%s", js_' % fn in napi
    # no context: refused, with a message that names the call, before anything else is looked at
    a = _attr(ar.POS_X)
    n, s, cnt = ctypes.c_uint64(), _abi.GsAttrSummary(), np.zeros(4, np.uint64)
    calls = {"gs_attr_summary": lambda: L.gs_attr_summary(None, ctypes.byref(a), 0, 0, ctypes.byref(s)),
             "gs_attr_histogram": lambda: L.gs_attr_histogram(None, ctypes.byref(a), 0, 0, 0.0, 1.0, 1, cnt.ctypes.data),
             "gs_attr_read": lambda: L.gs_attr_read(None, ctypes.byref(a), 0, 0, None, 0, ctypes.byref(n), None),
             "gs_state_attr": lambda: L.gs_state_attr(None, ctypes.byref(a), 0.0, 1.0, 1, 0, 0, 1, 2, None)}
    for name, call in calls.items():
        assert call() == _abi.GS_ERR_INVALID_ARGUMENT
        msg = L.gs_last_error()
        assert name.encode() in msg and b"null ctx" in msg
    # a new module of free functions, re-exported; the classes keep their surface
    from gsplat import attributes
    assert gsplat.attributes is attributes
    for fn in ("attr", "summary", "histogram", "values", "select", "bounds", "centre", "depth_attr", "quantile"):
        assert callable(getattr(attributes, fn))
    for cls in (gsplat.Renderer, gsplat.PipelinedRenderer):
        assert not [m for m in dir(cls) if not m.startswith("_") and ("attr" in m.lower() or m in ("summary", "histogram", "quantile", "bounds", "centre"))]


def test_restatement_is_pinned():
    """value(LOG_SCALE_MAX) is the upload's smax expression; value(PLANE, view row 2) is state_restate.project's pvz bit for bit;
    value(DIST2) reproduces the SPHERE membership; the histogram's counts add up to matched; the summary's min and max are the
    values folded in the key order."""
    for name, rec in (("special", special_records(3001)), ("hand", hand_records())):
        l0, l1, l2 = rec[:, 4], rec[:, 5], rec[:, 6]
        smax = np.fmax(l0, np.fmax(l1, l2))
        assert ar.same_values(ar.value(ar.LOG_SCALE_MAX, rec), smax, ar.LOG_SCALE_MAX)
        got = ar.value(ar.ANISOTROPY, rec)
        assert (got[~np.isnan(got)] >= 0).all()
    s, u, W, H = state_scene("cfgA")
    for rec in (s, special_records(3001)):
        pvz = sr.project(rec, u, W, H)[4]
        got = ar.value(ar.PLANE, rec, _p(ar.PLANE))
        np.testing.assert_array_equal(got.view(np.uint32)[~np.isnan(pvz)], pvz.view(np.uint32)[~np.isnan(pvz)])
        assert (np.isnan(got) == np.isnan(pvz)).all()
        for a, b in (((0.0, 0.0, 0.0), 1.0), (P_DIST2, 0.75)):
            inside = sr.member(sr.SPHERE, rec, W, H, a=a, b=(b, 0, 0))
            d2 = ar.value(ar.DIST2, rec, a)
            np.testing.assert_array_equal(d2 <= F(b) * F(b), inside)
            np.testing.assert_array_equal(ar.select(d2, -INF, F(b) * F(b)), inside)
            assert 0 < inside.sum() < rec.shape[0]
    rec = special_records(3001)
    keep = _third(3001) & 0x04 != 0
    for kind in ar.SCENE_KINDS:
        v = ar.value(kind, rec, _p(kind))
        for kp in (None, keep):
            sm = ar.summary(v, kp)
            vv = v if kp is None else v[kp]
            for bins in (1, 7, 256, 1024):
                lo, hi = _range_on_values(vv)
                h = ar.histogram(v, lo, hi, bins, kp)
                assert h.size == bins + 3 and int(h.sum()) == sm["matched"] and int(h[bins + 2]) == sm["nan"]
            order = sorted((x for x in vv if not np.isnan(x)), key=lambda x: int(ar.keys([x])[0]))  # a fold in the key order
            assert sm["min"].view(np.uint32) == order[0].view(np.uint32) and sm["max"].view(np.uint32) == order[-1].view(np.uint32)
    # the key order: -inf < -1 < -0 < +0 < denormal < 1 < +inf, and the map inverts
    seq = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf], F)
    k = ar.keys(seq)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert [ar.unkey(x).view(np.uint32) for x in k] == list(seq.view(np.uint32))
    sm = ar.summary(np.array([0.0, -0.0, np.nan], F))
    assert sm["min"].view(np.uint32) == 0x80000000 and sm["max"].view(np.uint32) == 0 and sm["nan"] == 1 and sm["matched"] == 3
    assert ar.summary(np.array([np.nan], F)) == {"matched": 1, "nan": 1, "min": F(np.inf), "max": F(-np.inf)}


@pytest.mark.parametrize("bins", [1, 7, 256, 1024])
def test_bin_rule_edges(bins):
    """Hand-made values against hand-made answers: lo is the first bin, the float below it is below; hi and everything from it up
    is above, the float below hi is the last bin (the clamp: its product may round to `bins`); +-inf, NaN, -0 and +0."""
    lo, hi = F(-0.5), F(0.75)
    v = np.array([lo, np.nextafter(lo, F(-np.inf)), hi, np.nextafter(hi, F(-np.inf)), np.inf, -np.inf, np.nan, -0.0, 0.0], F)
    b = ar.bin_of(v, lo, hi, bins)
    zero = min(int(F(0.5) * (F(bins) / F(1.25))), bins - 1)
    assert list(b) == [0, bins, bins + 1, bins - 1, bins + 1, bins, bins + 2, zero, zero]
    h = ar.histogram(v, lo, hi, bins)
    assert int(h.sum()) == v.size and int(h[bins]) == 2 and int(h[bins + 1]) == 2 and int(h[bins + 2]) == 1
    # a range over zero: -0 and +0 are both on lo, hence in the first bin
    assert list(ar.bin_of(np.array([-0.0, 0.0], F), F(0.0), F(1.0), bins)) == [0, 0]
    assert list(ar.bin_of(np.array([-0.0, 0.0], F), F(-1.0), F(0.0), bins)) == [bins + 1, bins + 1]
    # an infinite scale (a denormal width): the value on lo is bin 0, everything else inside saturates into the last bin
    tiny, two = F(1e-45), F(3e-45)  # one and two spacings of the denormals
    with np.errstate(over="ignore"):
        assert tiny < two and not np.isfinite(F(1024) / two)
    assert list(ar.bin_of(np.array([0.0, tiny, two], F), F(0.0), two, 1024)) == [0, 1023, 1025]


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("length", LENGTHS)
def test_values_scene_kinds(length):
    """gs_attr_read of every scene kind, dense and filtered, on the first N special records: the restatement's values, ascending and
    correct ids, nothing written past *n."""
    from gsplat import attributes
    rec = np.ascontiguousarray(special_records(3001)[:length])
    st = _third(length)
    keep = np.flatnonzero(st & 0x04)
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    for kind in ar.SCENE_KINDS:
        want = ar.value(kind, rec, _p(kind))
        a = _attr(kind)
        got, ids = _raw_read(r, a, (0, 0), True)
        assert ar.same_values(got, want, kind), (kind, "dense")
        np.testing.assert_array_equal(ids, np.arange(length, dtype=np.uint32))
        got, ids = _raw_read(r, a, THIRD, True)
        np.testing.assert_array_equal(ids, keep.astype(np.uint32))
        assert ar.same_values(got, want[keep], kind), (kind, "filtered")
        got, ids = _raw_read(r, a, THIRD, False)
        assert ids is None and ar.same_values(got, want[keep], kind)
        _same_summary(attributes.summary(r, a), ar.summary(want), kind, (kind, length))
        _same_summary(attributes.summary(r, a, THIRD), ar.summary(want[keep]), kind, (kind, length, "filtered"))
    r.destroy()


@pytest.mark.gpu
def test_values_hand_records():
    from gsplat import attributes
    rec = hand_records()
    n = rec.shape[0]
    assert n % 4 == 3
    st = _third(n)
    allnan = np.isnan(rec[:, 4:7]).all(axis=1)
    st[allnan] |= 0x08
    keep = (st & 0x04) != 0
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    for kind in ar.SCENE_KINDS:
        want = ar.value(kind, rec, _p(kind))
        a = _attr(kind)
        assert ar.same_values(_raw_read(r, a, (0, 0), False)[0], want, kind), kind
        assert ar.same_values(_raw_read(r, a, THIRD, False)[0], want[keep], kind), kind
        _same_summary(attributes.summary(r, a), ar.summary(want), kind, kind)
        _same_summary(attributes.summary(r, a, THIRD), ar.summary(want, keep), kind, kind)
        # a filter that matches nothing
        assert attributes.summary(r, a, (0x80, 0x80)) == {"matched": 0, "nan": 0, "min": F(np.inf), "max": F(-np.inf)}
        assert attributes.values(r, a, (0x80, 0x80)).size == 0
    # a filter that matches only NaN values
    for kind in (ar.LOG_SCALE_MAX, ar.LOG_SCALE_MIN, ar.LOG_SCALE_SUM, ar.ANISOTROPY):
        sm = attributes.summary(r, _attr(kind), (0x08, 0x08))
        assert sm == {"matched": int(allnan.sum()), "nan": int(allnan.sum()), "min": F(np.inf), "max": F(-np.inf)} and sm["matched"] == 54
        c, below, above, nan = attributes.histogram(r, _attr(kind), -1.0, 1.0, 7, (0x08, 0x08))
        assert int(c.sum()) == 0 and (below, above, nan) == (0, 0, 54)
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("length", [10000, 9997])
def test_cover_kinds(length):
    """The COVER_* kinds against read_coverage put through the restatement: values, summary, select; before any accumulate the
    planes read as zeros."""
    from gsplat import _abi, attributes
    s, u, W, H = state_scene("cfgA")
    rec = np.ascontiguousarray(s[:length])
    r = _mk(rec, W, H, 16)
    st = _third(length)
    keep = (st & 0x04) != 0
    r.write_state(st)
    for kind in ar.COVER_KINDS:  # the planes are allocated and zeroed by the first call that needs them
        assert attributes.summary(r, _attr(kind)) == {"matched": length, "nan": 0, "min": F(0), "max": F(0)}
    r.render_uniforms(u)
    r.wait()
    r.accumulate_coverage()
    cov = r.read_coverage()
    assert 100 < (cov["hits"] > 0).sum() < length
    for kind in ar.COVER_KINDS:
        want = ar.value(kind, rec, cov=cov)
        a = _attr(kind)
        got, ids = _raw_read(r, a, (0, 0), True)
        assert ar.same_values(got, want, kind), kind
        got, ids = _raw_read(r, a, THIRD, True)
        np.testing.assert_array_equal(ids, np.flatnonzero(keep).astype(np.uint32))
        assert ar.same_values(got, want[keep], kind), kind
        _same_summary(attributes.summary(r, a), ar.summary(want), kind, kind)
        _same_summary(attributes.summary(r, a, THIRD), ar.summary(want, keep), kind, kind)
        lo, hi = _range_on_values(want[want > 0])
        for bins in (1, 7, 256, 1024):
            for where, kp in (((0, 0), None), (THIRD, keep)):
                c, below, above, nan = attributes.histogram(r, a, lo, hi, bins, where)
                wh = ar.histogram(want, lo, hi, bins, kp)
                np.testing.assert_array_equal(np.concatenate([c, [below, above, nan]]).astype(np.uint64), wh, err_msg=str((kind, bins, where)))
                assert below > 0 and above > 0
        for inside in (True, False):
            r.write_state(st)
            new, matched = sr.apply_region(st, ar.select(want, lo, hi, inside), sr.SET, sr.SELECTED, (0x04, 0x04))
            assert attributes.select(r, a, lo, hi, inside, where=THIRD) == matched > 0
            np.testing.assert_array_equal(r.read_state(), new)
    np.testing.assert_array_equal(r.read_coverage().view(np.uint32), cov.view(np.uint32))  # the planes are only read
    r.destroy()


@pytest.mark.gpu
def test_summary_spreads_over_slots():
    """scene(40000): 40 workgroups, more than GS_STATE_SLOTS = 32, so two of them share a slot; every kind, dense and filtered."""
    from gsplat import attributes
    rec = scene(40000)
    n = rec.shape[0]
    st = _third(n)
    keep = (st & 0x04) != 0
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    for kind in ar.SCENE_KINDS:
        want = ar.value(kind, rec, _p(kind))
        a = _attr(kind)
        _same_summary(attributes.summary(r, a), ar.summary(want), kind, kind)
        _same_summary(attributes.summary(r, a, THIRD), ar.summary(want, keep), kind, kind)
    new, matched = sr.apply_region(st, ar.select(ar.value(ar.POS_Y, rec), -0.25, 0.5), sr.TOGGLE, 0x22, THIRD)
    assert 0 < matched < int(keep.sum())
    assert attributes.select(r, _attr(ar.POS_Y), -0.25, 0.5, op=sr.TOGGLE, bits=0x22, where=THIRD) == matched
    np.testing.assert_array_equal(r.read_state(), new)
    r.destroy()


HIST_KINDS = (ar.POS_X, ar.OPACITY_LOGIT, ar.ANISOTROPY, ar.DC_G, ar.DIST2)  # (COVER_SUM: test_cover_kinds)


def _check_hist(r, rec, kinds, st, cell):
    from gsplat import attributes
    keep = (st & 0x04) != 0
    for kind in kinds:
        want = ar.value(kind, rec, _p(kind))
        a = _attr(kind)
        lo, hi = _range_on_values(want)
        assert (want == lo).any() and (want == hi).any() and (want < lo).any() and (want > hi).any()
        for bins in (1, 7, 256, 1024):
            for where, kp in (((0, 0), None), (THIRD, keep)):
                c, below, above, nan = attributes.histogram(r, a, lo, hi, bins, where)
                np.testing.assert_array_equal(np.concatenate([c, [below, above, nan]]).astype(np.uint64), ar.histogram(want, lo, hi, bins, kp),
                                              err_msg=str((cell, kind, bins, where)))
                assert int(c.sum()) + below + above + nan == (rec.shape[0] if kp is None else int(kp.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["special", "hand"])
def test_histogram(which):
    """All bins + 3 counts equal the restatement's, for ranges whose ends ARE values of the scene, with values below and above."""
    rec = special_records(3001) if which == "special" else hand_records()
    st = _third(rec.shape[0])
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    _check_hist(r, rec, HIST_KINDS, st, which)
    if which == "hand":  # the planted values: -0.5 and 0.75 exactly, their neighbours, +-0, +-inf, NaN
        from gsplat import attributes
        for kind in (ar.POS_X, ar.OPACITY_LOGIT, ar.DC_G, ar.DC_B, ar.DC_R):
            want = ar.value(kind, rec)
            for bins in (1, 7, 256, 1024):
                c, below, above, nan = attributes.histogram(r, _attr(kind), -0.5, 0.75, bins)
                np.testing.assert_array_equal(np.concatenate([c, [below, above, nan]]).astype(np.uint64), ar.histogram(want, -0.5, 0.75, bins))
    r.destroy()


@pytest.mark.gpu
def test_histogram_grid_and_one_bin():
    """scene(40000) with GS_OPT_PERSISTENT_GRID 1 and 2: the grid-stride loop makes 40 and 20 trips, and the counts are those of
    the default grid and of the restatement.  And the contention worst case: a range whose first bin holds every splat."""
    from gsplat import _abi, attributes
    rec = scene(40000)
    n = rec.shape[0]
    st = _third(n)
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    _check_hist(r, rec, HIST_KINDS, st, "default grid")
    x = ar.value(ar.POS_X, rec)
    lo = x.min()
    hi = F(lo + F(2048.0) * (x.max() - lo + F(1.0)))  # 1024 bins, each wider than the whole scene
    assert (ar.bin_of(x, lo, hi, 1024) == 0).all()
    default = {}
    for grid in (0, 1, 2):
        if grid:
            r.set_option(_abi.GS_OPT_PERSISTENT_GRID, grid)
            _check_hist(r, rec, HIST_KINDS, st, "grid %d" % grid)
        for bins in (256, 1024):
            c, below, above, nan = attributes.histogram(r, _attr(ar.POS_X), lo, hi, bins)
            assert int(c[0]) == n and int(c[1:].sum()) == 0 and (below, above, nan) == (0, 0, 0)
            c, below, above, nan = attributes.histogram(r, _attr(ar.POS_X), lo, hi, bins, THIRD)
            assert int(c[0]) == int(((st & 0x04) != 0).sum()) and int(c[1:].sum()) == 0
        got = attributes.histogram(r, _attr(ar.DIST2), 0.0, 4.0, 256)
        default.setdefault("dist2", got)
        np.testing.assert_array_equal(got[0], default["dist2"][0])
        assert got[1:] == default["dist2"][1:]
    r.destroy()


OPS = (sr.SET, sr.CLEAR, sr.TOGGLE, sr.ASSIGN)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["special", "hand"])
def test_select(which):
    """Every op, inside 0 and 1, a where filter, infinite bounds and the empty range lo > hi: the plane and `matched` equal the
    restatement's through state_restate.apply_region.  The NaN finder selects exactly the NaN splats."""
    from gsplat import attributes
    rec = special_records(3001) if which == "special" else hand_records()
    n = rec.shape[0]
    st = np.random.default_rng(5).integers(0, 256, n).astype(np.uint8)
    r = _mk(rec, 64, 64, 16)
    for kind in (ar.POS_X, ar.OPACITY_LOGIT, ar.LOG_SCALE_MAX, ar.LOG_SCALE_MIN, ar.ANISOTROPY, ar.DC_R, ar.DIST2, ar.PLANE):
        v = ar.value(kind, rec, _p(kind))
        a = _attr(kind)
        lo, hi = _range_on_values(v)
        ranges = [(lo, hi), (-INF, hi), (lo, INF), (-INF, INF), (hi, lo), (lo, lo)]
        if kind in (ar.POS_X, ar.OPACITY_LOGIT):
            ranges.append((-0.5, 0.75))
        for k, (a0, a1) in enumerate(ranges):
            for inside in (True, False):
                op, bits = OPS[(k + int(inside)) % 4], (0x02, 0xA4)[k % 2]
                where = ((0, 0), (0x0C, 0x04), (0x30, 0x10))[(k + kind) % 3]
                r.write_state(st)
                member = ar.select(v, a0, a1, inside)
                new, matched = sr.apply_region(st, member, op, bits, where)
                cell = (kind, a0, a1, inside, op, bits, where)
                assert attributes.select(r, a, a0, a1, inside, op, bits, where) == matched, cell
                np.testing.assert_array_equal(r.read_state(), new, err_msg=str(cell))
                if a0 > a1:
                    assert member.sum() == (0 if inside else n)
        # the NaN finder
        r.write_state(np.zeros(n, np.uint8))
        found = attributes.select(r, a, -INF, INF, inside=False)
        assert found == int(np.isnan(v).sum())
        np.testing.assert_array_equal(np.flatnonzero(r.read_state() & sr.SELECTED), np.flatnonzero(np.isnan(v)))
    if which == "special":
        assert sum(int(np.isnan(ar.value(k, rec, _p(k))).sum()) for k in (ar.POS_X, ar.OPACITY_LOGIT, ar.LOG_SCALE_MIN, ar.DC_R)) > 0
    # every op on one range
    v = ar.value(ar.OPACITY_LOGIT, rec)
    lo, hi = _range_on_values(v)
    for op in OPS:
        for bits in (0x02, 0xA4):
            r.write_state(st)
            new, matched = sr.apply_region(st, ar.select(v, lo, hi), op, bits, (0x0C, 0x04))
            assert attributes.select(r, _attr(ar.OPACITY_LOGIT), lo, hi, True, op, bits, (0x0C, 0x04)) == matched > 0
            np.testing.assert_array_equal(r.read_state(), new)
    r.destroy()


@pytest.mark.gpu
def test_select_then_hide_frame(oracle):
    """select(OPACITY_LOGIT < t) then hide_selected: the next EXACT frame equals the constructed reference of that plane in every tap."""
    from gpu_checks import check_stages
    from gsplat import _abi, attributes
    s, u, W, H = state_scene("cfgA")
    v = ar.value(ar.OPACITY_LOGIT, s)
    t = F(np.sort(v)[v.size // 4])
    below = np.nextafter(t, F(-np.inf))
    member = ar.select(v, -INF, below)
    assert 0 < member.sum() < v.size and not member[v == t].any()
    state = np.where(member, sr.HIDDEN | sr.SELECTED, 0).astype(np.uint8)
    ref = state_ref(oracle, "cfgA", 16, "opacity_below_q25", state)
    r = _mk(s, W, H, 16, exact=True)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    assert attributes.select(r, _attr(ar.OPACITY_LOGIT), -INF, below) == int(member.sum())
    assert r.hide_selected() == int(member.sum())
    np.testing.assert_array_equal(r.read_state(), state)
    r.render_uniforms(u, debug=True)
    r.wait()
    check_stages(r, ref, True, debug=True)
    r.destroy()


def _answers(r, rec_n):
    """What the three read-only calls return for a few kinds, dense and filtered, as comparable tuples."""
    from gsplat import attributes
    out = []
    for kind in (ar.POS_X, ar.OPACITY_LOGIT, ar.DC_B, ar.DIST2, ar.LOG_SCALE_MAX):
        a = _attr(kind)
        for where in ((0, 0), THIRD):
            sm = attributes.summary(r, a, where)
            c, below, above, nan = attributes.histogram(r, a, -0.5, 0.75, 7, where)
            out.append((kind, where, sm["matched"], sm["nan"], int(sm["min"].view(np.uint32)), int(sm["max"].view(np.uint32)),
                        tuple(int(x) for x in c), below, above, nan, attributes.values(r, a, where).tobytes()))
    return out


def _want_answers(rec, st):
    out = []
    for kind in (ar.POS_X, ar.OPACITY_LOGIT, ar.DC_B, ar.DIST2, ar.LOG_SCALE_MAX):
        v = ar.value(kind, rec, _p(kind))
        for where in ((0, 0), THIRD):
            kp = None if where == (0, 0) else (st & 0x04) != 0
            sm = ar.summary(v, kp)
            h = ar.histogram(v, -0.5, 0.75, 7, kp)
            out.append((kind, where, sm["matched"], sm["nan"], int(sm["min"].view(np.uint32)), int(sm["max"].view(np.uint32)),
                        tuple(int(x) for x in h[:7]), int(h[7]), int(h[8]), int(h[9]), (v if kp is None else v[kp]).tobytes()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_attributes_disturb_nothing(graph):
    """Config A, three frames in flight (and again with the frame graph): frames are enqueued, the three read-only calls are made
    without waiting -- they return the right numbers, so the ring was drained --, and the next frame's taps, image and statistics
    are those of a context that never made the calls."""
    from gsplat import _abi, synth
    s, u, W, H = state_scene("cfgA")
    st = _third(s.shape[0])
    cams = [synth.orbit_camera(k, W, H).uniforms(W, H) for k in (1, 7, 2)]
    want = _want_answers(s, st)
    a, b = _mk(s, W, H, 16), _mk(s, W, H, 16)
    for r in (a, b):
        r.set_option(_abi.GS_OPT_FRAME_GRAPH, graph)
        r.write_state(st)
    for rep in range(2):
        for uu in cams:
            a.render_uniforms(uu)
            b.render_uniforms(uu)
        assert _answers(a, s.shape[0]) == want  # (no wait in between)
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
def test_slab_and_borrower_answer_the_same():
    s, u, W, H = state_scene("cfgA")
    st = _third(s.shape[0])
    want = _want_answers(s, st)
    owner = _mk(s, W, H, 16)
    owner.write_state(st)
    assert _answers(owner, s.shape[0]) == want
    slab = _mk(s, W, H, 16, cols=SLAB_COLS[16])
    slab.write_state(st)
    assert _answers(slab, s.shape[0]) == want
    slab.destroy()
    borrower = _mk(s, W, H, 16, share_with=owner)  # (shares the owner's plane)
    assert _answers(borrower, s.shape[0]) == want
    borrower.destroy()
    import gsplat
    from gsplat import _abi
    p = gsplat.PipelinedRenderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(s), 16, frames_in_flight=2, flags=_abi.GS_FLAG_SPLAT_STATE)
    p.write_state(st)
    p.render_uniforms(u)
    p.render_uniforms(u)
    assert _answers(p, s.shape[0]) == want
    p.destroy()
    owner.destroy()


@pytest.mark.gpu
def test_attr_refusals_and_lifecycle():
    from gsplat import _abi, attributes
    L = _abi.load()
    s, u, W, H = state_scene("cfgA")
    n = s.shape[0]
    INV = _abi.GS_ERR_INVALID_ARGUMENT
    a = _attr(ar.POS_X)
    sm, cnt, nn = _abi.GsAttrSummary(), np.zeros(1027, np.uint64), ctypes.c_uint64()
    # before any upload: GS_ERR_NO_SCENE from all four
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(_abi.GsConfig), W, H, 16, _abi.GS_FLAG_SPLAT_STATE
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    assert L.gs_attr_summary(ctx, ctypes.byref(a), 0, 0, ctypes.byref(sm)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_attr_histogram(ctx, ctypes.byref(a), 0, 0, 0.0, 1.0, 4, cnt.ctypes.data) == _abi.GS_ERR_NO_SCENE
    assert L.gs_attr_read(ctx, ctypes.byref(a), 0, 0, None, 0, ctypes.byref(nn), None) == _abi.GS_ERR_NO_SCENE
    assert L.gs_state_attr(ctx, ctypes.byref(a), 0.0, 1.0, 1, 0, 0, 1, 2, None) == _abi.GS_ERR_NO_SCENE
    # N == 0: zero results, GS_OK
    _abi.check(L.gs_upload_splats(ctx, None, 0))
    _abi.check(L.gs_attr_summary(ctx, ctypes.byref(a), 0, 0, ctypes.byref(sm)))
    assert (sm.matched, sm.nan, sm.min, sm.max) == (0, 0, INF, -INF)
    cnt[:] = 7
    _abi.check(L.gs_attr_histogram(ctx, ctypes.byref(a), 0, 0, 0.0, 1.0, 4, cnt.ctypes.data))
    assert not cnt[:7].any() and (cnt[7:] == 7).all()
    nn.value = 9
    _abi.check(L.gs_attr_read(ctx, ctypes.byref(a), 0, 0, None, 0, ctypes.byref(nn), None))
    assert nn.value == 0
    m = ctypes.c_uint64(9)
    _abi.check(L.gs_state_attr(ctx, ctypes.byref(a), 0.0, 1.0, 1, 0, 0, 1, 2, ctypes.byref(m)))
    assert m.value == 0
    L.gs_destroy(ctx)

    r = _mk(s, W, H, 16)
    st = _third(n)
    r.write_state(st)

    def every_call(at, mask=0, value=0):
        return [("gs_attr_summary", lambda: L.gs_attr_summary(r._ctx, at, mask, value, ctypes.byref(sm))),
                ("gs_attr_histogram", lambda: L.gs_attr_histogram(r._ctx, at, mask, value, 0.0, 1.0, 4, cnt.ctypes.data)),
                ("gs_attr_read", lambda: L.gs_attr_read(r._ctx, at, mask, value, None, 0, ctypes.byref(nn), None)),
                ("gs_state_attr", lambda: L.gs_state_attr(r._ctx, at, 0.0, 1.0, 1, mask, value, 1, 2, None))]

    def refused(calls, *fragments):
        for name, call in calls:
            assert call() == INV, name
            msg = L.gs_last_error().decode()
            assert name in msg and all(f in msg for f in fragments), msg

    bad = attributes.attr(ar.POS_X)
    bad.struct_size = 20
    refused(every_call(ctypes.byref(bad)), "struct_size 20")
    refused(every_call(ctypes.byref(attributes.attr(ar.COUNT))), "kind 16")
    refused(every_call(ctypes.byref(attributes.attr(99))), "kind 99")
    refused(every_call(None), "null attribute")
    refused(every_call(ctypes.byref(attributes.attr(ar.DIST2, (0, float("nan"), 0)))), "p[1]", "not finite")
    refused(every_call(ctypes.byref(attributes.attr(ar.PLANE, (0, 0, 1, INF)))), "p[3]", "not finite")
    for ok in (attributes.attr(ar.DIST2, (0, 0, 0, float("nan"))), attributes.attr(ar.POS_Y, (INF, INF, INF, INF))):  # p the kind does not name
        for name, call in every_call(ctypes.byref(ok)):
            assert call() == 0, name
    r.write_state(st)
    refused(every_call(ctypes.byref(a), 0x100, 0)[:3], "0x100", "does not fit the state byte")
    refused(every_call(ctypes.byref(a), 0, 0x1FF)[:3], "0x1ff", "does not fit the state byte")
    refused(every_call(ctypes.byref(a), 0x100, 0)[3:], "where_mask 0x100")
    # the histogram's own
    hist = lambda lo, hi, bins: [("gs_attr_histogram", lambda: L.gs_attr_histogram(r._ctx, ctypes.byref(a), 0, 0, lo, hi, bins, cnt.ctypes.data))]
    cnt[:] = 7
    refused(hist(0.0, 1.0, 0), "0 bins")
    refused(hist(0.0, 1.0, 1025), "1025 bins")
    refused(hist(float("nan"), 1.0, 4), "not finite")
    refused(hist(0.0, INF, 4), "not finite")
    refused(hist(-INF, 0.0, 4), "not finite")
    refused(hist(1.0, 1.0, 4), "empty")
    refused(hist(2.0, 1.0, 4), "empty")
    refused(hist(-3e38, 3e38, 4), "width")
    refused([("gs_attr_histogram", lambda: L.gs_attr_histogram(r._ctx, ctypes.byref(a), 0, 0, 0.0, 1.0, 4, None))], "null counts")
    assert (cnt == 7).all()
    refused([("gs_attr_summary", lambda: L.gs_attr_summary(r._ctx, ctypes.byref(a), 0, 0, None))], "null summary")
    # the read's conventions are gs_state_list's
    refused([("gs_attr_read", lambda: L.gs_attr_read(r._ctx, ctypes.byref(a), 0, 0, None, 0, None, None))], "null n")
    keep = np.flatnonzero(st & 0x04)
    buf, ids = guarded(n, F), guarded(n, np.uint32)
    for where, need in (((0, 0), n), (THIRD, keep.size)):
        assert L.gs_attr_read(r._ctx, ctypes.byref(a), where[0], where[1], buf.ctypes.data, need - 1, ctypes.byref(nn), ids.ctypes.data) == INV
        assert ("%d values needed" % need).encode() in L.gs_last_error() and nn.value == need
        assert is_fill(buf) and is_fill(ids)
    # gs_state_attr's own: nothing is applied
    sel = lambda lo, hi, op, bits: [("gs_state_attr", lambda: L.gs_state_attr(r._ctx, ctypes.byref(a), lo, hi, 1, 0, 0, op, bits, ctypes.byref(m)))]
    m.value = 77
    refused(sel(float("nan"), 1.0, 1, 2), "not a number")
    refused(sel(0.0, float("nan"), 1, 2), "not a number")
    refused(sel(0.0, 1.0, 0, 2), "unknown op 0")
    refused(sel(0.0, 1.0, 5, 2), "unknown op 5")
    refused(sel(0.0, 1.0, 1, 0x100), "0x100")
    assert m.value == 77
    np.testing.assert_array_equal(r.read_state(), st)
    # after translate_selected the bounds move by the translation's f32 result
    lo, hi = (-1.0, -0.5, -1.0), (0.5, 1.0, 1.5)
    r.write_state(np.zeros(n, np.uint8))
    inside = sr.member(sr.BOX, s, W, H, a=lo, b=hi)
    assert r.select_box(lo, hi) == int(inside.sum()) > 100
    b0 = attributes.bounds(r)
    pos = s[inside, 0:3]
    np.testing.assert_array_equal(b0[0], pos.min(axis=0))
    np.testing.assert_array_equal(b0[1], pos.max(axis=0))
    assert b0[2] == int(inside.sum())
    t = np.array([0.3, -1.7, 12.5], F)
    r.translate_selected(t)
    b1 = attributes.bounds(r)
    np.testing.assert_array_equal(b1[0], b0[0] + t)  # (x + t is monotonic in x: the bounds are the old bounds' images)
    np.testing.assert_array_equal(b1[1], b0[1] + t)
    moved = np.array(s, copy=True)
    moved[inside, 0:3] = moved[inside, 0:3] + t
    np.testing.assert_array_equal(attributes.values(r, _attr(ar.POS_Z)).view(np.uint32), moved[:, 2].view(np.uint32))
    # after a compaction the values are those of the kept records, in order
    r.write_state(st)
    ids = r.compact(*THIRD)
    np.testing.assert_array_equal(ids, keep.astype(np.uint32))
    for kind in (ar.POS_X, ar.OPACITY_LOGIT, ar.DC_G, ar.ANISOTROPY, ar.DIST2):
        want = ar.value(kind, moved[keep], _p(kind))
        assert ar.same_values(attributes.values(r, _attr(kind)), want, kind)
        _same_summary(attributes.summary(r, _attr(kind)), ar.summary(want), kind)
    for kind in ar.COVER_KINDS:  # the planes were dropped with the old scene: they read as zeros for the new N
        assert attributes.summary(r, _attr(kind)) == {"matched": keep.size, "nan": 0, "min": F(0), "max": F(0)}
    r.destroy()
    # a context without the plane: (0, 0) works, any other filter and gs_state_attr are refused
    q = mk(s, W, H, 16)
    _same_summary(attributes.summary(q, a), ar.summary(s[:, 0]), ar.POS_X)
    assert ar.same_values(attributes.values(q, a), s[:, 0], ar.POS_X)
    c, below, above, nan = attributes.histogram(q, a, -0.5, 0.75, 7)
    np.testing.assert_array_equal(np.concatenate([c, [below, above, nan]]).astype(np.uint64), ar.histogram(s[:, 0], -0.5, 0.75, 7))
    for fn in (lambda: attributes.summary(q, a, THIRD), lambda: attributes.histogram(q, a, 0, 1, 4, THIRD), lambda: attributes.values(q, a, THIRD),
               lambda: attributes.select(q, a, 0, 1)):
        code, msg = code_of(fn)
        assert code == INV and "GS_FLAG_SPLAT_STATE" in msg
    q.destroy()


@pytest.mark.gpu
def test_verbs():
    """centre of a select_box selection lies inside the box and is the restated midpoint; depth_attr is the projection's depth;
    quantile(OPACITY_LOGIT, 0.3) is within its documented resolution of numpy's lower order statistic of values()."""
    from gsplat import attributes
    s, u, W, H = state_scene("cfgA")
    r = _mk(s, W, H, 16)
    lo, hi = np.array([-1.0, -0.5, -1.0], F), np.array([0.5, 1.0, 1.5], F)
    inside = sr.member(sr.BOX, s, W, H, a=lo, b=hi)
    assert r.select_box(lo, hi) == int(inside.sum())
    c = attributes.centre(r)
    pmin, pmax = s[inside, 0:3].min(axis=0), s[inside, 0:3].max(axis=0)
    np.testing.assert_array_equal(c.view(np.uint32), (pmin + (pmax - pmin) / F(2)).view(np.uint32))
    assert c.dtype == F and (c >= lo).all() and (c <= hi).all()
    assert r.rotate_selected((0.9, 0.1, 0.2, 0.3), pivot=attributes.centre(r)) == int(inside.sum())  # what the pivot is for
    r.clear_selection()
    with pytest.raises(ValueError):
        attributes.centre(r)
    pvz = sr.project(s, u, W, H)[4]
    rec = r.export_splats()
    np.testing.assert_array_equal(attributes.values(r, attributes.depth_attr(u)).view(np.uint32), sr.project(rec, u, W, H)[4].view(np.uint32))
    assert pvz.shape == (s.shape[0],)
    a = _attr(ar.OPACITY_LOGIT)
    v = attributes.values(r, a)
    for q in (0.0, 0.3, 0.5, 0.99, 1.0):
        got = attributes.quantile(r, a, q)
        want = np.quantile(v.astype(np.float64), q, method="lower")
        res = attributes.QUANTILE_RESOLUTION * (float(v.max()) - float(v.min())) + 2.0 * float(np.spacing(np.abs(v).max()))
        print("quantile %.2f: got %.7g, order statistic %.7g, resolution %.3g" % (q, got, want, res))
        assert abs(float(got) - want) <= res, (q, got, want, res)
    st = _third(s.shape[0])
    r.write_state(st)
    got = attributes.quantile(r, a, 0.3, THIRD)
    vk = v[(st & 0x04) != 0]
    assert abs(float(got) - np.quantile(vk.astype(np.float64), 0.3, method="lower")) <= attributes.QUANTILE_RESOLUTION * float(vk.max() - vk.min()) + 2e-6
    r.destroy()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_node_host_attributes_match_python(tmp_path):
    """attr_check.js on the ragged golden scene: its summary, histogram, first values and stateAttr count are the Python host's."""
    from gsplat import _abi, attributes
    s, u, W, H = state_scene("ragged")
    n = s.shape[0]
    rec = str(tmp_path / "rec.bin")
    np.ascontiguousarray(s, dtype=F).tofile(rec)
    info = run_node("attr_check.js", (rec, n, W, H, 8))
    r = _mk(s, W, H, 8)
    r.state_region(_abi.GS_REGION_SPHERE, _abi.GS_STATE_SET, 0x04, a=(0, 0, 0), b=(1.5, 0, 0))
    a = _attr(ar.OPACITY_LOGIT)
    for where, key in (((0, 0), "dense"), (THIRD, "filtered")):
        sm = attributes.summary(r, a, where)
        got = info[key]
        assert (got["matched"], got["nan"]) == (sm["matched"], sm["nan"])
        assert F(got["min"]) == sm["min"] and F(got["max"]) == sm["max"]
        c, below, above, nan = attributes.histogram(r, a, -2.0, 3.0, 16, where)
        assert got["histogram"] == {"counts": [int(x) for x in c], "below": below, "above": above, "nan": nan}
        v, ids = attributes.values(r, a, where, with_ids=True)
        assert got["count"] == v.size
        assert [F(x) for x in got["first"]] == list(v[:8]) and got["firstIds"] == [int(x) for x in ids[:8]]
    d2 = attributes.attr(ar.DIST2, P_DIST2)
    assert info["dist2Max"] == float(attributes.summary(r, d2)["max"])
    assert info["stateAttr"] == attributes.select(r, a, -INF, 0.0, where=THIRD) > 0
    assert info["selected"] == r.state_count(_abi.GS_SPLAT_SELECTED, _abi.GS_SPLAT_SELECTED)
    assert info["nanFinder"] == attributes.select(r, a, -INF, INF, inside=False) == 0
    assert info["errors"] == {"kind": "-1", "bins": "-1"}
    r.destroy()
