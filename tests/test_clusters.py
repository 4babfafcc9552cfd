"""Clusters: label the splats connected within a radius, select by cluster (include/gsplat/gs_abi.h "clusters").

The reference every GPU answer is held to is tests/cluster_restate.py: a breadth-first search over the links that
tests/neigh_restate.py's f32 expression gives.  The CPU tests pin the restatement by hand (a lattice whose links sit exactly on the
radius, a chain of 4096 exact floats, duplicates, special floats) and the ABI.  The GPU tests compare with np.array_equal on uint32
-- there is no tolerance anywhere -- over grids of many cells and of one, a cluster 4095 links long under three index orders,
filters, special floats, placement, the two selections, the editor's verbs, the planes' lifecycle, the work budget and the refusals.
"""
import ctypes
import functools
import re

import numpy as np
import pytest

import cluster_restate as cr
import state_restate as sr
from conftest import scene
from support import F, SLAB_COLS, c_layout, cached, code_of, frame_taps, host_sources, mk, state_scene, timeless
from test_neighbours import lattice_pos, records, special_pos

_mk = functools.partial(mk, state=True)
NONE = 2**32 - 1
OPS = (sr.SET, sr.CLEAR, sr.TOGGLE, sr.ASSIGN)
BELOW = float(np.nextafter(F(0.25), F(0)))
RAGGED = {0.1: (2936, 3), 0.3: (1860, 482), 0.5: (1091, 1711), 2.0: (536, 2286), 1e3: (1, 3001)}  # radius: (clusters, largest)


def want(key, pos, radius, members=None):
    """The restatement, once per key (which names pos and members) and session."""
    return cached(("clusters", key, float(radius)), lambda: cr.components(pos, radius, members))


def chain_pos(order):
    """x = 0.25 k, k < 4096 (every value and every difference exact in f32), splat i at k = order[i]."""
    p = np.zeros((4096, 3), F)
    p[:, 0] = np.asarray(order, F) * F(0.25)
    return p


def chain_orders():
    k = np.arange(4096)
    return {"ascending": k, "reversed": k[::-1].copy(), "permuted": np.random.default_rng(7).permutation(4096)}


def ragged():
    from gsplat import synth
    return cached("ragged_records", lambda: synth.bicycle_like(3001))


def info_counts(labels, sizes):
    """(members, clusters, largest) of two planes."""
    return int((labels != NONE).sum()), int((labels == np.arange(labels.size)).sum()), int(sizes.max()) if sizes.size else 0


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_restatement_is_pinned():
    p = lattice_pos()
    l, s = cr.components(p, 0.25)
    assert l.dtype == s.dtype == np.uint32
    assert not l.any() and (s == 216).all()  # one cluster of 216 with label 0
    l, s = cr.components(p, BELOW)
    assert np.array_equal(l, np.arange(216)) and (s == 1).all()  # 216 singletons
    # the chain: one cluster; with the member at k = 2000 filtered out two, of 2000 and 2095, whatever the index order
    for name, order in chain_orders().items():
        pos = chain_pos(order)
        l, s = want("chain_" + name, pos, 0.25)
        assert not l.any() and (s == 4096).all(), name
        assert (want("chain_" + name, pos, BELOW)[1] == 1).all()
        mem = order != 2000
        l, s = want("chain_cut_" + name, pos, 0.25, mem)
        low, high = order < 2000, order > 2000
        assert (s[low] == 2000).all() and (s[high] == 2095).all() and s[~mem].tolist() == [0] and l[~mem].tolist() == [NONE], name
        assert (l[low] == np.flatnonzero(low)[0]).all() and (l[high] == np.flatnonzero(high)[0]).all(), name
    order = chain_orders()["reversed"]
    assert want("chain_cut_reversed", chain_pos(order), 0.25, order != 2000)[0][0] == 0 and np.flatnonzero(order < 2000)[0] == 2096
    # duplicates at radius 0; NaN / inf members are singletons, also among their own duplicates
    dup = np.array([[1, 2, 3], [9, 9, 9], [1, 2, 3], [np.nan, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [1, 2, 3], [np.inf, 0, 0]], F)
    for radius in (0.0, 1e-40):  # a denormal radius: its square is 0
        l, s = cr.components(dup, radius)
        assert l.tolist() == [0, 1, 0, 3, 4, 5, 0, 7] and s.tolist() == [3, 1, 3, 1, 1, 1, 3, 1]
    l, s = cr.components(dup, 1e3)
    assert l.tolist() == [0, 0, 0, 3, 4, 5, 0, 7] and s.tolist() == [4, 4, 4, 1, 1, 1, 4, 1]
    l, s = cr.components(dup, 1e3, [0, 1, 1, 1, 0, 0, 1, 1])
    assert l.tolist() == [NONE, 1, 1, 3, NONE, NONE, 1, 7] and s.tolist() == [0, 3, 3, 1, 0, 0, 3, 1]
    # the ragged scene's table, and a removed bridge
    for radius, (clusters, largest) in RAGGED.items():
        l, s = want("ragged", ragged(), radius)
        assert info_counts(l, s) == (3001, clusters, largest), radius
        assert np.array_equal(s, np.bincount(l, minlength=3001)[l]) and (l <= np.arange(3001)).all()
    three = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F)
    assert cr.components(three, 1.0)[0].tolist() == [0, 0, 0] and cr.components(three, 1.0, [1, 0, 1])[0].tolist() == [0, NONE, 2]
    # the two memberships
    assert cr.member([0, 1, 2, 3], 1, 2).tolist() == [False, True, True, False]
    assert cr.member([0, 1, 2, 3], 2, 1, inside=False).all()
    assert cr.linked([0, 0, 2, NONE, 4, 4], [0, 1, 0, 1, 0, 0]).tolist() == [True, True, False, False, False, False]
    assert not cr.linked([0, 0, NONE], [0, 0, 1]).any()


def test_restatement_against_scipy():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    rec = ragged()
    p = np.asarray(rec[:, 0:3], F)
    for radius in (0.3, 0.5):
        with np.errstate(all="ignore"):
            d = p[None, :, :] - p[:, None, :]
            adj = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= F(radius) * F(radius)
        k, comp = connected_components(sp.csr_matrix(adj), directed=False)
        first = np.full(k, p.shape[0])
        np.minimum.at(first, comp, np.arange(p.shape[0]))
        l, s = want("ragged", rec, radius)
        assert np.array_equal(l, first[comp]) and np.array_equal(s, np.bincount(comp)[comp])


def test_cluster_abi(tmp_path):
    """The four symbols are exported and listed; gs_cluster is 32 bytes and gs_cluster_info 56 with the same offsets in the compiled
    header and in ctypes; GS_ABI_VERSION is still 3 and GS_ATTR_COUNT still 16; the header states the expression, the label and the
    planes' lifetime; a null context is refused by name; the Python host is a module and no method."""
    import gsplat
    from gsplat import _abi, clusters
    L = _abi.load()
    names = ("gs_cluster_label", "gs_cluster_read", "gs_state_cluster", "gs_state_cluster_linked")
    for name in names:
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    q_fields = [n for n, _ in _abi.GsCluster._fields_]
    i_fields = [n for n, _ in _abi.GsClusterInfo._fields_]
    assert q_fields == ["struct_size", "radius", "mask", "value", "reserved", "max_candidates"]
    assert i_fields == ["members", "clusters", "largest", "candidates", "rounds", "cells", "cell_edge", "reserved"]
    prog = 'printf("%d %d %zu %zu", GS_ABI_VERSION, (int)GS_ATTR_COUNT, sizeof(gs_cluster), sizeof(gs_cluster_info));'
    prog += "".join('printf(" %%zu", offsetof(gs_cluster, %s));' % n for n in q_fields)
    prog += "".join('printf(" %%zu", offsetof(gs_cluster_info, %s));' % n for n in i_fields)
    prog += 'printf(" %u %u", GS_CLUSTER_NONE == 0xFFFFFFFFu, GS_CLUSTER_MAX_ROUNDS);'
    out = c_layout(tmp_path, "cluster_layout", prog)
    assert out[0] == 3 and L.gs_abi_version() == 3 and out[1] == 16 == _abi.GS_ATTR_COUNT
    assert out[2] == 32 == ctypes.sizeof(_abi.GsCluster) and out[3] == 56 == ctypes.sizeof(_abi.GsClusterInfo)
    assert out[4:10] == [getattr(_abi.GsCluster, n).offset for n in q_fields] == [0, 4, 8, 12, 16, 24]
    assert out[10:18] == [getattr(_abi.GsClusterInfo, n).offset for n in i_fields] == [0, 8, 16, 24, 32, 36, 48, 52]
    assert out[18:] == [1, 64] and _abi.GS_CLUSTER_NONE == NONE == clusters.NONE == cr.NONE and _abi.GS_CLUSTER_MAX_ROUNDS == 64
    hdr = host_sources().hdr
    assert re.search(r"#define GS_ABI_VERSION 3\b", hdr)
    for name in names:
        assert re.search(r"int32_t %s\(gs_ctx\*" % name, hdr)
    assert hdr.index("---- neighbourhoods") < hdr.index("---- clusters") < hdr.index("Tuning / profiling knobs")
    sec = hdr[hdr.index("---- clusters"):hdr.index("Tuning / profiling knobs")]
    for text in ("d2 = (dx dx + dy dy) + dz dz", "d = p_j - p_i", "r2 = radius * radius", "INCLUSIVE", "smallest", "GS_CLUSTER_NONE", "u32[N]",
                 "DROPPED", "gs_upload_*", "gs_share_splats", "gs_compact", "GS_ERR_CAPACITY", "GS_CLUSTER_MAX_ROUNDS", "GS_ERR_DEVICE_FAULT"):
        assert text in sec, text
    q, info, n = _abi.GsCluster(), _abi.GsClusterInfo(), ctypes.c_uint64()
    calls = {"gs_cluster_label": lambda: L.gs_cluster_label(None, ctypes.byref(q), ctypes.byref(info)),
             "gs_cluster_read": lambda: L.gs_cluster_read(None, None, None, 0, ctypes.byref(n)),
             "gs_state_cluster": lambda: L.gs_state_cluster(None, 0, 1, 1, 0, 0, 1, 2, None),
             "gs_state_cluster_linked": lambda: L.gs_state_cluster_linked(None, 2, 2, 0, 0, 1, 2, None)}
    for name, call in calls.items():
        assert call() == _abi.GS_ERR_INVALID_ARGUMENT
        msg = L.gs_last_error()
        assert (name + ":").encode() in msg and b"null ctx" in msg
    assert gsplat.clusters is clusters
    for fn in ("label", "read", "select", "select_linked", "select_small_clusters", "select_connected", "select_largest_cluster"):
        assert callable(getattr(clusters, fn))
    for cls in (gsplat.Renderer, gsplat.PipelinedRenderer):
        assert not [m for m in dir(cls) if "cluster" in m.lower()]


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def check_labelling(r, key, pos, radius, members=None, filt=(0, 0), many=None):
    """label + read against the restatement, and the info numbers; many: whether the grid must have more than one cell on every
    axis (True), exactly one (False), or either (None).  Returns the info."""
    from gsplat import clusters
    wl, ws = want(key, pos, radius, members)
    info = clusters.label(r, radius, members=filt)
    l, s = clusters.read(r)
    print("%s radius %g: %s" % (key, radius, info))
    assert l.dtype == s.dtype == np.uint32
    assert np.array_equal(l, wl), (key, radius, int((l != wl).sum()))
    assert np.array_equal(s, ws), (key, radius, int((s != ws).sum()))
    assert (info["members"], info["clusters"], info["largest"]) == info_counts(wl, ws), info
    assert 1 <= info["rounds"] <= 64, info
    assert info["candidates"] >= 2 * int((ws > 1).sum()), info  # a member with a link had itself and its partner as candidates
    if many is not None:
        assert (min(info["cells"]) > 1) if many else (info["cells"] == (1, 1, 1)), info
    assert info["cell_edge"] >= 1.001 * radius
    return info


@pytest.mark.gpu
def test_labels_ragged_scene():
    """synth.bicycle_like(3001): almost all singletons, mixed, a giant cluster among a thousand small ones, a mean degree of 268, and
    one cell in which every pair hooks (the contention case)."""
    from gsplat import clusters
    rec = ragged()
    r = _mk(rec, 64, 64, 16)
    l, s = clusters.read(r)  # before any labelling
    assert l.shape == s.shape == (3001,) and (l == NONE).all() and not s.any()
    for radius, (ncl, largest) in RAGGED.items():
        info = check_labelling(r, "ragged", rec, radius, many=radius < 1e3)
        assert (info["members"], info["clusters"], info["largest"]) == (3001, ncl, largest)
    r.destroy()


@pytest.mark.gpu
def test_labels_length_no_multiple():
    """scene(10000)[:9997]: the length is no multiple of 4, 64 or 256."""
    rec = np.ascontiguousarray(scene(10000)[:9997])
    r = _mk(rec, 64, 64, 16)
    info = check_labelling(r, "cfgA9997", rec, 0.25, many=True)
    assert (info["clusters"], info["largest"]) == (4857, 3579)
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "reversed", "permuted"])
def test_long_chain(order):
    """A cluster 4095 links long across about a thousand cells: a propagation that stops early, or a hook that is lost and never
    retried, leaves it in pieces.  Then with the member at k = 2000 hidden and members = visible: two clusters."""
    from gsplat import clusters
    k = chain_orders()[order]
    pos = chain_pos(k)
    r = _mk(records(pos), 64, 64, 16)
    info = check_labelling(r, "chain_" + order, pos, 0.25)
    assert (info["clusters"], info["largest"]) == (1, 4096) and max(info["cells"]) > 900
    info = check_labelling(r, "chain_" + order, pos, BELOW)
    assert (info["clusters"], info["largest"]) == (4096, 1)
    st = np.where(k == 2000, sr.HIDDEN, 0).astype(np.uint8)
    r.write_state(st)
    info = check_labelling(r, "chain_cut_" + order, pos, 0.25, members=st == 0, filt=(sr.HIDDEN, 0))
    assert (info["members"], info["clusters"], info["largest"]) == (4095, 2, 2095)
    l, s = clusters.read(r)
    assert l[k == 2000].tolist() == [NONE] and s[k == 2000].tolist() == [0]
    assert sorted(set(l.tolist())) == sorted([int(np.flatnonzero(k < 2000)[0]), int(np.flatnonzero(k > 2000)[0]), NONE])
    r.destroy()


@pytest.mark.gpu
def test_equality_at_r2():
    """The lattice: links exactly one radius long, across cell borders; at the float below there is none."""
    p = lattice_pos()
    r = _mk(records(p), 64, 64, 16)
    info = check_labelling(r, "lattice", p, 0.25)
    assert (info["clusters"], info["largest"]) == (1, 216)
    info = check_labelling(r, "lattice", p, BELOW)
    assert (info["clusters"], info["largest"]) == (216, 1)
    check_labelling(r, "lattice", p, 0.36)
    r.destroy()


@pytest.mark.gpu
def test_special_floats():
    """NaN, +-inf, -0, a denormal, exact duplicates (of finite and of non-finite splats), with and without a far outlier."""
    from gsplat import clusters
    p = special_pos()
    n = p.shape[0]
    far = np.concatenate([p, np.array([[1e6, 1e6, -1e6]], F)])  # a far outlier coarsens (or is clamped by) the grid
    r, rf = _mk(records(p), 64, 64, 16), _mk(records(far), 64, 64, 16)
    for radius in (0.1, 0.0, 1e-40):
        check_labelling(r, "special", p, radius)
        check_labelling(rf, "special_far", far, radius)
        l, s = clusters.read(r)
        lf, sf = clusters.read(rf)
        assert np.array_equal(lf[:n], l) and np.array_equal(sf[:n], s) and (lf[n], sf[n]) == (n, 1)
        for i in (10, 20, 30, 70, 71):  # non-finite: singletons
            assert (l[i], s[i]) == (i, 1)
    assert (l[60], l[61], s[60]) == (60, 60, 2) and l[80] == l[81] == l[82] == 80 and s[80] == 3 and int((s > 1).sum()) == 5  # radius 0: the duplicates
    r.destroy()
    rf.destroy()
    # nothing but non-finite members: no grid, singletons all the same
    q = np.full((5, 3), np.nan, F)
    r = _mk(records(q), 64, 64, 16)
    info = clusters.label(r, 0.5)
    l, s = clusters.read(r)
    assert l.tolist() == [0, 1, 2, 3, 4] and s.tolist() == [1] * 5 and (info["members"], info["clusters"], info["largest"], info["rounds"]) == (5, 5, 1, 0)
    r.destroy()


@pytest.mark.gpu
def test_filters():
    """Members by a host bit on a pseudo-random half: the clusters are those of the members alone (a removed bridge splits one), the
    others read NONE / 0."""
    from gsplat import clusters
    rec = ragged()
    n = rec.shape[0]
    half = np.random.default_rng(3).integers(0, 2, n).astype(bool)
    st = (half * 4 + np.arange(n) % 2).astype(np.uint8)  # bit 2 is the filter; bit 0 is noise it must ignore
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    for radius in (0.5, 2.0):
        info = check_labelling(r, "ragged_half", rec, radius, members=half, filt=(4, 4))
        l, s = clusters.read(r)
        assert (l[~half] == NONE).all() and not s[~half].any() and info["members"] == int(half.sum())
    al, _ = want("ragged", rec, 0.5)
    wl, _ = want("ragged_half", rec, 0.5, half)
    big = np.flatnonzero((al == np.bincount(al).argmax()) & half)
    assert len(set(wl[big].tolist())) > 1  # at 0.5 the giant cluster of the whole scene falls apart without the other half
    info = clusters.label(r, 0.5, members=(0xFF, 0xEE))  # no member at all
    l, s = clusters.read(r)
    assert (l == NONE).all() and not s.any() and (info["members"], info["clusters"], info["largest"]) == (0, 0, 0)
    np.testing.assert_array_equal(r.read_state(), st)
    r.destroy()
    three = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F)
    r = _mk(records(three), 64, 64, 16)
    assert clusters.label(r, 1.0)["clusters"] == 1
    r.write_state(np.array([0, 1, 0], np.uint8))
    assert clusters.label(r, 1.0, members=(1, 0))["clusters"] == 2
    assert clusters.read(r)[0].tolist() == [0, NONE, 2]
    r.destroy()


@pytest.mark.gpu
def test_determinism_and_placement():
    """Two labellings agree; a slab context, a borrower and a PipelinedRenderer give a fresh whole-canvas context's planes."""
    import gsplat
    from gsplat import _abi, clusters
    rec = ragged()
    wl, ws = want("ragged", rec, 0.5)
    owner = _mk(rec, 64, 64, 16)
    for _ in range(2):
        clusters.label(owner, 0.5)
        l, s = clusters.read(owner)
        assert np.array_equal(l, wl) and np.array_equal(s, ws)
    slab = _mk(rec, 256, 256, 16, cols=SLAB_COLS[16])
    check_labelling(slab, "ragged", rec, 0.5)
    slab.destroy()
    borrower = _mk(rec, 64, 64, 16, share_with=owner)
    l, s = clusters.read(borrower)
    assert (l == NONE).all() and not s.any()  # the borrower keeps its own planes
    check_labelling(borrower, "ragged", rec, 0.3)
    l, s = clusters.read(owner)
    assert np.array_equal(l, wl) and np.array_equal(s, ws)
    borrower.destroy()
    owner.destroy()
    p = gsplat.PipelinedRenderer(gsplat.Canvas(64, 64), None, 0, gsplat.PackedGaussians(rec), 16, frames_in_flight=2, flags=_abi.GS_FLAG_SPLAT_STATE)
    p.render_uniforms(state_scene("ragged")[1])  # in flight when the call comes
    check_labelling(p, "ragged", rec, 0.5)
    assert clusters.select(p, 1, 9) == int((ws <= 9).sum())
    p.destroy()


@pytest.mark.gpu
def test_labelling_disturbs_no_frame():
    """A frame rendered before and after a labelling (and the two selections, changing nothing) is byte-identical in every tap, and
    its statistics are unchanged."""
    from gsplat import clusters
    s, u, W, H = state_scene("ragged")
    a, b = _mk(s, W, H, 8), _mk(s, W, H, 8)
    wl, ws = want("ragged", s, 0.5)
    before = frame_taps(a, u, False)
    frame_taps(b, u, False)
    for _ in range(3):  # three frames in flight on both; no wait: the labelling drains the ring
        a.render_uniforms(u)
        b.render_uniforms(u)
    clusters.label(a, 0.5)
    l, sz = clusters.read(a)
    assert np.array_equal(l, wl) and np.array_equal(sz, ws)
    assert clusters.select(a, 5, 1, op=sr.SET, bits=sr.HIDDEN) == 0  # the empty range
    assert clusters.select_linked(a, op=sr.SET, bits=sr.HIDDEN) == 0  # no seed
    ta, tb = frame_taps(a, u, False), frame_taps(b, u, False)
    for k in ta:
        np.testing.assert_array_equal(ta[k], tb[k], err_msg=k)
        np.testing.assert_array_equal(ta[k], before[k], err_msg=k)
    assert timeless(a.stats()) == timeless(b.stats())
    a.destroy()
    b.destroy()


@pytest.mark.gpu
def test_state_cluster():
    """matched and the plane against the restatement for every op, inside 0 and 1, a where filter and the empty range."""
    from gsplat import clusters
    rec = ragged()
    n = rec.shape[0]
    st = np.random.default_rng(7).integers(0, 256, n).astype(np.uint8)
    mem = (st & 0x40) == 0
    wl, ws = want("ragged_bit6", rec, 0.5, mem)
    r = _mk(rec, 64, 64, 16)
    r.write_state(st)
    clusters.label(r, 0.5, members=(0x40, 0))
    ranges = [(0, 0), (1, 1), (2, 9), (10, NONE), (0, NONE), (4, 1), (int(ws.max()), int(ws.max()))]
    for k, (lo, hi) in enumerate(ranges):
        for inside in (True, False):
            for op in OPS:
                bits = (0x02, 0xA4)[(k + op) % 2]
                where = ((0, 0), (0x0C, 0x04), (0x30, 0x10))[(k + op + int(inside)) % 3]
                r.write_state(st)
                member = cr.member(ws, lo, hi, inside)
                new, matched = sr.apply_region(st, member, op, bits, where)
                cell = (lo, hi, inside, op, bits, where)
                assert clusters.select(r, lo, hi, inside, where, op, bits) == matched, cell
                np.testing.assert_array_equal(r.read_state(), new, err_msg=str(cell))
                if lo > hi:
                    assert member.sum() == (0 if inside else n)
    assert cr.member(ws, 0, 0).sum() == int((~mem).sum()) > 0  # a non-member's 0 takes part
    l, s = clusters.read(r)
    assert np.array_equal(l, wl) and np.array_equal(s, ws)  # the selection only reads the planes
    r.destroy()


@pytest.mark.gpu
def test_state_cluster_linked():
    """One seed per chosen cluster, seeds in no cluster, seeds set after the labelling: states now, labels then."""
    from gsplat import clusters
    rec = ragged()
    n = rec.shape[0]
    rng = np.random.default_rng(11)
    base = (rng.integers(0, 4, n) * 0x10).astype(np.uint8)  # bits 4 and 5: what the where filters read
    mem = np.arange(n) % 7 != 3
    base[~mem] |= sr.HIDDEN
    wl, ws = want("ragged_mod7", rec, 0.5, mem)
    r = _mk(rec, 64, 64, 16)
    r.write_state(base)
    clusters.label(r, 0.5, members=(sr.HIDDEN, 0))
    roots = np.flatnonzero(wl == np.arange(n))
    chosen = roots[rng.permutation(roots.size)[:40]]
    giant = int(np.bincount(wl[mem]).argmax())
    one_each = np.array([rng.choice(np.flatnonzero(wl == c)) for c in list(chosen) + [giant]])  # a seed anywhere in its cluster
    cases = {"one_each": one_each, "non_members": np.flatnonzero(~mem)[:50], "none": np.zeros(0, np.int64),
             "mixed": np.concatenate([one_each[-5:], np.flatnonzero(~mem)[:5]])}
    for name, ids in cases.items():
        for op in OPS:
            for where in ((0, 0), (0x30, 0x10)):
                st = base.copy()
                st[ids] |= sr.SELECTED  # set AFTER the labelling
                r.write_state(st)
                member = cr.linked(wl, (st & sr.SELECTED) != 0)
                new, matched = sr.apply_region(st, member, op, 0x82, where)
                cell = (name, op, where)
                assert clusters.select_linked(r, (sr.SELECTED, sr.SELECTED), where, op, 0x82) == matched, cell
                np.testing.assert_array_equal(r.read_state(), new, err_msg=str(cell))
                if name in ("non_members", "none"):
                    assert matched == 0
                elif where == (0, 0):
                    assert matched == int(np.isin(wl, wl[ids[mem[ids]]]).sum()) > ids.size
    # the seed filter reads the whole byte as it is now: seeds = visible and selected
    st = base.copy()
    st[one_each[0]] |= sr.SELECTED
    st[np.flatnonzero(~mem)[0]] |= sr.SELECTED
    r.write_state(st)
    assert clusters.select_linked(r, (sr.SELECTED | sr.HIDDEN, sr.SELECTED), op=sr.SET, bits=0x80) == int(ws[one_each[0]])
    l, s = clusters.read(r)
    assert np.array_equal(l, wl) and np.array_equal(s, ws)
    r.destroy()


@pytest.mark.gpu
def test_verbs():
    from gsplat import clusters
    rec = ragged()
    n = rec.shape[0]
    wl, ws = want("ragged", rec, 0.5)
    r = _mk(rec, 64, 64, 16)
    # the largest cluster
    assert clusters.select_largest_cluster(r, 0.5) == 1711
    np.testing.assert_array_equal(r.read_state(), np.where(ws == 1711, sr.SELECTED, 0).astype(np.uint8))
    # the whole clusters a selection touches, among the visible splats
    hidden = np.arange(n) % 7 == 3
    hl, hs = want("ragged_mod7", rec, 0.5, ~hidden)
    inside = sr.member(sr.SPHERE, rec, 64, 64, a=(0, 0, 0), b=(1.0, 0, 0))
    st = np.where(hidden, sr.HIDDEN, 0).astype(np.uint8)
    st[inside] |= sr.SELECTED  # hidden ones too: they seed nothing
    r.write_state(st)
    touched = cr.linked(hl, inside & ~hidden)
    assert clusters.select_connected(r, 0.5) == int(touched.sum()) > int((inside & ~hidden).sum()) > 0
    np.testing.assert_array_equal(r.read_state(), np.where(touched, st | sr.SELECTED, st).astype(np.uint8))
    # islands of at most 9 splats, hidden and deleted: the restatement's survivors, in order
    r.write_state(np.zeros(n, np.uint8))
    small = ws <= 9
    assert clusters.select_small_clusters(r, 0.5, 9) == int(small.sum()) > 1000
    np.testing.assert_array_equal(r.read_state(), np.where(small, sr.SELECTED, 0).astype(np.uint8))
    assert r.hide_selected() == int(small.sum())
    kept = r.delete_hidden()
    assert np.array_equal(kept, np.flatnonzero(~small))
    assert np.array_equal(r.export_splats()[:, 0:3], rec[~small][:, 0:3])
    # ... and what is left consists of the clusters above 9, relabelled in the new indices
    info = clusters.label(r, 0.5)
    l, s = clusters.read(r)
    assert np.array_equal(s, ws[~small]) and info["clusters"] == int(((wl == np.arange(n)) & ~small).sum())
    assert np.array_equal(l, np.searchsorted(np.flatnonzero(~small), wl[~small]))
    r.destroy()


@pytest.mark.gpu
def test_lifecycle():
    """NONE / 0 before any labelling and after upload, compact and share_splats; state calls, a transform and a frame leave the planes."""
    from gsplat import _abi, clusters
    s, u, W, H = state_scene("ragged")
    n = s.shape[0]
    wl, ws = want("ragged", s, 0.5)

    def initial(r, m):
        l, sz = clusters.read(r)
        return l.shape == sz.shape == (m,) and bool((l == NONE).all()) and not sz.any()

    def labelled(r):
        l, sz = clusters.read(r)
        return np.array_equal(l, wl) and np.array_equal(sz, ws)

    r = _mk(s, W, H, 8)
    other = _mk(np.ascontiguousarray(s[:1500]), W, H, 8)
    assert initial(r, n)
    clusters.label(r, 0.5)
    assert labelled(r)
    assert r.select_sphere((0, 0, 0), 1.5) > 100
    r.translate_selected((0.3, -0.2, 0.1))
    r.hide_selected()
    r.render_uniforms(u)
    r.wait()
    assert labelled(r)  # they describe the positions and states at the time of the labelling
    st = (np.arange(n) % 3 == 0).astype(np.uint8) * 4
    r.write_state(st)
    kept = r.compact(4, 4)
    assert initial(r, kept.size)
    moved = r.export_splats()
    info = clusters.label(r, 0.5)
    ml, ms = cr.components(moved, 0.5)
    l, sz = clusters.read(r)
    assert np.array_equal(l, ml) and np.array_equal(sz, ms) and info["clusters"] == int((ml == np.arange(kept.size)).sum())
    arr = np.ascontiguousarray(s[:2000])
    _abi.check(r._L.gs_upload_splats(r._ctx, arr.ctypes.data, 2000))
    assert initial(r, 2000)
    clusters.label(r, 0.5)
    assert not initial(r, 2000)
    _abi.check(r._L.gs_share_splats(r._ctx, other._ctx))
    assert initial(r, 1500)
    r.destroy()
    other.destroy()


@pytest.mark.gpu
def test_budget():
    """max_candidates = 1 at radius 1e3 is refused with GS_ERR_CAPACITY, the message carries both numbers, info is filled and the
    planes still hold the previous labelling; the exact budget accepts the call."""
    from gsplat import _abi, clusters
    rec = ragged()
    wl, ws = want("ragged", rec, 0.5)
    r = _mk(rec, 64, 64, 16)
    clusters.label(r, 0.5)
    L = r._L
    q, info = _abi.GsCluster(), _abi.GsClusterInfo()
    q.struct_size, q.radius, q.max_candidates = ctypes.sizeof(q), 1e3, 1
    assert L.gs_cluster_label(r._ctx, ctypes.byref(q), ctypes.byref(info)) == _abi.GS_ERR_CAPACITY
    msg = L.gs_last_error().decode()
    assert info.candidates == 3001 * 3001 and info.members == 3001 and tuple(info.cells) == (1, 1, 1) and info.cell_edge >= 1001.0
    assert "gs_cluster_label" in msg and str(3001 * 3001) in msg and "max_candidates = 1 " in msg + " ", msg
    l, s = clusters.read(r)
    assert np.array_equal(l, wl) and np.array_equal(s, ws)  # the planes are left as they were
    code, msg = code_of(lambda: clusters.label(r, 1e3, max_candidates=3001 * 3001 - 1))
    assert code == _abi.GS_ERR_CAPACITY and str(3001 * 3001) in msg and str(3001 * 3001 - 1) in msg
    assert clusters.label(r, 1e3, max_candidates=3001 * 3001)["clusters"] == 1
    r.destroy()


@pytest.mark.gpu
def test_cluster_refusals():
    from gsplat import _abi, clusters
    L = _abi.load()
    INV = _abi.GS_ERR_INVALID_ARGUMENT
    rec = ragged()
    n = rec.shape[0]
    info, nn, m = _abi.GsClusterInfo(), ctypes.c_uint64(), ctypes.c_uint64(77)

    def query(**kw):
        q = _abi.GsCluster()
        q.struct_size, q.radius = ctypes.sizeof(_abi.GsCluster), 0.5
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    # before any upload: GS_ERR_NO_SCENE; N == 0: zero results, GS_OK
    cfg = _abi.GsConfig()
    cfg.struct_size, cfg.width, cfg.height, cfg.tile_size, cfg.flags = ctypes.sizeof(_abi.GsConfig), 64, 64, 16, _abi.GS_FLAG_SPLAT_STATE
    ctx = ctypes.c_void_p()
    _abi.check(L.gs_create(ctypes.byref(cfg), ctypes.byref(ctx)))
    q = query()
    assert L.gs_cluster_label(ctx, ctypes.byref(q), ctypes.byref(info)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_cluster_read(ctx, None, None, 0, ctypes.byref(nn)) == _abi.GS_ERR_NO_SCENE
    assert L.gs_state_cluster(ctx, 0, 1, 1, 0, 0, 1, 2, None) == _abi.GS_ERR_NO_SCENE
    assert L.gs_state_cluster_linked(ctx, 2, 2, 0, 0, 1, 2, None) == _abi.GS_ERR_NO_SCENE
    _abi.check(L.gs_upload_splats(ctx, None, 0))
    info.members = info.candidates = 9
    _abi.check(L.gs_cluster_label(ctx, ctypes.byref(q), ctypes.byref(info)))
    assert (info.members, info.clusters, info.largest, info.candidates, info.rounds) == (0, 0, 0, 0, 0)
    _abi.check(L.gs_cluster_label(ctx, ctypes.byref(q), None))
    nn.value = 9
    _abi.check(L.gs_cluster_read(ctx, None, None, 0, ctypes.byref(nn)))
    assert nn.value == 0
    _abi.check(L.gs_state_cluster(ctx, 0, 1, 1, 0, 0, 1, 2, ctypes.byref(m)))
    assert m.value == 0
    m.value = 77
    _abi.check(L.gs_state_cluster_linked(ctx, 2, 2, 0, 0, 1, 2, ctypes.byref(m)))
    assert m.value == 0
    L.gs_destroy(ctx)

    r = _mk(rec, 64, 64, 16)
    st = (np.arange(n) % 5).astype(np.uint8)
    r.write_state(st)
    clusters.label(r, 0.5)
    wl, ws = want("ragged", rec, 0.5)

    def refused(name, call, *fragments, code=INV):
        assert call() == code, name
        msg = L.gs_last_error().decode()
        assert name + ":" in msg and all(f in msg for f in fragments), msg
        l, s = clusters.read(r)
        assert np.array_equal(l, wl) and np.array_equal(s, ws)
        np.testing.assert_array_equal(r.read_state(), st)

    lab = lambda q: (lambda: L.gs_cluster_label(r._ctx, ctypes.byref(q) if q is not None else None, ctypes.byref(info)))
    refused("gs_cluster_label", lab(None), "null query")
    refused("gs_cluster_label", lab(query(struct_size=40)), "struct_size 40")
    refused("gs_cluster_label", lab(query(radius=float("nan"))), "radius nan")
    refused("gs_cluster_label", lab(query(radius=float("inf"))), "radius inf")
    refused("gs_cluster_label", lab(query(radius=-0.5)), "radius -0.5")
    refused("gs_cluster_label", lab(query(radius=2e19)), "radius 2e+19", "squared")
    refused("gs_cluster_label", lab(query(reserved=(ctypes.c_uint32 * 2)(5, 0))), "reserved[0] = 5")
    refused("gs_cluster_label", lab(query(reserved=(ctypes.c_uint32 * 2)(0, 6))), "reserved[1] = 6")
    refused("gs_cluster_label", lab(query(mask=0x100)), "0x100", "does not fit the state byte")
    refused("gs_cluster_label", lab(query(value=0x1FF)), "0x1ff", "does not fit the state byte")
    # the read's conventions are gs_neigh_read's
    refused("gs_cluster_read", lambda: L.gs_cluster_read(r._ctx, None, None, 0, None), "null n")
    a, b = np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, 0xA5A5A5A5, np.uint32)
    refused("gs_cluster_read", lambda: L.gs_cluster_read(r._ctx, a.ctypes.data, b.ctypes.data, n - 1, ctypes.byref(nn)), "%d words per plane needed" % n)
    assert nn.value == n and (a == 0xA5A5A5A5).all() and (b == 0xA5A5A5A5).all()
    _abi.check(L.gs_cluster_read(r._ctx, a.ctypes.data, None, n, ctypes.byref(nn)))  # either plane alone
    assert np.array_equal(a, wl) and (b == 0xA5A5A5A5).all()
    _abi.check(L.gs_cluster_read(r._ctx, None, b.ctypes.data, n, ctypes.byref(nn)))
    assert np.array_equal(b, ws)
    # the state calls' own: nothing is applied
    sel = lambda op, bits, wm=0: (lambda: L.gs_state_cluster(r._ctx, 0, 5, 1, wm, 0, op, bits, ctypes.byref(m)))
    lnk = lambda op, bits, sm=2, wm=0: (lambda: L.gs_state_cluster_linked(r._ctx, sm, 2, wm, 0, op, bits, ctypes.byref(m)))
    m.value = 77
    refused("gs_state_cluster", sel(0, 2), "unknown op 0")
    refused("gs_state_cluster", sel(5, 2), "unknown op 5")
    refused("gs_state_cluster", sel(1, 0x100), "0x100")
    refused("gs_state_cluster", sel(1, 2, 0x100), "where_mask 0x100")
    refused("gs_state_cluster_linked", lnk(0, 2), "unknown op 0")
    refused("gs_state_cluster_linked", lnk(5, 2), "unknown op 5")
    refused("gs_state_cluster_linked", lnk(1, 0x100), "0x100")
    refused("gs_state_cluster_linked", lnk(1, 2, sm=0x100), "seed_mask 0x100")
    refused("gs_state_cluster_linked", lnk(1, 2, wm=0x100), "where_mask 0x100")
    assert m.value == 77
    r.destroy()
    # a context without the state plane: (0, 0) works, any other filter and the two state calls are refused
    q = mk(rec, 64, 64, 16)
    check_labelling(q, "ragged", rec, 0.5)
    for fn in (lambda: clusters.label(q, 0.5, members=(1, 0)), lambda: clusters.select(q, 0, 1), lambda: clusters.select_linked(q)):
        code, msg = code_of(fn)
        assert code == INV and "GS_FLAG_SPLAT_STATE" in msg
    l, s = clusters.read(q)
    assert np.array_equal(l, wl) and np.array_equal(s, ws)
    q.destroy()
