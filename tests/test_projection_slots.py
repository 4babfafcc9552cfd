"""The tight projection (k_preprocess.hip, gs_preprocess_kernel<TIGHT = true, NB, STATE>) at its hand-written boundaries: trips of 256
survivors, the per-wave slot loop's batches of 64 with its marks, running maximum and carry, the packed LDS words at their maxima,
the two sharded bump cursors with their fit test and the regrow decision of gs_wait, and the entries of the units of a workgroup.

The other boundary suites lay their scenes out by depth-sorted slot position; here the RECORD ORDER is the subject: survivor v of a
workgroup (index order, culled splats skipped) is lane v % 64 of wave (v / 64) % 4 of trip v / 256.  Scenes are sequences of
row_scenes' splats in three classes whose cull outcome is unambiguous by construction: SURV (centred inside the canvas, with slots),
FAINT (centred inside the canvas, opacity logit -9: survives the cull, 0 slots) and CULLED (centred at ndc x >= 5).  proj_restate
restates the bookkeeping from the dump's slots per splat and these classes.  "Wave 0" is trip 0, wave 0 of workgroup 0; the other
waves hold dots.

Every scene has an unmarked test that asserts, from proj_restate, that the scene reaches the boundary its name says, and that the
restated owner computation with a switch turned (no carry, <= in the mark test, marks of survivors without slots) DISAGREES with the
direct one where the scene is named for it: the proof, on the CPU alone, that the scene discriminates.  The gpu test renders the
scene on the product path with GS_FLAG_EXACT_BLEND, on the default grid and with GS_OPT_PERSISTENT_GRID 4, and asserts the frame's
slot, item and instance counts with equality, the lists through gpu_checks.check_product_lists and the image bit for bit.  Nothing
here has a tolerance.

A survivor with slots all of whose items are holes (a GHOST) is built, not searched for: the dump leaves such a gaussian out, as
the frame's slot count does, so its slots are read off a twin inside the canvas (ghost_pair).
A one-column slab of a two-column canvas launches the 4-chunk kernel (gs_preprocess_prepare: 8 below 30 % of the canvas), so the
slab case restates NB = 4.
"""
import numpy as np
import pytest

import proj_restate as pr
import rows_restate as rr
import state_restate as sr
from gpu_checks import check_image, check_product_lists
from row_scenes import (FLOOR, LONG_CANVAS, POST_CANVAS, _rng, blankets, dots, frame_of, frames, model_of, params, per_splat, post, scene,
                        tight_check)
from support import cached, mk, oracle_frame, pinhole

SURV, FAINT, CULLED, GHOST = 0, 1, 2, 3
FIT_CANVAS = (16, 512, 8)   # posts of 64 slots
DOT_CANVAS = (192, 144, 16)
K = 40                      # slots of the short post (20 items, 20 aliased holes)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
class Seq:
    """Splats in record order with their classes."""

    def __init__(self, canvas, rng, col=None):
        self.W, self.H, self.ts = canvas
        self.rng, self.col, self.P, self.cls = rng, col, [], []

    def add(self, P, cls=SURV, times=1):
        for _ in range(times):
            self.P.append(P)
            self.cls.append(np.full(P.shape[0], cls))
        return self

    def _dots(self, k):
        ntx, nty = self.W // self.ts, self.H // self.ts
        tx = self.rng.integers(0, ntx, k) if self.col is None else np.full(k, self.col)
        return dots(self.ts, tx, self.rng.integers(0, nty, k), self.rng)

    def dots(self, k):
        return self.add(self._dots(k))

    def faint(self, k):
        P = self._dots(k)
        P[:, 5] = -9.0  # sigmoid(-9) = 1.2e-4 < 1/255
        return self.add(P, FAINT)

    def culled(self, k):
        P = self._dots(k)
        P[:, 0] = 3.0 * self.W + self.rng.uniform(0.0, self.W, k)  # ndc x = 5 .. 7
        return self.add(P, CULLED)

    def fill(self, to):
        """Dots up to `to` splats."""
        return self.dots(to - sum(p.shape[0] for p in self.P))

    def permuted(self, first, count):
        """Shuffles splats first .. first + count - 1."""
        P, cls = np.concatenate(self.P), np.concatenate(self.cls)
        o = first + self.rng.permutation(count)
        P[first:first + count], cls[first:first + count] = P[o], cls[o]
        self.P, self.cls = [P], [cls]
        return self

    def scene(self, name, cols=None, **want):
        sc = scene("proj_" + name, self.W, self.H, self.ts, np.concatenate(self.P), cols=cols, **want)
        sc["cls"] = np.concatenate(self.cls)
        return sc


def short_post(canvas=POST_CANVAS, slots=K):
    return post(*canvas, lambda r: r[0] == slots and r[1] == slots // 2)


def long_post():
    return post(*LONG_CANVAS, lambda r: r[0] >= 200 and r[1] >= 50)


def slots_per_splat(sc, hidden=None):
    """Slots of every splat from the dump (through the rows model of the scene), checked against the classes."""
    m = model_of(sc)
    ns = np.zeros(sc["P"].shape[0], np.int64)
    ns[m["order"]] = m["nslots"]
    assert (ns[sc["cls"] != SURV] == 0).all() and (ns[sc["cls"] == SURV] > 0).all()
    if (sc["cls"] == GHOST).any():  # (no slot of a ghost is in the dump: see ghost_pair)
        ns[sc["cls"] == GHOST] = int(per_splat(ghost_pair()[1], sc["W"], sc["H"], sc["ts"])[0, 0])
    if hidden is not None:
        ns[hidden] = 0
    return ns


def pm(sc, NB=2, hidden=None):
    culled = sc["cls"] == CULLED
    return pr.model(slots_per_splat(sc, hidden), culled if hidden is None else culled | hidden, NB)


def owners_agree(p):
    """The kernel's owner computation gives the direct one in every trip of every workgroup."""
    for g in p["wg"]:
        for t in range(g["trips"]):
            if g["R"][t]:
                direct, (kern, _) = pr.owners_direct(g["ns"][t]), pr.owners_kernel(g["ns"][t])
                assert all((a == b).all() for a, b in zip(direct, kern))
        np.testing.assert_array_equal(g["entry"], g["entry_direct"])
    return True


def differs(ns, **switch):
    direct, (kern, _) = pr.owners_direct(ns), pr.owners_kernel(ns, **switch)
    return any((a != b).any() for a, b in zip(direct, kern))


# a. wave slot totals
WAVE_TOTALS = (1, 63, 64, 65, 127, 128, 129)


def total_scene(Rw):
    """Workgroup 0, all 1024 survive: wave 0 holds one post (40 slots below 100, else 72), dots and faint splats adding up to Rw, shuffled
    (Rw = 1: one dot among 63 faint); wave 1 dots, wave 2 faint (Rw = 0), wave 3 dots; trip 1 all faint (R = 0); trips 2 and 3 dots."""
    def make():
        q = Seq(POST_CANVAS, _rng(20, Rw))
        if Rw == 1:
            q.dots(1).faint(63)
            nd = 1
        else:
            ps = K if Rw < 100 else 72
            nd = Rw - ps
            q.add(short_post(slots=ps)[0]).dots(nd).faint(63 - nd)
            nd += 1
        q.permuted(0, 64).dots(64).faint(64).dots(64).faint(256).dots(512)
        return q.scene("total_%d" % Rw, Rw=Rw, C=nd)
    return cached(("proj_total_scene", Rw), make)


@pytest.mark.parametrize("Rw", WAVE_TOTALS)
def test_wave_total_scenes(Rw):
    sc = total_scene(Rw)
    p = pm(sc)
    g = p["wg"][0]
    assert p["workgroups"] == 1 and g["nvis"] == 1024 and g["trips"] == 4
    assert g["Rw"][0, 0] == Rw and g["Cw"][0, 0] == sc["want"]["C"] and g["word"][0, 0] == Rw | (sc["want"]["C"] << 16)
    assert -(-Rw // 64) == {1: 1, 63: 1, 64: 1, 65: 2, 127: 2, 128: 2, 129: 3}[Rw]  # batches of wave 0
    assert list(g["Rw"][0, 1:]) == [64, 0, 64] and list(g["Cw"][0, 1:]) == [64, 0, 64]  # a wave without slots between two with
    assert g["R"][1] == 0 and g["C"][1] == 0 and g["R"][0] == Rw + 128 and list(g["R"][2:]) == [256, 256]  # a trip without a bump
    assert p["shard_rows"][0] == Rw + 128 + 512 and p["shard_recs"][0] == sc["want"]["C"] + 128 + 512
    assert owners_agree(p)


# b. one owner across a batch boundary
STRADDLE = {"x0": False, "x23": False, "x24": False, "x25": True, "x44": True, "x63": True, "two_posts": True, "three_posts": True, "start_64": False}


def straddle_scene(name):
    """Wave 0: X dots, the 40-slot post, dots (x*); post, post (the second one straddles); three posts (the third starts in the second
    batch); 24 dots, post, post (the second one starts at position 64)."""
    def make():
        q = Seq(POST_CANVAS, _rng(21, len(name), sum(map(ord, name))))
        pk = short_post()[0]
        if name[0] == "x":
            q.dots(int(name[1:])).add(pk)
        elif name == "start_64":
            q.dots(24).add(pk, times=2)
        else:
            q.add(pk, times=2 if name == "two_posts" else 3)
        return q.fill(256).scene("straddle_" + name)
    return cached(("proj_straddle_scene", name), make)


@pytest.mark.parametrize("name", list(STRADDLE))
def test_straddle_scenes(name):
    p = pm(straddle_scene(name))
    g = p["wg"][0]
    ns, rp = g["ns"][0, 0], g["myrp"][0, 0]
    posts = np.flatnonzero(ns == K)
    first = {"two_posts": [0, 40], "three_posts": [0, 40, 80], "start_64": [24, 64]}.get(name) or [int(name[1:])]
    assert list(rp[posts]) == first and (ns[ns != K] == 1).all() and g["nvis"] == 256 and (g["Rw"][0, 1:] == 64).all()
    if name[0] == "x":
        assert posts[0] == int(name[1:])  # the post's lane: x63 makes it lane 63, its first slot the batch's last
    last = first[-1] + K - 1
    assert {"x23": last == 62, "x24": last == 63, "x25": last == 64, "x44": first[0] + K // 2 == 64, "x63": first[0] == 63}.get(name, True)
    straddles = any(f // 64 != (f + K - 1) // 64 for f in first)
    assert straddles == STRADDLE[name]
    assert owners_agree(p)
    assert differs(g["ns"][0], carry=False) == straddles  # without the carry the slots beyond the boundary have no owner
    if name == "start_64":
        assert differs(g["ns"][0], strict=False)  # <= stores the mark of position 64 in the next wave's word 0 as well


# c. batches with no mark
MARKLESS = ("x1", "x40", "lane0", "lane63")


def markless_scene(name, col=None, cols=None, tag=""):
    """Wave 0: X dots, a long post, 5 dots, a second long post, dots (x1, x40); the same from lane 0; 63 dots and the long post in
    lane 63."""
    def make():
        q = Seq(LONG_CANVAS, _rng(22, len(name), sum(map(ord, name))), col)
        pl = long_post()[0]
        if name == "lane63":
            q.dots(63).add(pl)
        else:
            q.dots({"x1": 1, "x40": 40, "lane0": 0}[name]).add(pl).dots(5).add(pl)
        return q.fill(256).scene("markless_" + name + tag, cols=cols)
    return cached(("proj_markless_scene", name, tag), make)


def check_markless(p, name):
    g = p["wg"][0]
    ns, rp = g["ns"][0, 0], g["myrp"][0, 0]
    N = int(ns.max())
    lanes = np.flatnonzero(ns == N)
    assert N >= 200 and list(lanes) == {"x1": [1, 7], "x40": [40, 46], "lane0": [0, 6], "lane63": [63]}[name]
    batches = -(-int(g["Rw"][0, 0]) // 64)
    marked = np.unique(rp[ns > 0] // 64)
    want = batches - marked.size
    for l in lanes:  # at least two consecutive whole batches inside every long post
        assert (int(rp[l]) + N) // 64 - (int(rp[l]) // 64 + 1) >= 2
    _, markless = pr.owners_kernel(g["ns"][0])
    assert markless[0] == want >= 2 * lanes.size and markless[1:] == [0, 0, 0]
    assert owners_agree(p) and differs(g["ns"][0], carry=False)


@pytest.mark.parametrize("name", MARKLESS)
def test_markless_scenes(name):
    sc = markless_scene(name)
    assert long_post()[1][1] >= 50  # items of the long post
    check_markless(pm(sc), name)


# d. survivors without slots in every position
def faint_scene():
    """Wave 0: faint, 3 dots, long post, faint (the lane right after the post's), 2 dots, long post, 10 faint, long post, 43 dots,
    faint (lane 63)."""
    def make():
        q = Seq(LONG_CANVAS, _rng(23))
        pl = long_post()[0]
        q.faint(1).dots(3).add(pl).faint(1).dots(2).add(pl).faint(10).add(pl).dots(43).faint(1)
        return q.fill(256).scene("faint")
    return cached("proj_faint_scene", make)


def test_faint_scene():
    sc = faint_scene()
    p = pm(sc)
    g = p["wg"][0]
    ns, rp = g["ns"][0, 0], g["myrp"][0, 0]
    cls = sc["cls"][:64]
    assert list(np.flatnonzero(cls == FAINT)) == [0, 5] + list(range(9, 19)) + [63] and (ns[cls == FAINT] == 0).all()
    assert ns[4] == ns[8] == ns[19] >= 200
    assert g["Cw"][0, 0] == 64 - 13 and g["C"][0] == 256 - 13 and p["shard_recs"][0] == 256 - 13  # no record slot for a faint one
    assert (rp[9:19] == rp[19]).all() and rp[5] == rp[6]  # would they mark, the faint lanes would mark their successor's first slot
    assert owners_agree(p) and differs(g["ns"][0], empty_marks=True)


# e. a survivor whose items are all holes
GHOST_CANVAS = (512, 512, 8)


def ghost_pair():
    """(ghost, twin, slots): a thin vertical splat centred 20 px LEFT of the 512 x 512 canvas (ndc x = -1.078: inside the cull's 1.1;
    its alpha >= 1/255 ellipse is 2 px wide) and the same splat moved 40.3 px to the right.  The ghost's rect is clamped into the
    canvas and tight_rows, which looks at the vertical extent alone, leaves it the rows of its height: it has slots, and every one
    is a hole.  The dump, like the frame's slot count, leaves such a gaussian out, so its slots are read off the twin: the two differ
    in gx alone, which neither the rect's rows nor tight_rows reads, and neither reaches the aliased column."""
    ghost = params(-20.0, 256.3, FLOOR, 30.0, 0.0, 1.0)
    twin = params(20.3, 256.3, FLOOR, 30.0, 0.0, 1.0)
    return ghost, twin


def ghost_scene():
    """Wave 0: ghost, 20 dots, twin, 10 dots, ghost, 30 dots, ghost (lanes 0, 32 and 63)."""
    def make():
        q = Seq(GHOST_CANVAS, _rng(24))
        ghost, twin = ghost_pair()
        q.add(ghost, GHOST).dots(20).add(twin).dots(10).add(ghost, GHOST).dots(30).add(ghost, GHOST)
        return q.fill(256).scene("ghosts")
    return cached("proj_ghost_scene", make)


def test_ghost_scene():
    from oracle import gs_oracle
    W, H, ts = GHOST_CANVAS
    ghost, twin = ghost_pair()
    sh = per_splat(np.concatenate([ghost, twin]), W, H, ts)
    N = int(sh[1, 0])
    assert list(sh[0]) == [0, 0, 0, 0, 0] and list(sh[1, :3]) == [N, N, N] and N >= 10  # the twin: one one-tile item per row
    sc = ghost_scene()
    s, u = frame_of(sc)
    gd, cnt = gs_oracle.preprocess(s, u, W, H, ts)
    gh = np.flatnonzero(sc["cls"] == GHOST)
    assert list(gh) == [0, 32, 63] and (cnt[gh] > 0).all() and (gd[gh, 14] <= W // ts).all()  # survives the cull with a rect, not aliased
    assert (gd[gh, 13] == gd[21, 13]).all() and (gd[gh, 15] == gd[21, 15]).all()  # the rect's rows are the twin's
    assert gd[0, 11].view(np.float32) > 0.5  # not faint
    p = pm(sc)
    g = p["wg"][0]
    assert list(g["ns"][0, 0][[0, 21, 32, 63]]) == [N] * 4 and g["Cw"][0, 0] == 64  # a record slot each
    assert g["R"][0] == model_of(sc)["S"] + 3 * N  # the cursor hands out the ghosts' slots; the frame's slot count leaves them out
    assert owners_agree(p)


# f. the packed words at their maxima
def maxima_scene(name):
    """wave: 64 blankets as wave 0, 192 dots.  trip: 256 blankets as trip 0, 64 dots as trip 1."""
    def make():
        W, H, ts = LONG_CANVAS
        q = Seq(LONG_CANVAS, _rng(25, len(name)))
        q.add(blankets(W, H, 64 if name == "wave" else 256)).dots(192 if name == "wave" else 64)
        return q.scene("maxima_" + name)
    return cached(("proj_maxima_scene", name), make)


def check_maxima(p, name):
    g = p["wg"][0]
    cap = pr.shard_cap(pr.FRESH_ROWS)
    if name == "wave":
        assert g["Rw"][0, 0] == 32640 == 64 * pr.MAX_SLOTS and g["Cw"][0, 0] == 64 and g["word"][0, 0] == 32640 | (64 << 16)
        assert g["word"][0, 0] >> 16 == 64 and g["word"][0, 0] & 0xFFFF == 32640  # neither field reaches into the other
        assert g["R"][0] == 32640 + 192 < cap
    else:
        assert (g["Rw"][0] == 32640).all() and (g["Cw"][0] == 64).all() and g["R"][0] == 130560 > cap and g["R"][1] == 64
    assert owners_agree(p)


@pytest.mark.parametrize("name", ["wave", "trip"])
def test_maxima_scenes(name):
    sc = maxima_scene(name)
    W, H, ts = LONG_CANVAS
    sl, _ = tight_check.dump(*frame_of(sc), W, H, ts)
    b = sl[sl[:, 0] == 0].astype(np.int64)  # the first blanket: 255 rows' slots, then the aliased column's slots of the same rows
    assert b.shape[0] == 510 and list(b[:255, 2]) == list(range(255)) and list(b[255:509, 2]) == list(range(1, 255))  # nrows = 255, aliased (bit 31 of cw): tile (row + 1, 0)
    assert (b[:255, 4] == 2).all() and (b[255:509, 4] == 1).all() and b[509, 4] == 0  # 510 slots, 509 items, 764 instances
    check_maxima(pm(sc), name)


# g. trips
NVIS_2 = (1, 255, 256, 257, 511, 512, 513, 1023, 1024)
NVIS_8 = (3841, 4095, 4096)


def trips_scene(nvis, NB):
    """One workgroup of 512 NB splats: nvis survivors at random indices (dots; the LAST one a long post, which the idle lanes of the
    last trip replay), culled splats in between."""
    def make():
        n = 512 * NB
        rng = _rng(26, nvis, NB)
        keep = np.zeros(n, bool)
        keep[rng.permutation(n)[:nvis]] = True
        q = Seq(LONG_CANVAS, rng)
        q.dots(n)
        P, cls = q.P[0], q.cls[0]
        out = q.culled(n).P[1]
        P[~keep], cls[~keep] = out[~keep], CULLED
        P[np.flatnonzero(keep)[-1]] = long_post()[0][0]
        q.P, q.cls = [P], [cls]
        return q.scene("trips_%d_nb%d" % (nvis, NB))
    return cached(("proj_trips_scene", nvis, NB), make)


@pytest.mark.parametrize("nvis,NB", [(v, 2) for v in NVIS_2] + [(v, 8) for v in NVIS_8])
def test_trips_scenes(nvis, NB):
    sc = trips_scene(nvis, NB)
    p = pm(sc, NB)
    g = p["wg"][0]
    assert p["workgroups"] == 1 and g["nvis"] == nvis and g["trips"] == -(-nvis // 256)
    assert int(g["valid"][-1].sum()) == (nvis - 1) % 256 + 1
    if NB == 8:
        assert g["trips"] == 16 and int(g["valid"][-1].sum()) == {3841: 1, 4095: 255, 4096: 256}[nvis]
    flat = g["ns"].reshape(-1)
    assert flat[nvis - 1] >= 200 and (flat[:nvis - 1] == 1).all() and (flat[nvis:] == 0).all()
    if nvis < 512 * NB:
        assert (g["survivors"] != np.arange(nvis)).any()  # list position != index
    assert p["unit_n"].sum() == nvis and (p["unit_n"] > 0).all() and owners_agree(p)


# h. units inside a workgroup
GU = 1024
UNIT_KINDS = "FEMF" "EEEM" "MEEE" "EFFE" "TETT" "TEET" "M"  # at 8 chunks one workgroup per group of four; the last workgroup is short
THIN = (50, 10, 30, 70, 80)  # survivors of the thin units, in order


def unit_scene():
    """Units that are full (F), empty (E), mixed (M: 40 % visible, as test_gsort_dense._unit_scene makes them) or thin (T: the
    survivors THIN names, at random indices), under support.pinhole: visible iff z > 0.  A mixed unit has about 410 survivors and a
    full one 1024 = four whole trips, so of the plan's four workgroups only (F, E, M, F) lets two units share a trip and a wave (M's
    tail and F's head), and none does so across an empty unit.  The thin workgroups do: in (T, E, T, T) = (50, 0, 10, 30) wave 0
    holds survivors of three units, in (T, E, E, T) = (70, 0, 0, 80) wave 1 holds the last 6 of the first and 58 of the fourth."""
    def make():
        from test_gsort_dense import _small
        n = (len(UNIT_KINDS) - 1) * GU + 300
        rng = np.random.Generator(np.random.Philox(key=[977, 61]))
        z = rng.uniform(1.0, 6.0, n)
        thin = iter(THIN)
        for k, kind in enumerate(UNIT_KINDS):
            sl = slice(k * GU, min((k + 1) * GU, n))
            if kind == "T":
                keep = np.zeros(GU, bool)
                keep[rng.permutation(GU)[:next(thin)]] = True
                z[sl] *= np.where(keep, 1.0, -1.0)
            elif kind != "F":
                z[sl] *= np.where(rng.random(z[sl].size) < {"E": 0.0, "M": 0.4}[kind], 1.0, -1.0)
        return _small(z, 62), z
    return cached("proj_unit_scene", make)


def test_unit_scene():
    from test_gsort_dense import H, TS, W
    s, z = unit_scene()
    sl, _ = tight_check.dump(s, pinhole(W, H), W, H, TS)
    ns = np.bincount(sl[:, 0].astype(np.int64), minlength=z.size)
    assert (ns[z < 0] == 0).all() and z.size <= 35000
    for NB in (4, 8):
        p = pr.model(ns, z < 0, NB)
        assert owners_agree(p)
        for k, kind in enumerate(UNIT_KINDS):
            c, size = p["unit_n"][k], min(GU, z.size - k * GU)
            assert c == size if kind == "F" else c == 0 if kind == "E" else 0 < c < size
        assert p["wg"][-1]["survivors"].size and z.size % (512 * NB)  # the last workgroup is short
    wgs = p["wg"]  # NB = 8
    assert ["".join(UNIT_KINDS[4 * b:4 * b + 4]) for b in range(6)] == ["FEMF", "EEEM", "MEEE", "EFFE", "TETT", "TEET"] and len(wgs) == 7
    per_wave = lambda g: [list(np.unique(g["unit"][v:v + 64]) - g["unit"][0] // 4 * 4) for v in range(0, g["nvis"], 64)]
    per_trip = lambda g: [list(np.unique(g["unit"][v:v + 256]) - g["unit"][0] // 4 * 4) for v in range(0, g["nvis"], 256)]
    assert [2, 3] in per_wave(wgs[0]) and [2, 3] in per_trip(wgs[0])  # (F, E, M, F): M's tail and F's head
    assert per_wave(wgs[4]) == [[0, 2, 3], [3]] and per_trip(wgs[4]) == [[0, 2, 3]]  # three units in a wave, an empty one among them
    assert per_wave(wgs[5]) == [[0], [0, 3], [3]] and per_trip(wgs[5]) == [[0, 3]]   # two units in a wave, two empty ones between
    assert list(wgs[1]["first"]) == [0, 0, 0, 0] and list(wgs[2]["first"][1:]) == [wgs[2]["nvis"]] * 3 and list(wgs[3]["first"]) == [0, 0, 1024, 2048]
    assert list(wgs[4]["first"]) == [0, 50, 50, 60] and list(wgs[5]["first"]) == [0, 70, 70, 70]


# i. cursors and shards
def fit_scene(over):
    """33 workgroups; those of shard 0 (0, 16, 32) ask for exactly a fresh context's shard_cap slots: workgroup 0 holds 1000 posts of 64
    slots and 24 dots, workgroup 16 holds 23 posts and 39 dots among culled splats, workgroup 32 one dot (over: two).  Every other
    workgroup holds culled splats and one dot."""
    def make():
        q = Seq(FIT_CANVAS, _rng(27, over))
        pk = short_post(FIT_CANVAS, 64)[0]
        q.add(pk, times=1000).dots(24).permuted(0, 1024)
        for b in range(1, 33):
            if b == 16:
                q.culled(500).add(pk, times=23).dots(39).culled(1024 - 562)
            else:
                extra = 1 if b == 32 and over else 0
                q.culled(700).dots(1 + extra).culled(323 - extra)
        return q.scene("fit_%d" % over)
    return cached(("proj_fit_scene", over), make)


@pytest.mark.parametrize("over", [0, 1])
def test_fit_scenes(over):
    sc = fit_scene(over)
    p = pm(sc)
    n = sc["P"].shape[0]
    assert n == 33 * 1024 and max(2 * n, 1 << 20) == pr.FRESH_ROWS
    cap = pr.shard_cap(pr.FRESH_ROWS)
    assert cap == 65536 and p["shard_rows"][0] == cap + over and (p["shard_rows"][1:] == 2).all()
    assert p["shard_rows"].sum() == cap + over + 30 < pr.FRESH_ROWS // 15  # the frame's total is far below the arena's size
    bumps = [int(R) for b in (0, 16, 32) for R in p["wg"][b]["R"] if R]
    assert sum(bumps) == cap + over and len(bumps) == 6
    for R in bumps:  # whichever bump comes last ends on the shard's last slot (over: one beyond it)
        at = cap + over - R
        assert pr.fits(at, R, cap) == (not over)
        assert not pr.fits(at, R, cap, strict=False)  # with >= in place of > the exact fit would be refused too
    assert 16 * max(p["shard_rows"]) <= pr.FRESH_ROWS if not over else 16 * max(p["shard_rows"]) > pr.FRESH_ROWS  # gs_wait's rows_last
    assert owners_agree(p)


def record_scene(n):
    def make():
        q = Seq(DOT_CANVAS, _rng(28, n))
        return q.dots(n).scene("records_%d" % n)
    return cached(("proj_record_scene", n), make)


@pytest.mark.parametrize("n", [17 * 1024, 16 * 1024 + 1])
def test_record_scenes(n):
    p = pm(record_scene(n))
    assert p["workgroups"] == 17 and pr.rec_shard_cap(n, 2) == 2048
    assert p["shard_recs"][0] == (2048 if n == 17 * 1024 else 1025) and (p["shard_recs"][1:] == 1024).all()
    assert p["wg"][16]["nvis"] == n - 16 * 1024 and (p["shard_recs"] <= pr.rec_shard_cap(n, 2)).all()


# j. the other instantiations
def state_plane(sc, which):
    n = sc["P"].shape[0]
    return np.where((np.arange(n) % 3 == 2) & (which == "every_third"), sr.HIDDEN, 0).astype(np.uint8)


@pytest.mark.parametrize("which", ["zero", "every_third"])
@pytest.mark.parametrize("case", ["markless", "maxima"])
def test_state_scenes(case, which):
    """With every third splat hidden the survivors move up: the long posts of markless x40 (indices 40 and 46) stay, in lanes 27 and
    31; of the 64 blankets 43 stay, followed by dots in the same wave."""
    sc = markless_scene("x40") if case == "markless" else maxima_scene("wave")
    hidden = (state_plane(sc, which) & sr.HIDDEN) != 0
    p = pm(sc, hidden=hidden)
    g = p["wg"][0]
    assert g["nvis"] == 256 - int(hidden.sum()) and owners_agree(p)
    if which == "zero":
        check_markless(p, "x40") if case == "markless" else check_maxima(p, "wave")
    elif case == "markless":
        ns = g["ns"][0, 0]
        assert list(np.flatnonzero(ns >= 200)) == [27, 31] and pr.owners_kernel(g["ns"][0])[1][0] >= 4 and differs(g["ns"][0], carry=False)
    else:
        assert g["Rw"][0, 0] == 43 * 510 + 21 and g["Cw"][0, 0] == 64


SLAB = (1, 2)


def test_slab_scene():
    """cols = (1, 2) of the 2-column canvas: the posts stand in column 1 and so do all dots (the reach cull keeps them all); the posts'
    rects reach the aliased column, which is column 0 of the next row and outside the slab: a post has one slot per row."""
    sc = markless_scene("x40", col=1, cols=SLAB, tag="_slab")
    p = pm(sc, NB=4)
    assert p["workgroups"] == 1
    check_markless(p, "x40")


# ---- GPU: the frames ----------------------------------------------------------------------------------------------------------------
def proj_frames(oracle, sc, chunks=0, state=None, before=None, each=None):
    """row_scenes.frames with the options of a case: GS_OPT_FRAMES_IN_FLIGHT 1, GS_OPT_PROJ_CHUNKS, a state plane (the reference is
    then state_restate.state_frame's).  before(r, u) runs ahead of the first frame, each(r, stats, k) after the checks of frame k.
    Returns the stats of the two frames."""
    from gsplat import _abi
    s, u = frame_of(sc)
    W, H, ts, cols = sc["W"], sc["H"], sc["ts"], sc["cols"]
    if state is None:
        m = model_of(sc)
        ref = oracle_frame(oracle, "rows_" + sc["name"], s, u, W, H, ts, cols=cols)
    else:
        hidden = (state & sr.HIDDEN) != 0
        sl, bucket = tight_check.dump(s, u, W, H, ts, cols)
        m = rr.model(sl[~hidden[sl[:, 0].astype(np.int64)]], bucket)
        ref = cached(("proj_state_ref", sc["name"], int(hidden.sum())), lambda: sr.state_frame(oracle, s, u, W, H, ts, state, cols=cols))
    r = mk(s, W, H, ts, exact=True, cols=cols, state=state is not None)
    out = []
    try:
        r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
        if chunks:
            r.set_option(_abi.GS_OPT_PROJ_CHUNKS, chunks)
        if state is not None:
            r.write_state(state)
        if before:
            before(r, u)
        for k, grid in enumerate((0, 4)):
            if grid:
                r.set_option(_abi.GS_OPT_PERSISTENT_GRID, grid)
            r.render_uniforms(u)
            r.wait()
            st = r.stats()
            print("%s grid %d: slots %d items %d instances %d (model %d %d %d) row_capacity %d" % (
                sc["name"], grid, st["num_row_slots"], st["num_row_items"], st["num_intersections"], m["S"], m["R"], m["I"], st["row_capacity"]))
            assert st["tight_binning"] == 1
            assert st["num_row_slots"] == m["S"]
            assert st["num_row_items"] == m["R"]
            assert st["num_intersections"] == m["I"]
            check_product_lists(r, ref, oracle, W, H, ts)
            check_image(r, ref, True)
            if each:
                each(r, st, k)
            out.append(st)
    finally:
        r.destroy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("Rw", WAVE_TOTALS)
def test_wave_totals(oracle, Rw):
    frames(oracle, total_scene(Rw))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STRADDLE))
def test_owner_across_a_batch(oracle, name):
    frames(oracle, straddle_scene(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", MARKLESS)
def test_batches_without_a_mark(oracle, name):
    frames(oracle, markless_scene(name))


@pytest.mark.gpu
def test_survivors_without_slots(oracle):
    frames(oracle, faint_scene())


@pytest.mark.gpu
def test_survivors_with_holes_alone(oracle):
    """The ghosts take arena slots and a record slot each, get count word 0 and are not listed."""
    from gsplat import _abi
    sc = ghost_scene()
    gh = np.flatnonzero(sc["cls"] == GHOST)

    def each(r, st, k):
        assert not r.read_buffer(_abi.GS_BUF_TILE_COUNTS)[gh].any() and not np.isin(gh, r.read_buffer(_abi.GS_BUF_VALUES)).any()
        assert st["num_visible"] == 256 - gh.size
    proj_frames(oracle, sc, each=each)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wave", "trip"])
def test_packed_words_at_their_maxima(oracle, name):
    """wave: no regrow.  trip: the first frame asks one shard for 130 560 slots, twice a fresh shard: it regrows and still passes every
    check; the second frame does not regrow and equals the first."""
    from gsplat import _abi
    seen = []

    def each(r, st, k):
        seen.append((r.read_rgba8(), r.read_buffer(_abi.GS_BUF_VALUES), r.read_buffer(_abi.GS_BUF_RANGES)))
    first, second = proj_frames(oracle, maxima_scene(name), each=each)
    if name == "wave":
        assert first["row_capacity"] == second["row_capacity"] == pr.FRESH_ROWS
    else:
        assert first["row_capacity"] > pr.FRESH_ROWS and first["row_capacity"] >= 16 * 130560 and second["row_capacity"] == first["row_capacity"]
    for a, b in zip(*seen):
        np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("nvis,NB", [(v, 2) for v in NVIS_2] + [(v, 8) for v in NVIS_8])
def test_trips(oracle, nvis, NB):
    sc = trips_scene(nvis, NB)
    if NB == 2:
        frames(oracle, sc)
    else:
        proj_frames(oracle, sc, chunks=NB)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [4, 8])
def test_units_inside_a_workgroup(oracle, chunks):
    from test_gsort_dense import H, TS, W, _check
    s, z = unit_scene()
    u = pinhole(W, H)
    got = _check(oracle, s, u, oracle_frame(oracle, "proj_units", s, u, W, H, TS), chunks=chunks)
    vis = got["TILE_COUNTS"] > 0
    assert not vis[z < 0].any() and vis.any()


@pytest.mark.gpu
@pytest.mark.parametrize("over", [0, 1])
def test_row_shard_exact_fit_and_one_over(oracle, over):
    """Shard 0 is asked for exactly its capacity: no regrow.  One slot more, with fifteen shards almost empty: the frame regrows."""
    fresh = []

    def before(r, u):
        r.render_uniforms(u, debug=True)  # a frame that hands out no arena slot
        r.wait()
        fresh.append(r.stats()["row_capacity"])
    first, second = proj_frames(oracle, fit_scene(over), before=before)
    assert fresh[0] == pr.FRESH_ROWS and pr.shard_cap(fresh[0]) == 65536
    if over:
        assert first["row_capacity"] > fresh[0] and second["row_capacity"] == first["row_capacity"]
    else:
        assert first["row_capacity"] == second["row_capacity"] == fresh[0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17 * 1024, 16 * 1024 + 1])
def test_record_shards_full(oracle, n):
    """Shard 0's two workgroups take all 2048 records of rec_shard_cap (one of them a single splat at 16 * 1024 + 1)."""
    from gsplat import _abi
    dbg = []

    def before(r, u):
        r.render_uniforms(u, debug=True)
        r.wait()
        dbg.append(r.read_buffer(_abi.GS_BUF_GAUSSIAN_DATA).reshape(-1, 16))

    def each(r, st, k):
        vals = r.read_buffer(_abi.GS_BUF_VALUES)
        gd = r.read_buffer(_abi.GS_BUF_GAUSSIAN_DATA).reshape(-1, 16)
        listed = np.unique(vals)
        assert listed.size == n and st["num_visible"] == n
        np.testing.assert_array_equal(gd[listed], dbg[0][listed])
        np.testing.assert_array_equal(r.read_buffer(_abi.GS_BUF_TILE_COUNTS), np.bincount(vals, minlength=n).astype(np.uint32))
    proj_frames(oracle, record_scene(n), before=before, each=each)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["zero", "every_third"])
@pytest.mark.parametrize("case", ["markless", "maxima"])
def test_state_instantiation(oracle, case, which):
    sc = markless_scene("x40") if case == "markless" else maxima_scene("wave")
    first, second = proj_frames(oracle, sc, state=state_plane(sc, which))
    assert first["row_capacity"] == second["row_capacity"] == pr.FRESH_ROWS


@pytest.mark.gpu
def test_slab_instantiation(oracle):
    proj_frames(oracle, markless_scene("x40", col=1, cols=SLAB, tag="_slab"))
