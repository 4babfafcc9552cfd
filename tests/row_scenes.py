"""Scenes whose row items are known, for the boundary suites of the tight path (test_row_boundaries.py, test_projection_slots.py).

Scenes are built in pixel space from four kinds of splat: DOTS (one slot, one item, one instance), BARS (one item of L tiles), POSTS
(one-tile items in consecutive tile rows) and BLANKETS (an item of ntx tiles in every row, plus the aliased column's items).  What a
scene gives the row pipeline is computed on the CPU: tools/tight_check (gs_tight.h compiled for the host) dumps every slot,
rows_restate.model orders and cuts them the way the kernels do.  `frames` renders a scene on the product path and compares counts,
lists and image.  A plain module like gpu_checks and the *_restate modules.
"""
import importlib.util
import os

import numpy as np

import rows_restate as rr
from gpu_checks import check_image, check_product_lists
from support import ROOT, cached, make_splats, mk, oracle_frame, pinhole, pixel_ellipse, pixel_uniforms

_spec = importlib.util.spec_from_file_location("tight_check_run_rows", os.path.join(ROOT, "tools", "tight_check", "run.py"))
tight_check = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tight_check)

FLOOR = 1e-4       # a pixel-space deviation far below the projection's 0.3 px^2: the splat is 0.55 px of sigma
BAR_LOGIT = 1.0    # bars, posts and ghosts have one opacity: their extent depends on it
BLANKET_LOGIT = -4.0  # opacity 0.018: ln(255 op) = 1.5
DEFAULT = (192, 144, 16)  # 12 x 9 tiles
POST_CANVAS = (16, 320, 8)
LONG_CANVAS = (16, 2040, 8)


# ---- splats -------------------------------------------------------------------------------------------------------------------------
def params(px, py, sl, ss, th, logit):
    """[n, 6]: centre, pixel-space deviations along axes rotated by th, opacity logit."""
    return np.stack([np.asarray(a, np.float64) for a in np.broadcast_arrays(np.atleast_1d(px), py, sl, ss, th, logit)], axis=1).reshape(-1, 6)


def dots(ts, tx, ty, rng):
    """Floor-size splats on the centres of tiles (tx, ty)."""
    tx, ty = np.asarray(tx, np.float64), np.asarray(ty, np.float64)
    return params(ts * tx + ts / 2.0, ts * ty + ts / 2.0, FLOOR, FLOOR, 0.0, rng.uniform(-1.0, 2.0, tx.shape))


def records(P, W, H, z=None, seed=0):
    """(splats, uniforms) of parameter rows P: at depth 1 in pixel space, or (z given) at depths z under support.pinhole, where a
    splat keeps its pixels: position and scales are multiplied by z."""
    rng = np.random.Generator(np.random.Philox(key=[6100, seed]))
    a, b, t = pixel_ellipse(W, H, P[:, 2], P[:, 3], P[:, 4])
    s = make_splats(W, H, P[:, 0], P[:, 1], a, b, t, P[:, 5].astype(np.float32), color=rng.uniform(-1.0, 1.5, (P.shape[0], 3)))
    if z is None:
        return s, pixel_uniforms(W, H)
    z = np.asarray(z, np.float64)
    s[:, 0] = (s[:, 0].astype(np.float64) * z).astype(np.float32)
    s[:, 1] = (s[:, 1].astype(np.float64) * z).astype(np.float32)
    s[:, 2] = z.astype(np.float32)
    s[:, 4:7] = (s[:, 4:7].astype(np.float64) + np.log(z)[:, None]).astype(np.float32)
    return s, pinhole(W, H)


def slots_of(P, W, H, ts, z=None, cols=None):
    s, u = records(P, W, H, z)
    return tight_check.dump(s, u, W, H, ts, cols)


def per_splat(P, W, H, ts):
    """Per row of P: (slots, items, instances, first tile column of its first item, tile row of its first item); 0s without slots."""
    sl, _ = slots_of(P, W, H, ts)
    n = P.shape[0]
    g, tiles = sl[:, 0].astype(np.int64), sl[:, 4].astype(np.int64)
    out = np.zeros((n, 5), np.int64)
    out[:, 0] = np.bincount(g, minlength=n)
    out[:, 1] = np.bincount(g[tiles > 0], minlength=n)
    out[:, 2] = np.bincount(g, weights=tiles, minlength=n)
    fi = np.flatnonzero(tiles > 0)[::-1]  # (reversed: the first item of a gaussian is written last)
    out[g[fi], 3], out[g[fi], 4] = sl[fi, 3], sl[fi, 2]
    return out


def bar_table(W, H, ts):
    """L -> (centre x, sigma) of a horizontal bar (floor thick, on a tile row's centre line) that is ONE slot holding one item of L tiles:
    its 3-sigma rect stays off the canvas's last column (no aliased slot).  Of the sigmas that give a length, the middle one: far from
    the two at which the run gains a tile, where the host's log2f and the device's v_log_f32 might disagree."""
    def make():
        sig = np.geomspace(1.0, W / 5.0, 500)
        ntx = W // ts
        xs = [ts * (ntx // 2) + 0.3, ts * (ntx // 2) + ts / 2.0 + 0.3]  # (off the integers: centre +- the rect's integer radius is on no tile boundary)
        P = np.concatenate([params(x, ts * 1.5, sig, FLOOR, 0.0, BAR_LOGIT) for x in xs])
        sh = per_splat(P, W, H, ts)
        table = {}
        for k, x in enumerate(xs):
            part = sh[k * sig.size:(k + 1) * sig.size]
            ok = (part[:, 0] == 1) & (part[:, 1] == 1)
            for L in np.unique(part[ok, 2]):
                idx = np.flatnonzero(ok & (part[:, 2] == L))
                if idx.size >= 3 and int(L) not in table:
                    table[int(L)] = (x, float(sig[idx[idx.size // 2]]))
        return table
    return cached(("bar_table", W, H, ts), make)


def bars(W, H, ts, row, L, rng):
    """One bar of L[i] tiles per entry, in tile row `row`, moved by whole tiles as far as its rect stays inside the canvas."""
    tab = bar_table(W, H, ts)
    out = []
    for l in np.atleast_1d(L):
        x, sg = tab[int(l)]
        room = int(max((min(x, W - x) - 3.0 * sg - 4.0) // ts, 0))
        out.append(params(x + ts * int(rng.integers(-room, room + 1)), ts * row + ts / 2.0, sg, FLOOR, 0.0, BAR_LOGIT))
    return np.concatenate(out) if out else np.zeros((0, 6))


def post(W, H, ts, want):
    """A vertical splat (floor thick, in tile column 1) and its per_splat row, the first of a sweep of heights and centres for which
    want(row) holds and whose neighbours in the sweep have the same shape.  On a canvas narrower than the post's 3-sigma radius the
    rect reaches the aliased column: the post then has twice as many slots as tile rows -- first the rows' items, then the aliased
    column's slots of the same rows, all holes (tile (row + 1, 0) is not touched from column 1)."""
    def make():
        sig = np.geomspace(3.0, H / 5.0, 300)
        P = np.concatenate([params(ts * 1.5, y, FLOOR, sig, 0.0, BAR_LOGIT) for y in (ts * (H // ts // 2) + 0.3, ts * (H // ts // 2) + ts / 2.0 + 0.3)])
        return P, per_splat(P, W, H, ts)
    P, sh = cached(("posts", W, H, ts), make)
    for i in range(1, P.shape[0] - 1):  # (inside a run of equal shapes: not the first or last height that gives it)
        if want(sh[i]) and (sh[i - 1] == sh[i]).all() and (sh[i + 1] == sh[i]).all():
            return P[i:i + 1], sh[i]
    raise AssertionError("no post of the wanted shape on %dx%d tile %d" % (W, H, ts))


def blankets(W, H, k):
    return params(np.full(k, W / 2.0), H / 2.0, 3.0 * max(W, H), 3.0 * max(W, H), 0.0, BLANKET_LOGIT)


def interleave(A, B):
    """Record order a0 b0 a1 b1 ...; the longer one's tail follows.  Returns (rows, which: 0 / 1)."""
    n = min(A.shape[0], B.shape[0])
    head = np.empty((2 * n, 6))
    head[0::2], head[1::2] = A[:n], B[:n]
    which = np.concatenate([np.tile([0, 1], n), np.zeros(A.shape[0] - n, int), np.ones(B.shape[0] - n, int)])
    return np.concatenate([head, A[n:], B[n:]]), which


# ---- scenes: name -> {P, z, W, H, ts, cols} and what the case is to reach ------------------------------------------------------------
def scene(name, W, H, ts, P, z=None, cols=None, **want):
    return dict(name=name, W=W, H=H, ts=ts, P=P, z=z, cols=cols, want=want)


def frame_of(sc):
    return cached(("rows_records", sc["name"]), lambda: records(sc["P"], sc["W"], sc["H"], sc["z"], seed=len(sc["name"])))


def model_of(sc):
    def make():
        s, u = frame_of(sc)
        return rr.model(*tight_check.dump(s, u, sc["W"], sc["H"], sc["ts"], sc["cols"]))
    return cached(("rows_model", sc["name"]), make)


def _rng(*key):
    word = 0
    for k in key:
        word = (word * 1000003 + int(k) + 1) % (1 << 63)
    return np.random.Generator(np.random.Philox(key=[6101, word]))


# ---- GPU: the frames ----------------------------------------------------------------------------------------------------------------
def frames(oracle, sc):
    """The scene on the product path, default grid and GS_OPT_PERSISTENT_GRID 4: counts (with equality), lists, exact image."""
    from gsplat import _abi
    s, u = frame_of(sc)
    m = model_of(sc)
    W, H, ts, cols = sc["W"], sc["H"], sc["ts"], sc["cols"]
    ref = oracle_frame(oracle, "rows_" + sc["name"], s, u, W, H, ts, cols=cols)
    r = mk(s, W, H, ts, exact=True, cols=cols)
    try:
        for grid in (0, 4):
            if grid:
                # (gs_set_option stores the value and drops the captured frame, so the next frame is launched with it; the library has no
                # read-back of an option or of a launch's grid, and this module adds no tap: that 4 means 3 / 8 / 6 workgroups is
                # rows_restate.grids' restatement of gs_frame.hip and k_rows.hip, not something a frame reports)
                r.set_option(_abi.GS_OPT_PERSISTENT_GRID, grid)
            r.render_uniforms(u)
            r.wait()
            st = r.stats()
            print("%s grid %d: slots %d items %d instances %d (model %d %d %d)" % (sc["name"], grid, st["num_row_slots"], st["num_row_items"],
                                                                                 st["num_intersections"], m["S"], m["R"], m["I"]))
            assert st["tight_binning"] == 1
            assert st["num_row_slots"] == m["S"]
            assert st["num_row_items"] == m["R"]
            assert st["num_intersections"] == m["I"]
            check_product_lists(r, ref, oracle, W, H, ts)
            check_image(r, ref, True)
    finally:
        r.destroy()
