"""What the test modules share: paths, the issue scenes with their oracle frames (one cache), the renderer factory, and the
blocks every feature's tests repeat (run a Node check script, compile a layout probe against the header, read the hosts'
sources).  A plain module like gpu_checks and the *_restate modules; a helper only one test file uses stays in that file.
"""
import collections
import ctypes
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import scene
import export_restate as er
import state_restate as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "gsplat", "gs_abi.h")
JS_DIR = os.path.join(ROOT, "gaussian-splatting-wgpu_amd", "js")
NAPI_SRC = os.path.join(ROOT, "gaussian-splatting-wgpu_amd", "csrc", "napi", "gs_napi.c")
F = np.float32
NODE = shutil.which("node")

_CACHE = {}


def cached(key, make):
    """make() once per key and session.  The key names everything the value depends on."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def oracle_frame(oracle, name, s, u, W, H, ts, **kw):
    """oracle.render of the scene called `name` (the name stands for s and u), once per (scene, canvas, tile size, arguments).  A
    frame rendered with other arguments is never handed out; an argument left out and one given as None / False are the same call
    (gs_oracle.render's defaults)."""
    args = tuple(sorted((k, v) for k, v in kw.items() if v is not None and v is not False))
    return cached(("render", name, W, H, ts, args), lambda: oracle.render(s, u, W, H, ts, **kw))


# ---- the splat-state scenes: config A and the ragged golden, their regions, planes and constructed frames ---------------------------
FRAME_CASES = [("cfgA", 8), ("cfgA", 16), ("cfgA", 32), ("ragged", 8)]  # (scene, tile size)


def state_scene(name):
    """(splats, uniforms, W, H) of "cfgA" or "ragged"."""
    def make():
        if name == "cfgA":
            from gpu_checks import orbit_uniforms
            return scene(10000), orbit_uniforms(256, 256), 256, 256
        from gsplat import synth
        z = np.load(os.path.join(GOLDEN, "ragged_3001_200x120_t8.npz"))
        n, W, H, _, _ = (int(v) for v in z["params"])
        return synth.bicycle_like(n), np.array(z["uniforms"], F), W, H
    return cached(("state_scene", name), make)


def in_region(name, region):
    """Membership of the scene's splats in one of state_restate.issue_regions."""
    def make():
        s, u, W, H = state_scene(name)
        kind, kw = sr.issue_regions(W, H, u)[region]
        return sr.member(kind, s, W, H, **kw)
    return cached(("inside", name, region), make)


def hidden_plane(name, which):
    s, _, _, _ = state_scene(name)
    n = s.shape[0]
    if which == "every_third":
        h = np.arange(n) % 3 == 1
    elif which == "centre_half_rect":
        h = in_region(name, "centre_half_rect")
    else:
        h = np.ones(n, bool)
    return np.where(h, sr.HIDDEN, 0).astype(np.uint8)


def state_ref(oracle, name, ts, key, state, tint=sr.TINT_DEFAULT, cols=None):
    """The constructed reference frame of a state plane (`key` names the plane), computed once per (scene, tile size, plane, tint,
    slab) and shared."""
    def make():
        s, u, W, H = state_scene(name)
        return sr.state_frame(oracle, s, u, W, H, ts, state, tint, cols, want_illcond=True)
    return cached(("state_ref", name, ts, key, tint, cols), make)


# ---- the margin scenes of the blend's parking culls (test_blend_culls.py), built in pixel space ------------------------------------
def pixel_uniforms(W, H):
    u = np.zeros(40, dtype=np.float32)
    u[0] = u[5] = u[10] = u[15] = 1.0      # view = I (column-major)
    u[16] = u[21] = u[26] = u[31] = 1.0    # proj = I: ndc = pos
    u[35] = u[36] = 0.5                    # tan_fov
    u[37], u[38] = W / 2.0, H / 2.0        # focal: one world unit at depth 1 = W / 2 pixels
    u[39] = 1.0
    return u


def pinhole(W, H):
    """Identity view, w = z: depth = the splat's z, ndc = (x, y) / z, focal = half the canvas."""
    u = np.zeros(40, dtype=np.float32)
    u[0] = u[5] = u[10] = u[15] = 1.0
    u[16] = u[21] = 1.0
    u[26] = 1.0
    u[27] = 1.0
    u[35] = u[36] = 1.0
    u[37], u[38] = W / 2.0, H / 2.0
    u[39] = 1.0
    return u


def make_splats(W, H, px, py, sig_long, sig_short, theta, logit, color=None, rng=None):
    """Records with centres (px, py) in pixels, pixel-space standard deviations (before the projection's +0.3 px^2) along the
    axes of a rotation by theta about the view axis, opacity logits.  Depth 1 for all: the list order is the record order."""
    n = np.size(px)
    s = np.zeros((n, 80), dtype=np.float32)
    s[:, 0] = 2.0 * np.asarray(px, np.float64) / W - 1.0
    s[:, 1] = 2.0 * np.asarray(py, np.float64) / H - 1.0
    s[:, 2] = 1.0
    f = W / 2.0  # = H / 2 * (W / H): both focal lengths map one unit to W / 2 resp. H / 2 pixels
    s[:, 4] = np.log(np.maximum(np.asarray(sig_long, np.float64), 1e-30) / f)
    s[:, 5] = np.log(np.maximum(np.asarray(sig_short, np.float64), 1e-30) / (H / 2.0))
    s[:, 6] = -30.0  # flat along the view axis: the projected covariance does not depend on the centre
    th = np.asarray(theta, np.float64)
    s[:, 8] = np.cos(th / 2.0)
    s[:, 11] = np.sin(th / 2.0)
    s[:, 12] = logit
    if color is None:
        color = (rng.uniform(-1.5, 1.5, (n, 3)) if rng is not None else np.zeros((n, 3)))
    s[:, 16:19] = color
    return s


def opacity_logits(oracle, targets):
    """Logits whose f32 opacity in the oracle's gdata (word 11) is the largest one <= target, by bisection (all at once)."""
    targets = np.asarray(targets, np.float64)
    lo = np.full(targets.shape, -20.0)
    hi = np.full(targets.shape, 20.0)
    W = H = 64
    u = pixel_uniforms(W, H)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        s = make_splats(W, H, np.full(mid.size, 32.0), np.full(mid.size, 32.0), 4.0, 4.0, 0.0, mid.astype(np.float32))
        op = oracle.preprocess(s, u, W, H, 8)[0][:, 11].view(np.float32).astype(np.float64)
        ok = op <= targets
        lo = np.where(ok, mid, lo)
        hi = np.where(ok, hi, mid)
    return lo.astype(np.float32)


def gdata_f32(gdata):
    return gdata.view(np.float32).reshape(-1, 16)


def box_qmin_f64(cx, cy, cz, dxlo, dxhi, dylo, dyhi):
    """min over [dxlo,dxhi] x [dylo,dyhi] of 0.5 (cx dx^2 + cz dy^2) + cy dx dy (positive-definite conics), in f64."""
    q = lambda dx, dy: 0.5 * (cx * dx * dx + cz * dy * dy) + cy * dx * dy
    inside = (dxlo <= 0) & (dxhi >= 0) & (dylo <= 0) & (dyhi >= 0)
    best = np.full(np.shape(cx), np.inf)
    with np.errstate(all="ignore"):
        for X in (dxlo, dxhi):  # vertical edges: dy = argmin clamped
            dy = np.clip(-cy * X / cz, dylo, dyhi)
            best = np.minimum(best, q(X, dy))
        for Y in (dylo, dyhi):
            dx = np.clip(-cy * Y / cx, dxlo, dxhi)
            best = np.minimum(best, q(dx, Y))
    return np.where(inside, 0.0, best)


HUGE = 1.0e5  # pixels of sigma: conic ~ 1e-10, alpha uniform over the canvas to ~1e-6


def _front(oracle, W, H, T0):
    """Two huge, near-uniform splats: T = 1 -> 0.01 -> T0 on every pixel."""
    ops = np.array([0.99, 1.0 - T0 / 0.01])
    lg = opacity_logits(oracle, ops)
    return make_splats(W, H, np.full(2, W / 2.0), np.full(2, H / 2.0), HUGE, HUGE, 0.0, lg, color=[[0.4, -0.2, 0.1], [-0.3, 0.6, 0.2]])


def transmittance_edge_scene(oracle, seed=0):
    """T just above the final threshold on most pixels, spread across pixels (so that Tmax is not most pixels' own T), then a
    sweep of huge, uniform entries whose T (1 - alpha) puts each block's Tmax pixel at 1e-4 (1 +- delta), and entries at the
    0.99 clamp.  Returns (splats, uniforms, W, H)."""
    W, H = 115, 83
    rng = np.random.Generator(np.random.Philox(key=[4101, seed]))
    parts = [_front(oracle, W, H, 1.048e-4)]
    # the spread: moderate splats, peak alpha 0.02 .. 0.044 (T0 (1 - alpha) >= 1e-4 needs alpha <= 0.0458)
    k = 9
    lg = opacity_logits(oracle, rng.uniform(0.02, 0.044, k))
    parts.append(make_splats(W, H, rng.uniform(0, W, k), rng.uniform(0, H, k), rng.uniform(15, 45, k), rng.uniform(15, 45, k),
                             rng.uniform(0, np.pi, k), lg, rng=rng))
    # the sweep: threshold tau = 1e-4 / (1 - alpha) from 1.048e-4 down in steps of ~0.05 %, with jitter
    tau = np.sort(1e-4 * np.exp(rng.uniform(np.log(1.0039), np.log(1.0485), 90)))[::-1]
    lg = opacity_logits(oracle, 1.0 - 1e-4 / tau)
    parts.append(make_splats(W, H, np.full(tau.size, W / 2.0), np.full(tau.size, H / 2.0), HUGE, HUGE, 0.0, lg, rng=rng))
    # ... and the 0.99 clamp: logits >= 4.6 (alpha = 0.99, alo = 0.99 * 0.99), uniform and local
    k = 6
    lg = np.array([4.6, 4.7, 6.0, 9.0, 12.0, 30.0], np.float32)
    parts.append(make_splats(W, H, rng.uniform(0, W, k), rng.uniform(0, H, k), np.where(np.arange(k) < 3, HUGE, 20.0),
                             np.where(np.arange(k) < 3, HUGE, 6.0), rng.uniform(0, np.pi, k), lg, rng=rng))
    return np.concatenate(parts), pixel_uniforms(W, H), W, H


def _live_patterns(bx0, by0, bw, bh):
    """Live pixel sets of an 8x8 block whose in-canvas part is bw x bh: one corner, one row, one column, two opposite corners."""
    xr, yb = bx0 + bw - 1, by0 + bh - 1
    return [[(bx0, by0)], [(xr, by0)], [(bx0, yb)], [(xr, yb)],
            [(x, by0) for x in range(bx0, xr + 1)], [(x, yb) for x in range(bx0, xr + 1)],
            [(bx0, y) for y in range(by0, yb + 1)], [(xr, y) for y in range(by0, yb + 1)],
            [(bx0, by0), (xr, yb)], [(xr, by0), (bx0, yb)]]


def live_box_scene(oracle, seed=0):
    """Blocks whose pixels are all final but for one corner, one row, one column or two opposite corners (every block of the
    canvas but a few, the partial ones at the right and bottom edges included), then thin rotated splats centred outside the
    block whose alpha = 1/255 contour passes just inside or just outside the live box: q_min(box) - ln(255 op) = +-3e-4 .. 1e-2.
    How: two huge, uniform splats bring every pixel to T0 = 5e-4; a tiny splat with alpha 0.005 at each pixel to be kept live
    (its neighbours see alpha < 1/255); a huge, uniform finisher with T0 (1 - alpha_f) = 1.002e-4 then leaves every other pixel
    final (T in [1e-4, 1.0039e-4)) and is rejected by the live ones (0.995 T0 (1 - alpha_f) < 1e-4)."""
    W, H = 101, 75
    rng = np.random.Generator(np.random.Philox(key=[4102, seed]))
    T0 = 5e-4
    front = _front(oracle, W, H, T0)
    live, boxes = [], []
    for by0 in range(0, H, 8):
        for bx0 in range(0, W, 8):
            if rng.uniform() < 0.25:
                continue  # left fully final
            pats = _live_patterns(bx0, by0, min(8, W - bx0), min(8, H - by0))
            pix = pats[int(rng.integers(len(pats)))]
            live += pix
            xs, ys = [p[0] for p in pix], [p[1] for p in pix]
            boxes.append((bx0, by0, min(xs), max(xs), min(ys), max(ys)))
    live = np.array(live, np.float64)
    nb = live.shape[0]
    blockers = make_splats(W, H, live[:, 0], live[:, 1], 1e-4, 1e-4, 0.0, opacity_logits(oracle, np.full(nb, 0.005)), rng=rng)
    fin = make_splats(W, H, [W / 2.0], [H / 2.0], HUGE, HUGE, 0.0, opacity_logits(oracle, [1.0 - 1.002e-4 / T0]), color=[[0.2, 0.2, 0.2]])
    # the probes: per live box, targets on its corners (outward quadrant) and edges (outward normal, only where the edge is
    # on the block's boundary, so that the centre lies outside the block)
    P, U = [], []
    for bx0, by0, x0, x1, y0, y1 in boxes:
        for _ in range(7):
            if rng.uniform() < 0.5:  # a corner of the box
                sx, sy = rng.choice([-1.0, 1.0]), rng.choice([-1.0, 1.0])
                phi = rng.uniform(0.15, 1.42)
                P.append((x0 if sx < 0 else x1, y0 if sy < 0 else y1))
                U.append((sx * np.cos(phi), sy * np.sin(phi)))
            else:  # an edge
                side = int(rng.integers(4))
                psi = rng.uniform(-0.9, 0.9)
                if side == 0:
                    P.append((rng.uniform(x0, x1), y0)); U.append((np.sin(psi), -np.cos(psi)))
                elif side == 1:
                    P.append((rng.uniform(x0, x1), y1)); U.append((np.sin(psi), np.cos(psi)))
                elif side == 2:
                    P.append((x0, rng.uniform(y0, y1))); U.append((-np.cos(psi), np.sin(psi)))
                else:
                    P.append((x1, rng.uniform(y0, y1))); U.append((np.cos(psi), np.sin(psi)))
    P, U = np.array(P), np.array(U)
    bidx = np.repeat(np.arange(len(boxes)), 7)
    bx = np.array(boxes, np.float64)[bidx]
    n = P.shape[0]
    theta = np.arctan2(U[:, 1], U[:, 0]) + rng.uniform(-0.5, 0.5, n)  # long axis roughly along the approach, rotated
    lg = np.where(rng.uniform(size=n) < 0.3, rng.uniform(-5.52, -5.45, n), rng.uniform(-4.0, 3.0, n)).astype(np.float32)
    sigl = rng.uniform(18.0, 30.0, n)  # eigenvalues of the projected covariance >= 324 : 0.3, a ratio >= 1e3
    probe = make_splats(W, H, P[:, 0], P[:, 1], sigl, 1e-4, theta, lg, rng=rng)
    g = gdata_f32(oracle.preprocess(probe, pixel_uniforms(W, H), W, H, 8)[0])
    cx, cy, cz, op = [g[:, k].astype(np.float64) for k in (4, 5, 6, 11)]
    target = np.log(255.0 * op) + rng.choice([-1e-2, -3e-3, -1e-3, -3e-4, 3e-4, 1e-3, 3e-3, 1e-2], n)
    lo, hi = np.zeros(n), np.full(n, 400.0)
    for _ in range(60):  # the distance along U at which min over the live box of q reaches the target
        t = 0.5 * (lo + hi)
        ex, ey = P[:, 0] + t * U[:, 0], P[:, 1] + t * U[:, 1]
        q = box_qmin_f64(cx, cy, cz, ex - bx[:, 3], ex - bx[:, 2], ey - bx[:, 5], ey - bx[:, 4])
        lo, hi = np.where(q < target, t, lo), np.where(q < target, hi, t)
    ex, ey = P[:, 0] + lo * U[:, 0], P[:, 1] + lo * U[:, 1]
    out = ~((ex > bx[:, 0] - 0.5) & (ex < bx[:, 0] + 7.5) & (ey > bx[:, 1] - 0.5) & (ey < bx[:, 1] + 7.5))
    ok = out & (ex > -0.04 * W) & (ex < 1.04 * W) & (ey > -0.04 * H) & (ey < 1.04 * H)
    probe = make_splats(W, H, ex[ok], ey[ok], sigl[ok], 1e-4, theta[ok], lg[ok], rng=rng)
    return np.concatenate([front, blockers, fin, probe]), pixel_uniforms(W, H), W, H


def degenerate_conic_scene(oracle, seed=0):
    """Extreme scales (the 0.3 px^2 floor .. 1e4 px) and anisotropy: at 45 degrees the projected covariance's determinant
    cancels in f32 (conics that fail the kernels' positive-definiteness test: such an entry must be kept), axis-aligned the
    conic has a tiny cx or cz (the rcp in block_qmin is huge); over a half-transparent front layer, so that blocks stay live.
    (No non-finite records: a NaN colour reaches a FINAL pixel's f32 accumulator as cond * NaN = NaN when the entry is
    evaluated there, so the culls and the early exit change such pixels by design; test_non_finite_splats covers them.)"""
    W, H = 77, 61
    rng = np.random.Generator(np.random.Philox(key=[4103, seed]))
    parts = [make_splats(W, H, [W / 2.0], [H / 2.0], HUGE, HUGE, 0.0, opacity_logits(oracle, [0.6]), color=[[0.3, 0.1, -0.2]])]
    k = 160
    sigl = np.exp(rng.uniform(0.0, np.log(1e4), k))
    theta = np.where(np.arange(k) % 2 == 0, np.pi / 4 + rng.uniform(-1e-3, 1e-3, k), np.where(np.arange(k) % 4 == 1, 0.0, np.pi / 2))
    parts.append(make_splats(W, H, rng.uniform(0, W, k), rng.uniform(0, H, k), sigl, 1e-4, theta, rng.uniform(-5.5, 4.0, k).astype(np.float32), rng=rng))
    k = 24  # both axes at the floor, and both huge at 45 degrees
    parts.append(make_splats(W, H, rng.uniform(0, W, k), rng.uniform(0, H, k), np.where(np.arange(k) < 12, 1e-4, 1e4),
                             np.where(np.arange(k) < 12, 1e-4, 5e3), np.pi / 4, rng.uniform(-5.5, 4.0, k).astype(np.float32), rng=rng))
    return np.concatenate(parts), pixel_uniforms(W, H), W, H


SCENES = {"transmittance_edge": transmittance_edge_scene, "live_box": live_box_scene, "degenerate_conic": degenerate_conic_scene}
SLAB_COLS = {8: (3, 9), 16: (2, 5), 32: (1, 3)}         # one tile-column slab per tile size (px0 != 0, the right edge included)


def margin_scene(oracle, name):
    """(splats, uniforms, W, H) of one of SCENES."""
    return cached(("margin_scene", name), lambda: SCENES[name](oracle))


def margin_ref(oracle, name, ts, cols=None):
    s, u, W, H = margin_scene(oracle, name)
    return oracle_frame(oracle, name, s, u, W, H, ts, cols=cols, want_illcond=True)


# ---- the margin scene of the tight binning (test_tight_margins.py, test_tight_host.py), built in pixel space ------------------------
# gs_tight.h drops an instance before the blend sees it; each of its tests is conservative by an explicit margin.  The scene puts
# the alpha = 1/255 contour within 1e-7 .. 1e-2 of the pixels a tile or a sub-block hangs on, the ellipse's extreme points on the
# strip boundaries, conics at the cancellation threshold, opacities at 1/255 and the aliased column, in labelled families.
TIGHT_FAMILIES = ("contour", "extreme_x", "extreme_y", "cancellation", "opacity_floor", "alias")
TIGHT_W, TIGHT_H = 500, 116  # 62.5 x 14.5 blocks: partial blocks and tiles at the right and bottom edges at every tile size


def pixel_ellipse(W, H, sig_long, sig_short, theta):
    """make_splats' (sig_long, sig_short, theta) for which the PIXEL-space covariance (before the +0.3 px^2) has standard deviations
    sig_long, sig_short along axes rotated by theta: make_splats scales the world axes by W/2 and H/2, so on a non-square canvas
    its own parameters name another ellipse."""
    sl, ss, th = (np.asarray(a, np.float64) for a in np.broadcast_arrays(sig_long, sig_short, theta))
    c, s = np.cos(th), np.sin(th)
    jx, jy = W / 2.0, H / 2.0
    M = np.empty(sl.shape + (2, 2))
    M[..., 0, 0] = (sl * sl * c * c + ss * ss * s * s) / (jx * jx)
    M[..., 0, 1] = M[..., 1, 0] = (sl * sl - ss * ss) * s * c / (jx * jy)
    M[..., 1, 1] = (sl * sl * s * s + ss * ss * c * c) / (jy * jy)
    w, v = np.linalg.eigh(M)
    return np.sqrt(w[..., 1]) * jx, np.sqrt(np.maximum(w[..., 0], 1e-16)) * jy, np.arctan2(v[..., 1, 1], v[..., 0, 1])


def tight_geometry(gdata, W, H):
    """f64 (gx, gy, cx, cy, cz, ln(255 op)) of the oracle's records: the centre is the f32 product the blend forms."""
    g = gdata_f32(gdata)
    with np.errstate(all="ignore"):
        return ((g[:, 0] * F(W)).astype(np.float64), (g[:, 1] * F(H)).astype(np.float64), g[:, 4].astype(np.float64),
                g[:, 5].astype(np.float64), g[:, 6].astype(np.float64), np.log(255.0 * g[:, 11].astype(np.float64)))


def block_qmin_pixels(gx, gy, cx, cy, cz, W, H):
    """[n, blocks down, blocks across]: the f64 minimum over the in-canvas PIXELS of every 8x8 block of
    q = 0.5 (cx dx^2 + cz dy^2) + cy dx dy, d = centre - pixel."""
    nbx, nby = -(-W // 8), -(-H // 8)
    px, py = np.arange(nbx * 8, dtype=np.float64), np.arange(nby * 8, dtype=np.float64)
    out = np.empty((np.size(gx), nby, nbx))
    for i in range(0, np.size(gx), 32):
        k = slice(i, i + 32)
        dx = gx[k, None, None] - px[None, None, :]
        dy = gy[k, None, None] - py[None, :, None]
        q = 0.5 * (cx[k, None, None] * dx * dx + cz[k, None, None] * dy * dy) + cy[k, None, None] * dx * dy
        q[:, :, W:] = np.inf
        q[:, H:, :] = np.inf
        out[k] = q.reshape(q.shape[0], nby, 8, nbx, 8).min(axis=(2, 4))
    return out


def facing_corner(gx, gy, W, H):
    """[n, blocks down, blocks across]: the block is the corner block of its 32-pixel tile (so of its 16-pixel tile too) on the
    side that faces the centre (gx, gy), the canvas's partial last tiles included."""
    nbx, nby = -(-W // 8), -(-H // 8)

    def side(c, nb):
        b = np.arange(nb)
        first, last = (b % 4 == 0), (b % 4 == 3) | (b == nb - 1)
        lo, hi = c[:, None] < 8.0 * b[None, :], c[:, None] > 8.0 * b[None, :] + 7.0
        return np.where(lo, first[None, :], np.where(hi, last[None, :], True))
    return side(gy, nby)[:, :, None] & side(gx, nbx)[:, None, :]


def _land_on_blocks(oracle, rng, s, W, H, allow=None, corner_share=0.0, decades=(-7.0, -2.0)):
    """Sets the opacity of every record of s so that ln(255 op) = qmin + delta for one 8x8 block of its reference rect (tile 8) whose
    f64 pixel minimum of q lies in (0.2, 5.5): delta = +-10^U(decades) max(1, qmin).  allow(bx, by) restricts the blocks; a
    corner_share of the records tries the tiles' corner blocks facing the centre first, and every record prefers a block the
    contour touches at a pixel (below).  Returns (keep, block x, block y)."""
    n = s.shape[0]
    u = pixel_uniforms(W, H)
    gd = oracle.preprocess(s, u, W, H, 8)[0]
    gx, gy, cx, cy, cz, _ = tight_geometry(gd, W, H)
    nbx, nby = -(-W // 8), -(-H // 8)
    qm = block_qmin_pixels(gx, gy, cx, cy, cz, W, H)
    bx, by = np.arange(nbx)[None, None, :], np.arange(nby)[None, :, None]
    r = gd[:, 12:16].astype(np.int64)
    ok = (qm > 0.2) & (qm < 5.5) & (bx >= r[:, 0, None, None]) & (bx < r[:, 2, None, None]) & (by >= r[:, 1, None, None]) & (by < r[:, 3, None, None])
    if allow is not None:
        ok &= allow(bx, by)
    # a block is TOUCHED at a pixel when the minimum of q over its pixels is the minimum over their bounding box too: the contour
    # then meets the box at that pixel, where the strip and column tests of gs_tight.h have nothing but their margins to spare
    # (touched[ts]: the same with the box of the block's whole ts-pixel tile: the tile, or the 16-pixel sub-block, hangs on that pixel)
    e = lambda a: a[:, None, None]
    touched = {}
    for ts in (8, 16, 32):
        x0, y0 = float(ts) * (8 * bx // ts), float(ts) * (8 * by // ts)
        x1, y1 = np.minimum(x0 + ts - 1.0, W - 1.0), np.minimum(y0 + ts - 1.0, H - 1.0)
        box = box_qmin_f64(e(cx), e(cy), e(cz), e(gx) - x1, e(gx) - x0, e(gy) - y1, e(gy) - y0)
        touched[ts] = ok & (qm - box <= 1e-9 * np.maximum(1.0, qm))
    corner = ok & facing_corner(gx, gy, W, H)
    want_corner = rng.uniform(size=n) < corner_share
    pick = rng.uniform(size=n)
    sign = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    mag = 10.0 ** rng.uniform(decades[0], decades[1], n)
    keep = np.zeros(n, bool)
    tbx, tby = np.zeros(n, np.int64), np.zeros(n, np.int64)
    target = np.full(n, 1.0 / 255.0)
    for i in range(n):
        pools = ([corner[i] & touched[32][i], corner[i] & touched[8][i], corner[i]] if want_corner[i] else []) + [touched[32][i], touched[16][i], touched[8][i], ok[i]]
        cand = next((np.argwhere(p) for p in pools if p.any()), None)
        if cand is None:
            continue
        tby[i], tbx[i] = cand[int(pick[i] * len(cand))]
        q = qm[i, tby[i], tbx[i]]
        op = np.exp(q + sign[i] * mag[i] * max(1.0, q)) / 255.0
        if op < 0.999:
            keep[i], target[i] = True, op
    s[:, 12] = opacity_logits(oracle, target)
    return keep, tbx, tby


def _extreme_centres(rng, cx, cy, cz, L, W, H, vertical):
    """Centres that put the rightmost / leftmost (vertical: topmost / bottommost) point of E = {q <= L} within +-10^U(-3, log 0.3)
    px of a strip boundary row (a multiple of 8; vertical: the first or last pixel row of a tile) and of the first or last pixel
    centre of an 8-pixel column (vertical: of a pixel column).  Returns (px, py, keep): a splat whose centre would leave the canvas
    for every boundary and both signs is not placed."""
    n = cx.size
    D = cx * cz - cy * cy
    if vertical:
        ey = np.sqrt(2.0 * L * cx / D)
        ex = -cy * ey / cx
    else:
        ex = np.sqrt(2.0 * L * cz / D)
        ey = -cy * ex / cz  # dy = -cy xmax / cz
    nbx, nby = -(-W // 8), -(-H // 8)
    px, py, keep = np.zeros(n), np.zeros(n), np.zeros(n, bool)
    rows = 8.0 * np.arange(1, nby) if not vertical else np.concatenate([8.0 * np.arange(1, nby), 8.0 * np.arange(1, nby) - 1.0])
    cols = (np.concatenate([8.0 * np.arange(nbx), np.minimum(8.0 * np.arange(nbx) + 7.0, W - 1.0)]) if not vertical
            else np.arange(W, dtype=np.float64))
    for i in range(n):
        opts = [(X, Y, sg) for sg in (-1.0, 1.0) for Y in rows if 0.0 < Y + sg * ey[i] < H - 1.0
                for X in cols[rng.integers(cols.size, size=3)] if 0.0 < X + sg * ex[i] < W - 1.0]
        if not opts:
            continue
        X, Y, sg = opts[int(rng.integers(len(opts)))]
        eps = rng.choice([-1.0, 1.0], 2) * 10.0 ** rng.uniform(-3.0, np.log10(0.3), 2)
        px[i], py[i], keep[i] = X + eps[0] + sg * ex[i], Y + eps[1] + sg * ey[i], True  # the point is at centre - d
    return px, py, keep


def _tip_centres(rng, cx, cy, cz, L, W, H):
    """Centres for thin diagonal splats near the cancellation threshold, aimed at tight_strip's `dyR +- eR` branches.  gs_tight.h works
    with three nested ellipses: the exact E, the chords' (discriminant inflated by 1e-5 of its terms S = cx cz + cy^2) and the
    extents' (Dlo = D - 1.14e-5 S), whose rightmost point is the dyR it compares with the strip.  Where S / D is in the thousands the
    extents' rightmost point lies ABOVE the chords' topmost point.  A strip boundary row between the two sees no chord there, and
    only eR tells the strip that it holds the extreme point.  The boundary row is a multiple of 32 (a boundary at every tile size)
    and the exact tip ends 0.5 .. 6 px past a multiple-of-32 column, so that the tip's pixels are a tile of their own.  Returns
    (px, py, keep); a conic without such a window, or whose centre would leave the canvas, is not placed."""
    n = cx.size
    S, D = cx * cz + cy * cy, cx * cz - cy * cy
    Dc, Dlo, lim2 = D - 1.0e-5 * S, D - 1.14e-5 * S, 2.0 * (L + 0.01)
    px, py, keep = np.zeros(n), np.zeros(n), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        top_c = np.sqrt(lim2 * 1.00001 * cx / Dc)                                            # the chords' topmost dy
        dyr = np.abs(cy) / cz * (np.sqrt(lim2 * 1.0001 * cz / Dlo) * 1.0002 + 0.02)          # |dyR| of tight_setup
        xs = np.sqrt(2.0 * L * cz / D)                                                       # the exact tip: (xs, -cy xs / cz)
        ys = np.abs(cy) * xs / cz
    for i in range(n):
        if not (Dlo[i] > 0.3 * D[i] and dyr[i] > top_c[i] + 0.05):
            continue
        b = top_c[i] + rng.uniform(0.15, 0.85) * (dyr[i] - top_c[i])
        opts = [(Y, sg) for sg in (-1.0, 1.0) for Y in 32.0 * np.arange(1, -(-H // 32)) if 0.0 < Y + sg * b < H - 1.0 and 0.0 <= Y + sg * (b - ys[i]) <= H - 1.0]
        if not opts:
            continue
        Y, sg = opts[int(rng.integers(len(opts)))]
        right = sg == -np.sign(cy[i])  # the extreme point at dy of sign sg is the rightmost in d = centre - pixel: it points to -x on screen
        dtip = xs[i] if right else -xs[i]
        cols = [X for X in 32.0 * np.arange(1, -(-W // 32)) if 0.0 < X + dtip < W - 1.0]
        if not cols:
            continue
        X = cols[int(rng.integers(len(cols)))]
        tip = X - 1.0 - rng.uniform(0.5, 6.0) if right else X + rng.uniform(0.5, 6.0)
        px[i], py[i], keep[i] = tip + dtip, Y + sg * b, True
    return px, py, keep


def _angles(rng, n):
    """Thirds: generic, within +-0.3 of 45 degrees (either diagonal), within +-0.05 of the axes."""
    k = np.arange(n) % 3
    diag = np.pi / 4 + np.pi / 2 * rng.integers(2, size=n) + rng.uniform(-0.3, 0.3, n)
    axis = np.pi / 2 * rng.integers(2, size=n) + rng.uniform(-0.05, 0.05, n)
    return np.where(k == 0, rng.uniform(0.0, np.pi, n), np.where(k == 1, diag, axis))


def tight_margin_scene(oracle, seed=0):
    """The labelled margin scene of the tight binning.  Returns a dict: splats, uniforms, W, H, family (index into TIGHT_FAMILIES
    per splat), block (the 8x8 block a splat's opacity was landed on, -1: none), drawn (per family, and for the tip-placed part of
    the cancellation family: how many splats the construction drew and how many it could place)."""
    W, H = TIGHT_W, TIGHT_H
    rng = np.random.Generator(np.random.Philox(key=[4201, seed]))
    u = pixel_uniforms(W, H)
    FLOOR = 1e-4  # a pixel-space deviation far below the projection's 0.3 px^2
    parts, fam, blocks, drawn = [], [], [], {}

    def records(px, py, sl, ss, th, logit=0.0):
        a, b, t = pixel_ellipse(W, H, sl, ss, th)
        return make_splats(W, H, px, py, a, b, t, logit, rng=rng)

    def conics(sl, ss, th, op):
        s = records(np.full(np.size(sl), W / 2.0), np.full(np.size(sl), H / 2.0), sl, ss, th, opacity_logits(oracle, op))
        return s, tight_geometry(oracle.preprocess(s, u, W, H, 8)[0], W, H)

    def add(name, s, keep, tb=None):
        drawn[name] = (int(keep.size), int(keep.sum()))
        parts.append(s[keep])
        fam.append(np.full(int(keep.sum()), TIGHT_FAMILIES.index(name)))
        blocks.append(np.stack([tb[0][keep], tb[1][keep]], axis=1) if tb is not None else np.full((int(keep.sum()), 2), -1))

    # contour on a block
    n = 520
    sl = np.exp(rng.uniform(np.log(2.0), np.log(300.0), n))
    ss = np.where(rng.uniform(size=n) < 0.4, FLOOR, np.exp(rng.uniform(np.log(0.3), np.log(sl))))
    s = records(rng.uniform(-0.03 * W, 1.03 * W, n), rng.uniform(-0.03 * H, 1.03 * H, n), sl, ss, _angles(rng, n))
    keep, tbx, tby = _land_on_blocks(oracle, rng, s, W, H, corner_share=0.6)
    add("contour", s, keep, (tbx, tby))
    # extreme points on the strip boundaries, in x and in y
    for name, n, vertical in (("extreme_x", 130, False), ("extreme_y", 100, True)):
        sl = np.exp(rng.uniform(np.log(3.0), np.log(20.0), n))
        ss = np.where(rng.uniform(size=n) < 0.6, FLOOR, np.exp(rng.uniform(np.log(0.3), np.log(sl))))
        th = rng.uniform(0.08, np.pi / 2 - 0.08, n) + np.pi / 2 * rng.integers(2, size=n)
        s, (_, _, cx, cy, cz, L) = conics(sl, ss, th, np.exp(rng.uniform(0.5, 4.0, n)) / 255.0)
        px, py, keep = _extreme_centres(rng, cx, cy, cz, L, W, H, vertical)
        s[:, 0], s[:, 1] = 2.0 * px / W - 1.0, 2.0 * py / H - 1.0
        add(name, s, keep)
    # cancellation threshold: thin at 45 degrees, the long axis swept across Dlo > 0.25 D, the opacity landed on a block
    n = 400
    sl = np.exp(rng.uniform(np.log(30.0), np.log(400.0), n))
    th = np.pi / 4 + np.pi / 2 * rng.integers(2, size=n) + rng.uniform(-0.03, 0.03, n)
    s = records(rng.uniform(-0.03 * W, 1.03 * W, n), rng.uniform(-0.03 * H, 1.03 * H, n), sl, FLOOR, th)
    keep, tbx, tby = _land_on_blocks(oracle, rng, s, W, H, corner_share=0.6, decades=(-7.0, -4.5))
    # ... and a part of them placed by their extreme point (the opacity drawn, the centre placed: _tip_centres)
    # S / D of a thin splat is about sl^2 sin^2 cos^2 / 0.15: drawn in 8e3 .. 5e4, with the angle between 15 and 45 degrees of either
    # axis direction and the opacity such that the tip lies 25 .. 80 px above or below the centre (the canvas is 116 px high)
    k = 150
    ratio, th = np.exp(rng.uniform(np.log(8.0e3), np.log(5.0e4), k)), rng.uniform(0.26, 0.78, k)
    sl = np.sqrt(0.15 * ratio) / (np.sin(th) * np.cos(th))
    Lt = np.clip(0.5 * (rng.uniform(25.0, 80.0, k) / (sl * np.sin(th))) ** 2, 0.2, 3.0)
    th = np.where(rng.uniform(size=k) < 0.5, th, np.pi - th)
    s2, (_, _, cx, cy, cz, L) = conics(sl, FLOOR, th, np.exp(Lt) / 255.0)
    px, py, keep2 = _tip_centres(rng, cx, cy, cz, L, W, H)
    s2[:, 0], s2[:, 1] = 2.0 * px / W - 1.0, 2.0 * py / H - 1.0
    drawn["cancellation_tips"] = (k, int(keep2.sum()))
    add("cancellation", np.concatenate([s, s2]), np.concatenate([keep, keep2]),
        (np.concatenate([tbx, np.full(k, -1)]), np.concatenate([tby, np.full(k, -1)])))
    # opacity at 1/255: ln(255 op) in [-0.02, 0.02], centres on corner pixels of tiles and sub-blocks and half a pixel off them
    n = 100
    sl = np.exp(rng.uniform(np.log(0.05), np.log(0.9), n))
    ss = np.where(rng.uniform(size=n) < 0.5, FLOOR, sl * rng.uniform(0.3, 1.0, n))
    px = np.minimum(8.0 * rng.integers(-(-W // 8), size=n) + 7.0 * rng.integers(2, size=n), W - 1.0) + 0.5 * rng.integers(2, size=n)
    py = np.minimum(8.0 * rng.integers(-(-H // 8), size=n) + 7.0 * rng.integers(2, size=n), H - 1.0) + 0.5 * rng.integers(2, size=n)
    s = records(px, py, sl, ss, rng.uniform(0.0, np.pi, n), opacity_logits(oracle, np.exp(rng.uniform(-0.02, 0.02, n)) / 255.0))
    add("opacity_floor", s, np.ones(n, bool))
    # aliased column: the rect reaches column ntx, a long near-horizontal axis reaches, misses or just reaches the first columns
    n = 100
    free = np.arange(n) % 10 >= 7  # three in ten keep a free opacity (far misses and plain reaches), the others land on a block
    sl = np.where(free, rng.uniform(140.0, 260.0, n), rng.uniform(190.0, 260.0, n))
    ss = np.where(rng.uniform(size=n) < 0.4, FLOOR, np.exp(rng.uniform(np.log(0.3), np.log(6.0), n)))
    px, py = rng.uniform(W - 12.0, 1.045 * W, n), rng.uniform(0.0, H, n)
    s = records(px, py, sl, ss, rng.uniform(-0.05, 0.05, n))
    near = rng.uniform(size=n) < 0.5
    keep, tbx, tby = _land_on_blocks(oracle, rng, s, W, H, allow=lambda bx, by: bx < np.where(near, 1, 4)[:, None, None])
    s[free, 12] = opacity_logits(oracle, np.exp(rng.uniform(0.1, 5.5, int(free.sum()))) / 255.0)
    tbx[free] = tby[free] = -1
    add("alias", s, keep | free, (tbx, tby))
    return {"splats": np.concatenate(parts), "uniforms": u, "W": W, "H": H, "family": np.concatenate(fam), "block": np.concatenate(blocks),
            "drawn": drawn}


TIGHT_SCENES = {"tight_margins": tight_margin_scene}


def tight_scene(oracle, name="tight_margins"):
    return cached(("tight_scene", name), lambda: TIGHT_SCENES[name](oracle))


def tight_ref(oracle, name, ts, cols=None):
    t = tight_scene(oracle, name)
    return oracle_frame(oracle, name, t["splats"], t["uniforms"], t["W"], t["H"], ts, cols=cols, want_illcond=True)


# ---- the cases of gs_pick (test_pick.py), which the coverage tests fold per splat ---------------------------------------------------
def lattice(W, H, x0, dx, y0, dy):
    return np.array([(x, y) for y in range(y0, H, dy) for x in range(x0, W, dx)], np.uint32)


def weight_ties_scene(oracle):
    """16 pairs of splats centred on 16 pixels of a 64 x 64 canvas (pixel space, all at depth 1: list order = record order).  At
    its centre pixel a splat has power = 0, so alpha is its opacity a.  The front splat of pair k gets an opacity a_k in
    [0.26, 0.33) and the one behind it the f32 opacity b_k with fl(b_k fl(1 - a_k)) == a_k (one exists: b steps by one ulp, the
    product by less than an ulp of a): the two weights a_k * 1 and b_k * T are then the same f32.  Returns (splats, uniforms, W, H,
    centres); whether the ties came about is asserted on the restatement, not assumed."""
    W = H = 64
    u = pixel_uniforms(W, H)

    def opacities(logits):
        s = make_splats(W, H, np.full(logits.size, 32.0), np.full(logits.size, 32.0), 4.0, 4.0, 0.0, logits)
        return oracle.preprocess(s, u, W, H, 8)[0][:, 11].view(np.float32).copy()

    cx = np.array([8 + 16 * i for j in range(4) for i in range(4)], np.float64)
    cy = np.array([8 + 16 * j for j in range(4) for i in range(4)], np.float64)
    la = opacity_logits(oracle, np.linspace(0.26, 0.33, 16))
    a = opacities(la)
    b = np.zeros_like(a)
    for k in range(a.size):
        c = F(a[k] / F(F(1.0) - a[k]))
        near = [c]
        for _ in range(4):
            near = [np.nextafter(near[0], F(0.0), dtype=F)] + near + [np.nextafter(near[-1], F(2.0), dtype=F)]
        hit = [v for v in near if F(v * F(F(1.0) - a[k])) == a[k]]
        b[k] = hit[0] if hit else c
    lb = opacity_logits(oracle, b.astype(np.float64))  # (the largest reachable opacity <= b: b itself for most pairs)
    s = make_splats(W, H, np.repeat(cx, 2), np.repeat(cy, 2), 1.5, 1.5, 0.0, np.stack([la, lb], axis=1).ravel(),
                    rng=np.random.default_rng(5))
    return s, u, W, H, np.stack([cx, cy], axis=1).astype(np.uint32)


def pick_case(oracle, name, ts):
    """(splats, uniforms, W, H, oracle frame, query pixels) of one case: config A, the ragged golden, a margin scene or
    "weight_ties"."""
    def make():
        if name == "cfgA":
            s, u, W, H = state_scene("cfgA")
            ref = oracle_frame(oracle, name, s, u, W, H, ts)
            xy = lattice(W, H, 5, 13, 3, 17)
        elif name == "ragged":
            from gsplat import synth
            z = np.load(os.path.join(GOLDEN, "ragged_3001_200x120_t8.npz"))
            n, W, H, gts, _ = (int(v) for v in z["params"])
            assert gts == ts
            s, u = synth.bicycle_like(n), z["uniforms"]
            gdata, _ = oracle.preprocess(s, u, W, H, ts)
            assert hashlib.sha256(np.ascontiguousarray(gdata).tobytes()).hexdigest() == str(z["gdata_sha256"])
            ref = {"gdata": gdata, "sorted_values": z["sorted_values"], "ranges": z["ranges"]}
            xy = lattice(W, H, 2, 7, 1, 5)
        elif name == "weight_ties":
            s, u, W, H, centres = weight_ties_scene(oracle)
            ref = oracle_frame(oracle, name, s, u, W, H, ts)
            xy = np.concatenate([centres, lattice(W, H, 2, 7, 1, 5)])
        else:
            s, u, W, H = margin_scene(oracle, name)
            ref = margin_ref(oracle, name, ts)
            xy = lattice(W, H, 2, 7, 1, 5)
        return s, u, W, H, ref, xy
    return cached(("pick_case", name, ts), make)


# ---- records with special floats, and a guarded export (test_export.py, test_transform.py) -----------------------------------------
def special(rec):
    """A copy with a handful of floats overwritten by a NaN, a payload NaN, -0.0, +-inf and a denormal (carried floats), and the
    padding floats of two records filled with junk that must NOT come back."""
    out = np.array(rec, dtype=F, copy=True).reshape(-1, 80)
    w = out.view(np.uint32)
    n = out.shape[0]
    vals = [0x7FC00000, 0x7FA12345, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0xFFC0BEEF]
    slots = [0, 5, 9, 12, 16, 18, 17 + 4 * 15, 4, 2, 22]
    for k, v in enumerate(vals * 2):
        w[(k * 7) % n, slots[k % len(slots)]] = v
    w[0, er.PADDING] = 0xA5A5A5A5
    w[n - 1, er.PADDING] = 0x3F800000
    return out


def special_records(n):
    """n records of synth.bicycle_like (the ragged fixture's own scene for 3001) with the special floats."""
    def make():
        from gsplat import synth
        return special(synth.bicycle_like(3001) if n == 3001 else scene(10000)[:n])
    return cached(("special_records", n), make)


def guarded(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8).fill(0xA5)
    return a


def is_fill(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xA5).all())


def raw_export(r, mask, value, with_ids, device=False):
    """gs_export_splats[_device] into buffers one record and one id longer than needed, pre-filled with 0xA5; returns (records,
    ids or None) after checking the guards."""
    from gsplat import _abi
    L = _abi.load()
    n = ctypes.c_uint64()
    _abi.check(L.gs_export_splats(r._ctx, mask, value, None, 0, ctypes.byref(n), None))
    m = n.value
    if device:
        import torch
        rec_t = torch.full((m + 1, 80), 0, dtype=torch.float32, device="cuda")
        rec_t.view(torch.uint8).fill_(0xA5)
        ids_t = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
        ids_t.view(torch.uint8).fill_(0xA5)
        torch.cuda.synchronize()
        n2 = ctypes.c_uint64()
        _abi.check(L.gs_export_splats_device(r._ctx, mask, value, rec_t.data_ptr(), m + 1, ctypes.byref(n2), ids_t.data_ptr() if with_ids else None))
        rec, ids = rec_t.cpu().numpy(), ids_t.cpu().numpy().view(np.uint32)
    else:
        rec, ids = guarded((m + 1, 80), F), guarded(m + 1, np.uint32)
        n2 = ctypes.c_uint64()
        _abi.check(L.gs_export_splats(r._ctx, mask, value, rec.ctypes.data, m + 1, ctypes.byref(n2), ids.ctypes.data if with_ids else None))
    assert n2.value == m
    assert is_fill(rec[m:]) and is_fill(ids[m:])
    if not with_ids:
        assert is_fill(ids)
    return rec[:m], (ids[:m] if with_ids else None)


# ---- renderers and frames ----------------------------------------------------------------------------------------------------------
def mk(s, W, H, ts, exact=False, state=False, aux=False, cols=None, flags=0, **kw):
    """gpu_checks.make_renderer with the feature flags by name; a test file binds its own defaults with functools.partial."""
    from gpu_checks import make_renderer
    from gsplat import _abi
    fl = (flags | (_abi.GS_FLAG_EXACT_BLEND if exact else 0) | (_abi.GS_FLAG_SPLAT_STATE if state else 0) |
          (_abi.GS_FLAG_AUX_OUTPUTS if aux else 0))
    return make_renderer(s, W, H, ts, flags=fl, cols=cols, **kw)


def code_of(fn):
    """(code, message) of the GsError fn() must raise."""
    from gsplat import _abi
    with pytest.raises(_abi.GsError) as e:
        fn()
    return e.value.code, str(e.value)


def timeless(st):
    """stats() without what a clock measured."""
    return {k: v for k, v in st.items() if k not in ("frame_us", "frame_us_mean", "frames_timed", "stage_us", "stage_us_mean")}


TAPS = ("TILE_COUNTS", "GAUSSIAN_DATA", "KEYS", "VALUES", "RANGES")


def frame_taps(r, u, debug):
    """One frame: its TAPS, the image and the f32 tap."""
    from gsplat import _abi
    r.render_uniforms(u, debug=debug)
    r.wait()
    out = {t: r.read_buffer(getattr(_abi, "GS_BUF_" + t)) for t in TAPS}
    out["rgba8"] = r.read_rgba8()
    out["rgbf"] = r.read_buffer(_abi.GS_BUF_RGB_F32)
    return out


# ---- the other hosts ---------------------------------------------------------------------------------------------------------------
def run_node(script, args, timeout=300):
    """Runs tests/js/<script> under Node with `args`; returns the JSON on the last line of its output."""
    res = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", script)] + [str(a) for a in args], capture_output=True, text=True,
                         timeout=timeout)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def c_layout(tmp_path, name, body):
    """Compiles the statements `body` (printfs of sizeof / offsetof / constants) into a C program against gs_abi.h, runs it and
    returns the integers it prints."""
    src, exe = tmp_path / (name + ".c"), tmp_path / name
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsplat/gs_abi.h"\nint main(void){' + body + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [int(x) for x in subprocess.check_output([str(exe)]).split()]


HostSources = collections.namedtuple("HostSources", "rjs idx dts napi hdr")


def host_sources():
    """The texts of js/renderer.js, js/index.js, js/index.d.ts, csrc/napi/gs_napi.c and gs_abi.h, read once."""
    def make():
        paths = [os.path.join(JS_DIR, f) for f in ("renderer.js", "index.js", "index.d.ts")] + [NAPI_SRC, HEADER]
        return HostSources(*(open(p).read() for p in paths))
    return cached("host_sources", make)
