"""The blend's two parking culls at their margins, in every blend kernel.

An entry is parked (evaluated for a block's pixels) only if (1) its alpha >= 1/255 ellipse reaches the bounding box of the block's
LIVE pixels (`block_qmin` against ln(255 op) + 0.01, with 1e-5 of the terms' magnitude on q) and (2) Tmax (1 - alpha_lo) over
that box is not below 0.0000999 (alpha_lo = 0.99 min(0.99, op exp(-qmax))).  Both are meant to skip only work that cannot change a
pixel.  The scenes below are built in pixel space (identity view and projection, focal W/2, H/2, centres in pixels, one depth
bucket so that the list order is the splat order) and aim at the margins of the two decisions:

  * transmittance_edge_scene: T brought to just above the final threshold (1.0039e-4) by huge, near-uniform splats, then a sweep
    of entries whose T (1 - alpha) lands at 1e-4 (1 +- delta), and entries at the 0.99 clamp;
  * live_box_scene: most pixels of a block finished, one corner / one row / one column / two opposite corners left live, then
    thin (eigenvalue ratio >= 1e3), rotated splats whose alpha = 1/255 contour passes just inside or just outside the live box;
  * degenerate_conic_scene: extreme scales and anisotropy at 45 degrees (conics that are not positive definite in f32, tiny cx or
    cz).

Every scene PROVES that it reaches its margins (unmarked tests, they run in the CPU suite): `replay_blocks` replays the oracle's
EXACT blend per 8x8 block in f32 and records, per (block, entry), the live set, its box, Tmax, the f64 minimum of q over the box
against ln(255 op) and Tmax (1 - alpha_min).  The GPU tests then render each scene with the culls on and off
(GS_OPT_BLEND_ABLATION bit 2) in every blend kernel, binning and mode, against each other and against the oracle.
"""
import numpy as np
import pytest

C255 = np.float32(1.0 / 255.0)
F = np.float32


# ---- scene construction (pixel space) ------------------------------------------------------------------------------------------
def pixel_uniforms(W, H):
    u = np.zeros(40, dtype=np.float32)
    u[0] = u[5] = u[10] = u[15] = 1.0      # view = I (column-major)
    u[16] = u[21] = u[26] = u[31] = 1.0    # proj = I: ndc = pos
    u[35] = u[36] = 0.5                    # tan_fov
    u[37], u[38] = W / 2.0, H / 2.0        # focal: one world unit at depth 1 = W / 2 pixels
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


# ---- the replay --------------------------------------------------------------------------------------------------------------
def _box_qmin_f64(cx, cy, cz, dxlo, dxhi, dylo, dyhi):
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


def replay_blocks(ref, W, H, ts, cols=None):
    """Replays the oracle's EXACT blend (gs_oracle.c gso_blend, the kernels' EXACT expression tree) per tile in f32 and returns,
    per (8x8 block, list entry) whose block still has a live pixel before the entry, one row of:
      block, entry, nlive, Tmax, m_box = qmin(live box) - ln(255 op)  (f64; <= 0: the entry reaches alpha >= 1/255 in the box),
      m_pix = min over the live PIXELS of q - ln(255 op), r_T = Tmax (1 - alpha_min) / 1e-4 - 1 (f64, alpha over the live box),
      pd (the kernels' f32 positive-definiteness test), min(cx, cz), box area / live pixels.
    Also returns the replayed f32 image (it must equal the oracle's bit for bit) and the per-pixel T before each entry is not
    kept.  The per-entry live set is tighter than the kernels' per-batch one."""
    from oracle import np_oracle as npo
    ntx = int(np.ceil(F(W) / F(ts)))
    nty = int(np.ceil(F(H) / F(ts)))
    c0, c1 = cols if cols is not None else (0, ntx)
    g = gdata_f32(ref["gdata"])
    vals, rng = ref["sorted_values"], ref["ranges"]
    img = np.zeros((H, W, 3), np.float32)
    rows = []
    fin = F(1.0) - C255
    for ty in range(nty):
        for tx in range(c0, c1):
            tile = tx + ty * ntx
            start = int(rng[tile - 1]) if tile > 0 else 0
            end = int(rng[tile])
            ly, lx = np.meshgrid(np.arange(ts), np.arange(ts), indexing="ij")
            gx, gy = (tx * ts + lx).ravel(), (ty * ts + ly).ravel()
            inside = (gx < W) & (gy < H)
            blk = ((ly // 8) * (ts // 8) + lx // 8).ravel()
            pxf, pyf = gx.astype(F), gy.astype(F)
            T = np.ones(gx.size, F)
            acc = np.zeros((gx.size, 3), F)
            if end > start:
                rec = g[vals[start:end]]
                gxp = rec[:, 0] * F(W)
                gyp = rec[:, 1] * F(H)
                cx, cy, cz = rec[:, 4], rec[:, 5], rec[:, 6]
                op = rec[:, 11]
                with np.errstate(all="ignore"):
                    dx = gxp[:, None] - pxf[None, :]
                    dy = gyp[:, None] - pyf[None, :]
                    t1 = cx[:, None] * dx * dx
                    t2 = cz[:, None] * dy * dy
                    t3 = cy[:, None] * dx * dy
                    power = F(-0.5) * (t1 + t2) - t3
                    alpha = npo.wmin(F(0.99), op[:, None] * npo.expf(power))
                    pd = (cx > 0) & (cz > 0) & (cx * cz - cy * cy > 0)
                    lim0 = np.log(255.0 * op.astype(np.float64))
                    qpix = -power.astype(np.float64)
                for e in range(end - start):
                    live = inside & ~(T * fin < F(0.0001))
                    with np.errstate(all="ignore"):
                        for b in np.unique(blk[live]):
                            lb = live & (blk == b)
                            bx = gx[lb].astype(np.float64)
                            by = gy[lb].astype(np.float64)
                            x0, x1, y0, y1 = bx.min(), bx.max(), by.min(), by.max()
                            Tm = float(T[lb].max())
                            cxd, cyd, czd = float(cx[e]), float(cy[e]), float(cz[e])
                            ex, ey = float(gxp[e]), float(gyp[e])
                            if pd[e] and np.isfinite([cxd, cyd, czd, ex, ey]).all():
                                mb = _box_qmin_f64(cxd, cyd, czd, ex - x1, ex - x0, ey - y1, ey - y0) - lim0[e]
                                cs = [(ex - a) for a in (x0, x1)], [(ey - a) for a in (y0, y1)]
                                qmax = max(0.5 * (cxd * a * a + czd * c * c) + cyd * a * c for a in cs[0] for c in cs[1])
                                amin = min(0.99, float(op[e]) * np.exp(-qmax))
                                rT = Tm * (1.0 - amin) / 1e-4 - 1.0
                            else:
                                mb, rT = np.nan, np.nan
                            mp = float((qpix[e, lb] - lim0[e]).min()) if pd[e] else np.nan
                            area = (x1 - x0 + 1) * (y1 - y0 + 1) / lb.sum()
                            rows.append((tile * 64 + b, start + e, int(lb.sum()), Tm, mb, mp, rT, bool(pd[e]),
                                         float(min(cxd, czd)), area))
                    a = alpha[e]
                    test = T * (F(1.0) - a)
                    cond = ((power[e] <= 0) & (a >= C255) & (test >= F(0.0001))).astype(F)
                    for ch in range(3):
                        acc[:, ch] = acc[:, ch] + cond * rec[e, 8 + ch] * a * T
                    T = cond * test + (F(1.0) - cond) * T
            img[gy[inside], gx[inside]] = acc[inside]
    dt = np.dtype([("block", np.int64), ("entry", np.int64), ("nlive", np.int64), ("Tmax", np.float64), ("m_box", np.float64),
                   ("m_pix", np.float64), ("r_T", np.float64), ("pd", bool), ("cmin", np.float64), ("sparse", np.float64)])
    return np.array(rows, dtype=dt), img


# ---- the scenes ------------------------------------------------------------------------------------------------------------
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
        q = _box_qmin_f64(cx, cy, cz, ex - bx[:, 3], ex - bx[:, 2], ey - bx[:, 5], ey - bx[:, 4])
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
_CACHE = {}


def _scene(oracle, name):
    if name not in _CACHE:
        _CACHE[name] = SCENES[name](oracle)
    return _CACHE[name]


def _ref(oracle, name, ts, cols=None):
    key = (name, ts, cols)
    if key not in _CACHE:
        s, u, W, H = _scene(oracle, name)
        _CACHE[key] = oracle.render(s, u, W, H, ts, cols=cols, want_illcond=True)
    return _CACHE[key]


def _replay(oracle, name):
    key = (name, "replay")
    if key not in _CACHE:
        s, u, W, H = _scene(oracle, name)
        ref = _ref(oracle, name, 8)
        rows, img = replay_blocks(ref, W, H, 8)
        np.testing.assert_array_equal(img.view(np.uint32), ref["rgbf"].view(np.uint32))  # the replay IS the oracle's blend
        _CACHE[key] = rows
    return _CACHE[key]


def _both_sides(v, d):
    """(pairs with v in [-d, 0), pairs with v in [0, d])"""
    return int(((v < 0) & (v >= -d)).sum()), int(((v >= 0) & (v <= d)).sum())


# ---- the scenes reach their margins (oracle only: CPU suite) ------------------------------------------------------------------
def test_transmittance_edge_scene_reaches_its_margins(oracle):
    rows = _replay(oracle, "transmittance_edge")
    rT = rows["r_T"]
    # the kernels cull when Tmax (1 - 0.99 alpha_lo) < 0.999e-4: entries at 1e-4 (1 +- delta) for every delta down to 3e-4,
    # on both sides of the exact decision T (1 - alpha) >= 1e-4
    for d, need in ((3e-2, 500), (3e-3, 300), (1e-3, 150), (3e-4, 60)):
        below, above = _both_sides(rT, d)
        assert below >= need and above >= need, (d, below, above)
    # Tmax is not most pixels' own T: most (block, entry) pairs have several live pixels
    assert (rows["nlive"] > 1).sum() > 0.5 * rows.size
    # the 0.99 clamp: entries with alpha 0.99 over blocks that are still live
    g = gdata_f32(_ref(oracle, "transmittance_edge", 8)["gdata"])
    ent = _ref(oracle, "transmittance_edge", 8)["sorted_values"][rows["entry"]]
    assert (g[ent, 11] >= 0.99).sum() >= 100


def test_live_box_scene_reaches_its_margins(oracle):
    rows = _replay(oracle, "live_box")
    mb, mp = rows["m_box"], rows["m_pix"]
    # min over the live box of q against ln(255 op): just inside (must park) and just outside (may skip) the alpha = 1/255 contour
    for d, need in ((1e-2, 150), (3e-3, 100), (1e-3, 60), (3e-4, 15)):
        below, above = _both_sides(mb, d)
        assert below >= need and above >= need, (d, below, above)
    # ... with the contour's inside on a live PIXEL (an entry there with alpha in [1/255, 1.01/255): a cull that drops it changes a bit)
    assert _both_sides(mp, 1e-2)[0] >= 100 and _both_sides(mp, 1e-3)[0] >= 40
    # every live set: one pixel, a row or column, two opposite corners (the box much larger than the live set), partial blocks
    near = np.abs(mb) <= 1e-2
    assert (near & (rows["nlive"] == 1)).sum() >= 30
    assert (near & (rows["nlive"] >= 3) & (rows["sparse"] == 1.0)).sum() >= 30
    assert (near & (rows["nlive"] == 2) & (rows["sparse"] >= 4.0)).sum() >= 10
    s, u, W, H = _scene(oracle, "live_box")
    ntx = int(np.ceil(W / 8))
    blk = rows["block"] // 64
    edge = ((blk % ntx) == ntx - 1) | ((blk // ntx) == int(np.ceil(H / 8)) - 1)
    assert (near & edge).sum() >= 10
    # the opacities just above 1/255, where lim = ln(255 op) is near 0
    g = gdata_f32(_ref(oracle, "live_box", 8)["gdata"])
    op = g[_ref(oracle, "live_box", 8)["sorted_values"][rows["entry"]], 11]
    assert (near & (op < 0.0045)).sum() >= 20


def test_degenerate_conic_scene_reaches_its_margins(oracle):
    rows = _replay(oracle, "degenerate_conic")
    ref = _ref(oracle, "degenerate_conic", 8)
    g = gdata_f32(ref["gdata"])
    fin = np.isfinite(g[:, :12]).all(axis=1)
    ent = ref["sorted_values"][rows["entry"]]
    # valid (finite) records whose conic fails the kernels' f32 test cx cz - cy^2 > 0 (an indefinite conic: a covariance
    # determinant that cancelled to a negative number), reaching live blocks: such an entry must be kept
    assert (~rows["pd"] & fin[ent]).sum() >= 20
    # tiny cx or cz (rcp huge in block_qmin) on live blocks
    assert (rows["pd"] & (rows["cmin"] < 1e-6)).sum() >= 500


# ---- the matrix (GPU) ---------------------------------------------------------------------------------------------------------
KERNELS = [(16, 0), (32, 0), (16, 8), (32, 8), (8, 0)]  # (tile, GS_OPT_BLEND_ABLATION): the quad kernel at 16 / 32, the workgroup-
                                                          # per-tile kernel at 16 / 32, gs_blend_kernel<8>
SLAB_COLS = {8: (3, 9), 16: (2, 5), 32: (1, 3)}         # one tile-column slab per tile size (px0 != 0, the right edge included)


def _frame(r, u, debug=False):
    from gsplat import _abi
    r.render_uniforms(u, debug=debug)
    r.wait()
    return (r.read_buffer(_abi.GS_BUF_RGB_F32, np.float32).copy(), r.read_rgba8(), r.stats())


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS, ids=["quad16", "quad32", "wg16", "wg32", "tile8"])
@pytest.mark.parametrize("name", list(SCENES))
def test_blend_culls_at_their_margins(oracle, name, kernel):
    """Every blend kernel, both binnings (gs_render tight = MASKED walkers; GS_OPT_TILE_CULL 0 and gs_render_debug = the reference's
    lists), EXACT and fused, the whole canvas and one tile-column slab: the frame with the culls (ablation bit 2 clear) equals the
    frame without them bit for bit, EXACT frames equal the oracle (lists included), fused frames are within the fused bounds, and
    the culls removed work."""
    from gsplat import _abi
    from gpu_checks import check_image, check_stages, make_renderer
    ts, abl = kernel
    s, u, W, H = _scene(oracle, name)
    for cols in (None, SLAB_COLS[ts]):
        ref = _ref(oracle, name, ts, cols)
        for flags, exact in ((_abi.GS_FLAG_EXACT_BLEND, True), (0, False)):
            r = make_renderer(s, W, H, ts, flags=flags, cols=cols)
            ev_on = ev_off = 0
            for tight, debug in ((1, False), (0, False), (0, True)):
                r.set_option(_abi.GS_OPT_TILE_CULL, tight)
                r.set_option(_abi.GS_OPT_BLEND_ABLATION, abl | 4)
                f_off, i_off, st_off = _frame(r, u, debug)
                r.set_option(_abi.GS_OPT_BLEND_ABLATION, abl)
                f_on, i_on, st_on = _frame(r, u, debug)
                cell = (name, ts, abl, cols, exact, tight, debug)
                assert st_on["tight_binning"] == (tight and not debug), cell
                np.testing.assert_array_equal(f_on.view(np.uint32), f_off.view(np.uint32), err_msg=str(cell))
                np.testing.assert_array_equal(i_on, i_off, err_msg=str(cell))
                if exact:  # every tap of a debug frame, the (subset) lists of a product frame, the image bit for bit
                    check_stages(r, ref, exact_image=True, debug=debug, oracle=oracle, W=W, H=H)
                else:  # these scenes put many decisions within rounding of their thresholds on purpose: flagged pixels abound
                    check_image(r, ref, False, max_ill=0.5)
                assert st_on["num_evaluated"] <= st_off["num_evaluated"], (cell, st_on["num_evaluated"], st_off["num_evaluated"])
                ev_on += st_on["num_evaluated"]
                ev_off += st_off["num_evaluated"]
            assert ev_on < ev_off, (name, ts, abl, cols, exact, ev_on, ev_off)  # the switch and the culls exist in this kernel
            r.destroy()
