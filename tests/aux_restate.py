"""CPU restatement of the blend with the two planes of GS_FLAG_AUX_OUTPUTS (include/gsplat/gs_abi.h).

Follows oracle/np_oracle.py::blend (compute_tiles.wgsl:30-75: the EXACT expression tree, one f32 rounding per operation, the
oracle's exp) and adds, with the colour's own entries, weights and association:
    alpha  A = 1 - T_final
    depth  D = D + cond * z * alpha * T   (left to right, in list order; z = GaussianData.depth, word 7)
Input: the C oracle's GaussianData, sorted values and ranges.  All tiles of the slab walk their lists in lock step (tiles
sorted by list length, the ones whose list has ended drop out of the slice), so every pixel sees exactly the operations the
per-tile loop of np_oracle.blend applies to it.
"""
import numpy as np

F = np.float32


def restate(gdata, sorted_values, rng, W, H, ts, cols=None):
    """Returns (rgbf f32 [H, W, 3], alpha f32 [H, W], depth f32 [H, W]); pixels outside the tile-column slab `cols` are 0."""
    from oracle import np_oracle as npo
    ntx = int(np.ceil(F(W) / F(ts)))
    nty = int(np.ceil(F(H) / F(ts)))
    c0, c1 = cols if cols is not None else (0, ntx)
    g = np.ascontiguousarray(gdata).view(np.float32).reshape(-1, 16)
    vals = np.asarray(sorted_values)
    rng = np.asarray(rng).astype(np.int64)
    tiles = np.array([tx + ty * ntx for ty in range(nty) for tx in range(c0, c1)], np.int64)
    start = np.where(tiles > 0, rng[np.maximum(tiles - 1, 0)], 0)
    length = rng[tiles] - start
    order = np.argsort(-length, kind="stable")
    tiles, start, length = tiles[order], start[order], length[order]
    ly, lx = np.meshgrid(np.arange(ts), np.arange(ts), indexing="ij")
    gx = ((tiles % ntx) * ts)[:, None] + lx.ravel()[None, :]
    gy = ((tiles // ntx) * ts)[:, None] + ly.ravel()[None, :]
    pxf, pyf = gx.astype(F), gy.astype(F)
    nt, npx = tiles.size, ts * ts
    T = np.ones((nt, npx), F)
    acc = np.zeros((3, nt, npx), F)
    D = np.zeros((nt, npx), F)
    c255 = F(1.0 / 255.0)
    with np.errstate(all="ignore"):
        for e in range(int(length.max(initial=0))):
            k = int(np.searchsorted(-length, -e, side="left"))  # tiles whose list still has entry e: the first k
            rec = g[vals[start[:k] + e]]
            gxp = (rec[:, 0] * F(W))[:, None]
            gyp = (rec[:, 1] * F(H))[:, None]
            cx, cy, cz, z, op = (rec[:, c][:, None] for c in (4, 5, 6, 7, 11))
            dx = gxp - pxf[:k]
            dy = gyp - pyf[:k]
            power = F(-0.5) * (cx * dx * dx + cz * dy * dy) - cy * dx * dy
            alpha = npo.wmin(F(0.99), op * npo.expf(power))
            Tk = T[:k]
            test = Tk * (F(1.0) - alpha)
            cond = ((power <= 0) & (alpha >= c255) & (test >= F(0.0001))).astype(F)
            for ch in range(3):
                acc[ch, :k] = acc[ch, :k] + cond * rec[:, 8 + ch][:, None] * alpha * Tk
            D[:k] = D[:k] + cond * z * alpha * Tk
            T[:k] = cond * test + (F(1.0) - cond) * Tk
    rgbf = np.zeros((H, W, 3), F)
    A = np.zeros((H, W), F)
    Dp = np.zeros((H, W), F)
    inside = (gx < W) & (gy < H)
    ys, xs = gy[inside], gx[inside]
    for ch in range(3):
        rgbf[ys, xs, ch] = acc[ch][inside]
    A[ys, xs] = (F(1.0) - T)[inside]
    Dp[ys, xs] = D[inside]
    return rgbf, A, Dp


def restate_ref(ref, W, H, ts, cols=None):
    """restate() of an oracle.render(...) result."""
    return restate(ref["gdata"], ref["sorted_values"], ref["ranges"], W, H, ts, cols)
