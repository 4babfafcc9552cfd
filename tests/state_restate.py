"""numpy restatement of the splat-state layer (include/gsplat/gs_abi.h "splat state"): region membership, the four operations,
and the frame a state plane must produce.  TEST INFRASTRUCTURE ONLY.

Every float expression is evaluated in f32 with one rounding per operation, in the order the header fixes, so that the GPU
kernels (k_state.hip, the STATE projection of k_preprocess.hip) can be held to it bit for bit.  The CPU tests of
test_splat_state.py prove that the projection below IS the oracle's (uv words of GaussianData) and that the constructed frame
IS the oracle's frame of the scene without the hidden records.
"""
import numpy as np

F = np.float32
HIDDEN, SELECTED = 0x1, 0x2
SET, CLEAR, TOGGLE, ASSIGN = 1, 2, 3, 4
ALL, SPHERE, BOX, RECT, MASK = range(5)
TINT_DEFAULT = 0x80FFFF00


def positions(splats):
    s = np.ascontiguousarray(splats, dtype=F).reshape(-1, 80)
    return s[:, 0].copy(), s[:, 1].copy(), s[:, 2].copy()


def _row(m, r, x, y, z):
    """m4_mulv, row r of a column-major mat4: ((m[r] x + m[4+r] y) + m[8+r] z) + m[12+r]."""
    return ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r]


def project(splats, uniforms, W, H):
    """(uvx, uvy, px, py, pvz) of every centre, as the projection computes them."""
    u = np.ascontiguousarray(uniforms, dtype=F).reshape(40)
    view, proj = u[0:16], u[16:32]
    x, y, z = positions(splats)
    with np.errstate(all="ignore"):
        phx, phy, phw = _row(proj, 0, x, y, z), _row(proj, 1, x, y, z), _row(proj, 3, x, y, z)
        pvz = _row(view, 2, x, y, z)
        pw = F(1.0) / (phw + F(0.0000001))
        uvx = (phx * pw) * F(0.5) + F(0.5)
        uvy = (phy * pw) * F(0.5) + F(0.5)
        px, py = uvx * F(W), uvy * F(H)
    return uvx, uvy, px, py, pvz


def member(kind, splats, W, H, *, a=(0, 0, 0), b=(0, 0, 0), rect=(0, 0, 0, 0), uniforms=None, mask=None):
    """bool[N]: which centres lie in the region (a NaN fails every test)."""
    x, y, z = positions(splats)
    n = x.size
    with np.errstate(all="ignore"):
        if kind == ALL:
            return np.ones(n, bool)
        if kind == SPHERE:
            dx, dy, dz = x - F(a[0]), y - F(a[1]), z - F(a[2])
            return (dx * dx + dy * dy) + dz * dz <= F(b[0]) * F(b[0])
        if kind == BOX:
            return ((x >= F(a[0])) & (x <= F(b[0])) & (y >= F(a[1])) & (y <= F(b[1])) & (z >= F(a[2])) & (z <= F(b[2])))
        _, _, px, py, pvz = project(splats, uniforms, W, H)
        front = ~(pvz <= F(0.2))
        if kind == RECT:
            x0, y0, x1, y1 = (F(v) for v in rect)
            return front & (px >= x0) & (px < x1) & (py >= y0) & (py < y1)
        if kind == MASK:
            m = np.asarray(mask, np.uint8).reshape(H, W)
            inside = front & (px >= F(0)) & (px < F(W)) & (py >= F(0)) & (py < F(H))
            out = np.zeros(n, bool)
            ix, iy = px[inside].astype(np.int64), py[inside].astype(np.int64)  # (truncation, as (int) does)
            out[inside] = m[iy, ix] != 0
            return out
    raise ValueError(kind)


def op_apply(s, op, bits):
    s = np.asarray(s, np.uint8)
    bits = np.uint8(bits)
    if op == SET:
        return s | bits
    if op == CLEAR:
        return s & np.uint8(~bits & 0xFF)
    if op == TOGGLE:
        return s ^ bits
    if op == ASSIGN:
        return np.full_like(s, bits)
    raise ValueError(op)


def apply_region(state, inside, op, bits, where=(0, 0)):
    """(new plane, matched): matched counts the splats in the region that pass the filter, changed or not."""
    state = np.asarray(state, np.uint8)
    hit = inside & ((state & np.uint8(where[0])) == where[1])
    out = state.copy()
    out[hit] = op_apply(state[hit], op, bits)
    return out, int(hit.sum())


def apply_ids(state, ids, op, bits):
    """The sequential application, one id after the other (duplicates included)."""
    out = np.asarray(state, np.uint8).copy()
    for i in np.asarray(ids, np.int64).ravel():
        out[i] = op_apply(out[i:i + 1], op, bits)[0]
    return out


def count(state, mask, value):
    return int(((np.asarray(state, np.uint8).astype(np.uint32) & np.uint32(mask)) == value).sum())


# ---- the regions of the issue, for a W x H canvas --------------------------------------------------------------------------------
def issue_mask(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    disc = (xx - W / 2) ** 2 + (yy - 0.45 * H) ** 2 < (0.3 * H) ** 2
    return (disc & ((xx // 8 + yy // 8) % 2 == 0)).astype(np.uint8)


def issue_regions(W, H, uniforms):
    """name -> (kind, keyword arguments of member / Renderer.state_region)."""
    return {
        "centre_half_rect": (RECT, dict(rect=(W // 4, H // 4, 3 * W // 4, 3 * H // 4), uniforms=uniforms)),
        "strip": (RECT, dict(rect=(3, 5, 40, H), uniforms=uniforms)),
        "sphere_r1": (SPHERE, dict(a=(0.0, 0.0, 0.0), b=(1.0, 0, 0))),
        "sphere_r075": (SPHERE, dict(a=(0.5, 0.2, -0.3), b=(0.75, 0, 0))),
        "box": (BOX, dict(a=(-1.0, -0.5, -1.0), b=(0.5, 1.0, 1.5))),
        "mask": (MASK, dict(mask=issue_mask(W, H), uniforms=uniforms)),
    }


# ---- the frame a state plane must produce -------------------------------------------------------------------------------------------
def tint_colour(col, tint):
    """col f32[..., 3] -> col + k (t - col), k = a / 255, t = channel / 255; a = 0 leaves the colour untouched."""
    a = (tint >> 24) & 255
    if a == 0:
        return col.copy()
    k = F(a) / F(255.0)
    t = np.array([F((tint >> 16) & 255) / F(255.0), F((tint >> 8) & 255) / F(255.0), F(tint & 255) / F(255.0)], F)
    with np.errstate(all="ignore"):
        return (col + k * (t - col)).astype(F)


def state_frame(oracle, splats, uniforms, W, H, ts, state, tint=TINT_DEFAULT, cols=None, **blend_kw):
    """The oracle's frame for a state plane: preprocess the full scene (ids keep their meaning), zero the count and the record of
    every hidden splat, tint the colour words 8-10 of every selected visible one, then the oracle's own scan -> emit -> sort ->
    ranges -> blend.  Returns what oracle.render returns."""
    state = np.asarray(state, np.uint8)
    ntx, nty = oracle.num_tiles(W, H, ts)
    gdata, counts = oracle.preprocess(splats, uniforms, W, H, ts, cols)
    hidden = (state & HIDDEN) != 0
    counts[hidden] = 0
    gdata[hidden] = 0
    sel = ((state & SELECTED) != 0) & ~hidden & (counts > 0)
    if sel.any():
        col = gdata[sel, 8:11].copy().view(F)
        gdata[sel, 8:11] = tint_colour(col, tint).view(np.uint32)
    offsets, total = oracle.scan(counts)
    keys, values = oracle.emit(gdata, offsets, counts, total, W, ts, cols)
    skeys, svalues = oracle.sort(keys, values)
    rng = oracle.ranges(skeys, ntx * nty)
    out = oracle.blend(gdata, svalues, rng, W, H, ts, cols, **blend_kw)
    out.update(gdata=gdata, tile_counts=counts, offsets=offsets, num_intersections=total, keys=keys, values=values,
               sorted_keys=skeys, sorted_values=svalues, ranges=rng)
    return out
