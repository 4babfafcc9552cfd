"""Host restatement of the slab reach cull (csrc/k_preprocess.hip, in_frustum_slab) in numpy f32, the spectral norm of a view
matrix's 3x3 in f64, and builders of non-rigid uniform blocks.

A tile-column slab context drops a gaussian in phase 1 of the projection, before its record is read, when

    rb = 3 sqrt(2 |J|_F^2 w2 s_max^2 + 0.92) 1.001 + 2        (pixels)

around its projected centre cannot reach the slab's columns; w2 bounds the squared spectral norm of the view's 3x3 (w2 = 1 is the
bound of a rigid view).  tests/test_slab_reach.py uses this module to CHOOSE and QUALIFY its inputs only (which splats a bound
with w2 = 1 would drop, how close a centre lies to a slab edge); the expected result of every test is the oracle's.  It is no
bit-level model of the kernel: numpy's exp stands where the kernel has its fast exponential (the bound's 1.001 covers both).
"""
import numpy as np

F = np.float32


# ---- the uniform block (160 bytes: view[16] and proj[16] column-major, cam[3], tan_fovx, tan_fovy, focal_x, focal_y, scale modifier) ---
def view3(u):
    """The upper 3x3 of the view matrix as a (row, column) array, f64."""
    return np.asarray(u, np.float64)[:16].reshape(4, 4).T[:3, :3].copy()


def spectral_norm(u):
    """Largest singular value of the view's 3x3, f64."""
    return float(np.linalg.svd(view3(u), compute_uv=False)[0])


def apply_view(u, A):
    """A copy of u with view' = [A 0; 0 1] view; proj, the camera position, the focals and the rest stay as they are."""
    out = np.array(u, dtype=F, copy=True)
    V = out[:16].astype(np.float64).reshape(4, 4).T
    M = np.eye(4)
    M[:3, :3] = np.asarray(A, np.float64)
    out[:16] = (M @ V).T.reshape(16).astype(F)
    return out


def with_scale_modifier(u, mod):
    out = np.array(u, dtype=F, copy=True)
    out[39] = mod
    return out


def uniform_scale(k):
    return np.eye(3) * float(k)


def shear_z_by_x(k=4.0):
    """Row 2 of the view gains k times row 0: depth = z + k x."""
    A = np.eye(3)
    A[2, 0] = k
    return A


# ---- in_frustum_slab in f32, one rounding per written operation ---------------------------------------------------------------------
def _mulv(m, x, y, z):
    return [((m[0 + r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * F(1.0) for r in range(4)]


def reach(splats, u, W, w2=1.0):
    """(in the frustum, pixel x of the centre, rb) per splat; w2: the factor on |J|_F^2."""
    s = np.asarray(splats, F).reshape(-1, 80)
    u = np.asarray(u, F).reshape(40)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    smax_log = np.maximum(s[:, 4], np.maximum(s[:, 5], s[:, 6]))
    with np.errstate(all="ignore"):
        ph = _mulv(u[16:32], x, y, z)
        pw = F(1.0) / (ph[3] + F(0.0000001))
        ndx, ndy = ph[0] * pw, ph[1] * pw
        pv = _mulv(u[0:16], x, y, z)
        out = (pv[2] <= F(0.2)) | (ndx <= F(-1.1)) | (ndx >= F(1.1)) | (ndy <= F(-1.1)) | (ndy >= F(1.1))
        sm = np.exp(smax_log).astype(F) * u[39] * F(1.001)
        limx, limy = F(1.3) * u[35], F(1.3) * u[36]
        iz = F(1.0) / pv[2]
        jf2 = (u[37] * iz) * (u[37] * iz) * (F(1.0) + limx * limx) + (u[38] * iz) * (u[38] * iz) * (F(1.0) + limy * limy)
        jf2 = jf2 * F(w2)
        rb = F(3.0) * np.sqrt(F(2.0) * jf2 * sm * sm + F(0.92)) * F(1.001) + F(2.0)
        pxs = ((ndx * F(0.5)) + F(0.5)) * F(W)
    return ~out, pxs, rb


def keeps(splats, u, W, ts, ntx, cols, w2=1.0):
    """The cull's verdict per splat for the slab cols = (c0, c1) of a canvas ntx tile columns wide."""
    c0, c1 = cols
    vis, pxs, rb = reach(splats, u, W, w2)
    with np.errstate(all="ignore"):
        lo, hi = pxs - rb, pxs + rb
        hit = (lo < F(c1) * F(ts)) & ((c0 == 0) | (hi >= F(c0) * F(ts)))
        alias = (c0 == 0) & (hi >= F(ntx) * F(ts))
    return vis & (hit | alias | ~(rb == rb))


def cull_chunks(ntx, cols, tight):
    """NB of the projection kernel gs_preprocess_prepare launches for a slab (reference binning 1 / 4 / 8, tight 2 / 4 / 8)."""
    w = cols[1] - cols[0]
    nb = 1 if (cols == (0, ntx) or w * 4 > ntx * 3) else (4 if w * 10 > ntx * 3 else 8)
    return (2 if nb == 1 else nb) if tight else nb


# ---- what the oracle projected, for measuring distances to a slab edge ----------------------------------------------------------------
def oracle_centre_radius(gdata, W):
    """(pixel x of the centre, the radius ceil(3 sigma) of the rect) of the oracle's whole-canvas records, recomputed in f64 from
    the conic; NaN where the record is all zero (culled)."""
    g = np.ascontiguousarray(gdata).view(F).reshape(-1, 16).astype(np.float64)
    cx, cy, cz = g[:, 4], g[:, 5], g[:, 6]
    with np.errstate(all="ignore"):
        d = cx * cz - cy * cy
        a, c = cz / d, cx / d  # the 2D covariance back from its inverse
        mid = 0.5 * (a + c)
        l1 = mid + np.sqrt(np.maximum(0.1, mid * mid - 1.0 / d))
        r = np.ceil(3.0 * np.sqrt(l1))
    live = np.ascontiguousarray(gdata).reshape(-1, 16).any(axis=1)
    return np.where(live, g[:, 0] * W, np.nan), np.where(live, r, np.nan)
