"""An f64 model of one frame, written from the mathematics: projection of the 320-byte records under the 40-float uniform block, and
the front-to-back blend over a given sorted list.  It imports neither the library nor oracle/np_oracle.py and follows neither's
expression tree: the covariance is a product of matrices, the spherical harmonics come from the associated-Legendre recurrence.
What it does take from the shaders are the semantics a test has to share with them: the constants (0.2, 1.1, 1.3, 0.3, 1e-7, 0.99,
1/255, 1e-4), the culls, the clamp of the Jacobian's view position and the record / uniform layouts.

ERROR ACCOUNTING.  U = 2^-24 is the relative error of one f32 operation.  The oracle's expression tree (oracle/gs_oracle.c writes
every operation out) is cut into STAGES.  A stage's result q has a MAGNITUDE: the stage's expression with every term replaced by its
absolute value, so a sum that cancels keeps the size of what cancelled.  Its own roundings are bounded by k U magnitude(q), k the
number of f32 operations on the longest path through the stage; the errors of the stage's inputs are propagated to first order
(product: |a| e_b + |b| e_a; quotient a / b: e_a / |b| + |a / b| e_b / |b|; sqrt: e / (2 sqrt); min, max, clamp: 1-Lipschitz).  The
tolerance of a quantity is the sum of the two, nothing else.  The stages and their counts k (STAGE_K below):
    view position t, clip position    4   ((m0 x + m4 y) + m8 z) + m12: a product and three adds; magnitude |m0 x| + .. + |m12|
    clip.w + 1e-7, 1 / w, clip.x / w  1   each (a single operation on the value)
    uv = ndc / 2 + 0.5                1   (the halving is exact)
    scale = exp(s) * mod              4   the canonical exp is within 1.5 ulp = 3 U (tests/test_oracle.py), the product 1
    |q|^2                             4   a product and three adds, all terms positive
    |q|, q / |q|                      1   each                                                  -> q / |q| within 4 U |q / |q||
    rotation entry  1 - 2 (y y + z z) 2+1 y y and the add: 2 on the inner magnitude 2 (yy + zz); the subtraction from 1: 1
    M = diag(scale) R                 1
    Sigma = M^T M, T = J W, T Sigma, (T Sigma) T^T     3 each: a product and two adds; magnitude |A| |B|
    view x / z, the limit 1.3 tan_fov 1, 2   (the limit: the constant is no f32, and a product)
    clamped x = clamp(x / z) z        1
    f / z;  f x;  z z;  (f x) / (z z) 1   each
    cov2d + 0.3                       2   the constant is no f32, and the add
    det = a c - b^2                   1+1 each product on its own value, the subtraction on |a c| + b^2 ... |det| (first order: below)
    conic = (c, -b, a) * (1 / det)    2
    d = pos - cam                     1   both are inputs: the one rounding is on |d|
    |d|^2                             1+2 d d on its value; two adds, all terms positive        -> 5 U |d|^2
    |d|, d / |d|                      1   each                                                  -> 5.5 U per direction component
    SH term Y_i c_i of degree l       BASIS_K[l] = 2, 10, 16, 23 on magnitude BASIS_ABS[i] |c_i|: l times the 5.5 U of a direction component
                                          (l = 0: none), the operations of the shader's polynomial on its longest path (l = 1: the two
                                          adds inside C1 (..); l = 2: 3; l = 3: 5), the constant (no f32) and its product, the product with c_i
    colour                            16  the fifteen adds of the terms and the + 0.5, each at most U x (0.5 + sum BASIS_ABS |c_i|)
    opacity                           8   z / (1 + z), z = exp(o): 3 + (3 + 1) + 1 (the other branch, 1 / (1 + exp(-o)): 5)
det cancels, so the conic's bound goes through it to first order:
    e_det = |c| u_a + |a| u_c + 2 |b| u_b + s_det + U (|a c| + b^2 + |det|),   e(c / det) = e_c / |det| + |c| e_det / det^2 + 2 U |c / det|
with u the part of cov2d's error that comes from the three matrix products' own roundings, and s_det the part of det's error that
comes from the errors of J W and diag(scale) R, through B = J W R diag(scale): cov2d = B B^T + 0.3, and a long thin splat is all but
rank one, where a, b and c move together and det does not follow any of them (project() has the formula).
BASIS_ABS[i] is the sum of the absolute monomial coefficients of the polynomial the shader evaluates for basis function i, rounded
up; a direction component is at most 1.  No number here is measured from any implementation.

THE BLEND (blend below) carries the same first-order accounting per pixel through alpha, the transmittance and the accumulator; its
comments state each term.
"""
import math

import numpy as np

U = 2.0 ** -24

STAGE_K = {"affine": 4, "scale": 4, "norm2": 4, "rotation_inner": 2, "matmul3": 3, "limit": 2, "conic": 2,
           "direction": 5.5, "colour_adds": 16, "opacity": 8}
BASIS_K = (2, 10, 16, 23)  # per degree: see ERROR ACCOUNTING

NEAR = 0.2          # a splat with view z <= NEAR is culled
NDC_LIMIT = 1.1     # ... and one with |ndc.x| or |ndc.y| >= NDC_LIMIT
CLAMP = 1.3         # the Jacobian is taken at view x / z clamped to +-CLAMP tan_fov
LOW_PASS = 0.3      # added to the diagonal of cov2d
W_EPS = 1e-7        # ndc = clip.xy / (clip.w + W_EPS)
ALPHA_MAX = 0.99
ALPHA_MIN = 1.0 / 255.0
T_MIN = 1e-4

# sum of the absolute monomial coefficients of the shader's polynomial for basis function i (degree l = floor(sqrt(i))), rounded up
BASIS_ABS = np.array([0.283, 0.489, 0.489, 0.489, 1.093, 1.093, 1.262, 1.093, 1.093, 2.361, 2.891, 2.743, 2.986, 2.743, 2.891, 2.361])
BASIS_DEGREE = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3])  # the direction d / |d| is within STAGE_K["direction"] U per component

PERTURBATIONS = ("transposed_rotation", "swapped_focal", "sh_sign")  # what a shared misreading could look like (the tests' teeth)


def real_sh(d, lmax=3):
    """Real spherical harmonics Y_lm of unit vectors d [n, 3] up to degree lmax, column l^2 + l + m, by the associated-Legendre
    recurrence with the Condon-Shortley phase (-1)^m in P_l^m:
        P_m^m = (-1)^m (2m - 1)!! sin^m,  P_{m+1}^m = (2m + 1) z P_m^m,  (l - m) P_l^m = (2l - 1) z P_{l-1}^m - (l + m - 1) P_{l-2}^m
        Y_l0 = K_l0 P_l^0,  Y_l,+m = sqrt 2 K_lm cos(m phi) P_l^m,  Y_l,-m = sqrt 2 K_lm sin(m phi) P_l^m,
        K_lm = sqrt((2l + 1) / (4 pi) (l - m)! / (l + m)!)."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    st = np.hypot(x, y)
    phi = np.arctan2(y, x)
    out = np.zeros((d.shape[0], (lmax + 1) ** 2))
    for m in range(lmax + 1):
        dfact = 1.0
        for k in range(1, 2 * m, 2):
            dfact *= k
        P = {m: (-1.0) ** m * dfact * st ** m}
        if m < lmax:
            P[m + 1] = (2 * m + 1) * z * P[m]
        for l in range(m + 2, lmax + 1):
            P[l] = ((2 * l - 1) * z * P[l - 1] - (l + m - 1) * P[l - 2]) / (l - m)
        for l in range(m, lmax + 1):
            Klm = math.sqrt((2 * l + 1) / (4.0 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
            if m == 0:
                out[:, l * l + l] = Klm * P[l]
            else:
                out[:, l * l + l + m] = math.sqrt(2.0) * Klm * np.cos(m * phi) * P[l]
                out[:, l * l + l - m] = math.sqrt(2.0) * Klm * np.sin(m * phi) * P[l]
    return out


def rotation(q):
    """(R, e_R) [n, 3, 3] of the normalised quaternions q = (r, x, y, z) [n, 4]: v -> R v rotates v.  e_R: a component of q / |q| is
    within 4 U of itself, a product of two within 9 U, so an entry's inner sum 2 (y y + z z) or 2 (x y - r z) within 10 U of its
    magnitude; the diagonal's subtraction from 1 adds U |R|."""
    q = q / np.linalg.norm(q, axis=1)[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)
    a = np.abs(q)
    r, x, y, z = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    inner = np.empty_like(R)
    inner[:, 0, 0], inner[:, 1, 1], inner[:, 2, 2] = 2 * (y * y + z * z), 2 * (x * x + z * z), 2 * (x * x + y * y)
    inner[:, 0, 1] = inner[:, 1, 0] = 2 * (x * y + r * z)
    inner[:, 0, 2] = inner[:, 2, 0] = 2 * (x * z + r * y)
    inner[:, 1, 2] = inner[:, 2, 1] = 2 * (y * z + r * x)
    k = 2 * STAGE_K["norm2"] + STAGE_K["rotation_inner"]
    return R, U * (k * inner + np.abs(R) * np.eye(3))


def matmul_err(A, eA, B, eB):
    """First-order error of the f32 product A B with inner dimension 3 (a product and two adds per entry)."""
    return np.abs(A) @ eB + eA @ np.abs(B) + STAGE_K["matmul3"] * U * (np.abs(A) @ np.abs(B))


def project(splats, uniforms, perturb=None):
    """The projection of records [n, 80] under uniforms [40] in f64.  Returns a dict of [n] / [n, k] arrays: every quantity q of the
    projected record (uv, conic, depth, colour, opacity) with its f32 tolerance q_tol, the intermediate t (view position), ndc, cov
    (a, b, c of the symmetric cov2d) and det, `visible` (the f64 cull decision) and `decided` (False where some cull's f64 margin is
    inside its tolerance, so that an f32 evaluation may decide either way).  perturb: one of PERTURBATIONS, for the tests that show
    that the comparison notices."""
    assert perturb is None or perturb in PERTURBATIONS
    s = np.asarray(splats, np.float64).reshape(-1, 80)
    u = np.asarray(uniforms, np.float64).reshape(40)
    n = s.shape[0]
    V = u[0:16].reshape(4, 4).T   # the block holds columns: V[r, c] = u[4 c + r]
    P = u[16:32].reshape(4, 4).T
    cam, tanx, tany, fx, fy, mod = u[32:35], u[35], u[36], u[37], u[38], u[39]
    if perturb == "swapped_focal":
        fx, fy = fy, fx
    pos = s[:, 0:3]
    hom = np.concatenate([pos, np.ones((n, 1))], axis=1)
    out = {}
    with np.errstate(all="ignore"):
        # ---- view and clip position, depth, ndc, uv ------------------------------------------------------------------------------
        t, e_t = hom @ V.T, STAGE_K["affine"] * U * (np.abs(hom) @ np.abs(V).T)
        clip, e_clip = hom @ P.T, STAGE_K["affine"] * U * (np.abs(hom) @ np.abs(P).T)
        w = clip[:, 3] + W_EPS
        e_w = e_clip[:, 3] + U * (np.abs(w) + W_EPS)
        e_inv = e_w / (w * w) + U / np.abs(w)
        ndc = clip[:, 0:2] / w[:, None]
        e_ndc = e_clip[:, 0:2] / np.abs(w)[:, None] + np.abs(clip[:, 0:2]) * e_inv[:, None] + U * np.abs(ndc)
        uv = 0.5 * ndc + 0.5
        out.update(t=t, ndc=ndc, ndc_tol=e_ndc, depth=t[:, 2], depth_tol=e_t[:, 2], uv=uv, uv_tol=0.5 * e_ndc + U * np.abs(uv))
        # ---- Sigma = R diag(scale^2) R^T; the oracle forms M = diag(scale) R^T and M^T M ------------------------------------------
        scale = np.exp(s[:, 4:7]) * mod
        R, e_R = rotation(s[:, 8:12])
        if perturb == "transposed_rotation":
            R = R.transpose(0, 2, 1)
        RS = R * scale[:, None, :]  # Sigma = RS RS^T
        e_RS = e_R * scale[:, None, :] + np.abs(RS) * ((STAGE_K["scale"] + 1) * U)
        Sigma = RS @ RS.transpose(0, 2, 1)
        # ---- the perspective Jacobian at the clamped view position, cov2d = (J W) Sigma (J W)^T + LOW_PASS -----------------------
        tz, e_tz = t[:, 2], e_t[:, 2]
        J, e_J = np.zeros((n, 2, 3)), np.zeros((n, 2, 3))
        for a, (f, tan) in enumerate(((fx, tanx), (fy, tany))):
            lim = CLAMP * tan
            e_lim = STAGE_K["limit"] * U * lim
            ratio = t[:, a] / tz
            e_ratio = e_t[:, a] / np.abs(tz) + np.abs(ratio) * e_tz / np.abs(tz) + U * np.abs(ratio)
            deep = np.abs(ratio) - lim > e_ratio + e_lim  # clamped in f32 and in f64: the value is the limit
            c = np.clip(ratio, -lim, lim)
            e_c = np.where(deep, e_lim, np.maximum(e_ratio, e_lim))
            x = c * tz
            e_x = np.abs(c) * e_tz + np.abs(tz) * e_c + U * np.abs(x)
            J[:, a, a] = f / tz
            e_J[:, a, a] = np.abs(J[:, a, a]) * (e_tz / np.abs(tz) + U)
            num, den = f * x, tz * tz
            e_num, e_den = f * e_x + U * np.abs(num), 2 * np.abs(tz) * e_tz + U * den
            J[:, a, 2] = -num / den
            e_J[:, a, 2] = e_num / den + np.abs(J[:, a, 2]) * (e_den / den + U)
        Wv = V[0:3, 0:3][None, :, :]
        JW = J @ Wv
        e_JW = matmul_err(J, e_J, Wv, np.zeros_like(Wv))
        # cov = B B^T with B = JW RS: the errors of JW and RS reach cov as dB B^T + B dB^T, |dB| <= e_JW |RS| + |JW| e_RS, which keeps
        # the cancellation a thin splat seen edge-on has in B; the three products' own roundings (Sigma = M^T M, T Sigma, (T Sigma) T^T)
        # are unstructured: k U |A| |B| each, carried through the exact factors that follow
        B = JW @ RS
        e_B = e_JW @ np.abs(RS) + np.abs(JW) @ e_RS
        k3 = STAGE_K["matmul3"] * U
        half = JW @ Sigma
        cov = half @ JW.transpose(0, 2, 1)
        aJWt = np.abs(JW).transpose(0, 2, 1)
        e_covS = e_B @ np.abs(B).transpose(0, 2, 1) + np.abs(B) @ e_B.transpose(0, 2, 1)
        e_covU = k3 * (np.abs(JW) @ (np.abs(RS) @ np.abs(RS).transpose(0, 2, 1)) @ aJWt + (np.abs(JW) @ np.abs(Sigma)) @ aJWt + np.abs(half) @ aJWt)
        cov = cov + LOW_PASS * np.eye(2)
        e_covU = e_covU + U * (np.abs(cov) + LOW_PASS) * np.eye(2)
        e_cov = e_covS + e_covU
        a, b, c = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
        ea, eb, ec = e_cov[:, 0, 0], np.maximum(e_cov[:, 0, 1], e_cov[:, 1, 0]), e_cov[:, 1, 1]
        ua, ub, uc = e_covU[:, 0, 0], np.maximum(e_covU[:, 0, 1], e_covU[:, 1, 0]), e_covU[:, 1, 1]
        det = a * c - b * b
        # det through dB, where a, b and c move together (a long thin splat is all but rank one: a c - b^2 cancels, and does not move when
        # B is scaled): det(B B^T + p I) = sum_{k<l} m_kl^2 + p |B|_F^2 + p^2 with the minors m_kl = B_0k B_1l - B_0l B_1k (Cauchy-Binet)
        e_detS = LOW_PASS * 2 * (np.abs(B) * e_B).sum(axis=(1, 2))
        for k, l in ((0, 1), (0, 2), (1, 2)):
            minor = B[:, 0, k] * B[:, 1, l] - B[:, 0, l] * B[:, 1, k]
            e_minor = (np.abs(B[:, 1, l]) * e_B[:, 0, k] + np.abs(B[:, 0, k]) * e_B[:, 1, l] +
                       np.abs(B[:, 1, k]) * e_B[:, 0, l] + np.abs(B[:, 0, l]) * e_B[:, 1, k])
            e_detS = e_detS + 2 * np.abs(minor) * e_minor
        det_tol = e_detS + np.abs(c) * ua + np.abs(a) * uc + 2 * np.abs(b) * ub + U * (np.abs(a * c) + b * b + np.abs(det))
        conic = np.stack([c / det, -b / det, a / det], axis=1)
        conic_tol = np.stack([e / np.abs(det) + np.abs(v) * det_tol / (det * det) + STAGE_K["conic"] * U * np.abs(v / det)
                              for v, e in ((c, ec), (b, eb), (a, ea))], axis=1)
        out.update(cov=np.stack([a, b, c], axis=1), cov_tol=np.stack([ea, eb, ec], axis=1), det=det, det_tol=det_tol, conic=conic,
                   conic_tol=conic_tol)
        # ---- opacity and colour ---------------------------------------------------------------------------------------------------
        opacity = 1.0 / (1.0 + np.exp(-s[:, 12]))
        out.update(opacity=opacity, opacity_tol=STAGE_K["opacity"] * U * opacity)
        d = pos - cam[None, :]
        Y = real_sh(d / np.linalg.norm(d, axis=1)[:, None])
        if perturb == "sh_sign":
            Y[:, 11] = -Y[:, 11]
        coeff = s[:, 16:80].reshape(n, 16, 4)[:, :, 0:3]
        colour = np.maximum(0.0, 0.5 + np.einsum("ni,nic->nc", Y, coeff))
        size = np.einsum("i,nic->nc", BASIS_ABS, np.abs(coeff))
        own = np.einsum("i,nic->nc", BASIS_ABS * np.array(BASIS_K, np.float64)[BASIS_DEGREE], np.abs(coeff))
        out.update(colour=colour, colour_tol=U * (own + STAGE_K["colour_adds"] * (0.5 + size)), sh=Y)
        # ---- the culls: near plane, the four ndc planes, det == 0 -----------------------------------------------------------------
        margins = np.stack([t[:, 2] - NEAR, NDC_LIMIT - ndc[:, 0], ndc[:, 0] + NDC_LIMIT, NDC_LIMIT - ndc[:, 1], ndc[:, 1] + NDC_LIMIT],
                           axis=1)  # > 0: kept by that plane
        margin_tol = np.stack([out["depth_tol"] + U * NEAR] + [out["ndc_tol"][:, k] + U * NDC_LIMIT for k in (0, 0, 1, 1)], axis=1)
        finite = np.isfinite(margins).all(axis=1)
        kept = finite & (margins > 0).all(axis=1)
        surely_culled = finite & (margins < -margin_tol).any(axis=1)
        surely_kept = finite & (margins > margin_tol).all(axis=1) & (np.abs(det) > det_tol)
    out.update(margins=margins, margin_tol=margin_tol, visible=kept & (det != 0.0), decided=surely_culled | surely_kept)
    return out


PLANES = ("near", "ndc +x", "ndc -x", "ndc +y", "ndc -y")  # the columns of project()["margins"]


def blend(proj, values, ranges, W, H, ts, tiles=None):
    """The image of compute_tiles in f64: per pixel, front to back over its tile's part of the sorted list `values` (tile t owns
    values[ranges[t - 1] : ranges[t]]; the order is an integer result, pinned elsewhere); every float comes from proj = project(..).
    An entry is kept iff power <= 0, alpha = min(0.99, opacity exp(power)) >= 1/255 and T (1 - alpha) >= 1e-4; a kept entry adds
    colour alpha T and multiplies T by 1 - alpha.  tiles: evaluate these tile indices only (the rest of the result is zero and
    `done` False there).

    Returns (image [H, W, 3], bound [H, W, 3], flagged [H, W], done [H, W]).
    bound: what an f32 evaluation of the same pixel may differ by, to first order, while it takes the same decisions.  Per entry:
        g = uv * size      e_g = size e_uv + U |g|                          (the f32 rounding of the product: at g ~ 100 px this is
        d = g - pixel      e_d = e_g + U |d|                                 6e-6 px, the largest single term)
        power = -(c0 d0^2 + c2 d1^2) / 2 - c1 d0 d1
                           e_p = sum over the three terms of (conic error + 2 x relative error of d + 2 U) |term|
                                 + U |t1 + t2| / 2 + U |power|               (two products per term, the add, the subtraction)
        alpha              relative e_a / alpha = e_opacity / opacity + e_p + 4 U   (exp: 3, product: 1); at the 0.99 clamp U
        1 - alpha          e_m = e_a + U (1 - alpha)
        T (1 - alpha)      relative: that of T + e_m / (1 - alpha) + U
        colour alpha T     relative: e_colour / colour + e_a / alpha + that of T + 2 U; the accumulator's add: U |sum so far|
    flagged: some entry's power, alpha - 1/255 or T (1 - alpha) - 1e-4 lies inside its own band (e_p, e_a, the error of T (1 - alpha)),
    unless another of the three tests rejects the entry outside ITS band: there f32 and f64 may legitimately decide differently."""
    values = np.asarray(values).astype(np.int64)
    ranges = np.asarray(ranges).astype(np.int64)
    ntx, nty = -(-W // ts), -(-H // ts)
    yy, xx = np.mgrid[0:H, 0:W]
    tile = ((yy // ts) * ntx + xx // ts).ravel()
    start_t = np.concatenate([[0], ranges[:-1]])
    len_t = np.maximum(ranges - start_t, 0)
    if tiles is not None:
        chosen = np.zeros(ntx * nty, bool)
        chosen[np.asarray(tiles, np.int64)] = True
        len_t = np.where(chosen, len_t, 0)
        done = chosen[tile]
    else:
        done = np.ones(W * H, bool)
    order = np.argsort(-len_t[tile], kind="stable")  # pixels by falling list length: the active ones are a prefix
    px, py = xx.ravel()[order].astype(np.float64), yy.ravel()[order].astype(np.float64)
    start, length = start_t[tile][order], len_t[tile][order]
    table = np.concatenate([proj["uv"], proj["uv_tol"], proj["conic"], proj["conic_tol"], proj["colour"], proj["colour_tol"],
                            proj["opacity"][:, None], proj["opacity_tol"][:, None]], axis=1)
    npx = W * H
    acc, acc_abs, err = np.zeros((npx, 3)), np.zeros((npx, 3)), np.zeros((npx, 3))
    T, T_rel, flagged = np.ones(npx), np.zeros(npx), np.zeros(npx, bool)
    size = np.array([float(W), float(H)])
    neg_count = -length  # ascending
    with np.errstate(all="ignore"):
        for j in range(int(length.max(initial=0))):
            m = int(np.searchsorted(neg_count, -j, side="left"))  # pixels with length > j
            g = table[values[start[:m] + j]]
            uv, e_uv, con, e_con, col, e_col, op, e_op = g[:, 0:2], g[:, 2:4], g[:, 4:7], g[:, 7:10], g[:, 10:13], g[:, 13:16], g[:, 16], g[:, 17]
            c = uv * size
            e_c = size * e_uv + U * np.abs(c)
            d0, d1 = c[:, 0] - px[:m], c[:, 1] - py[:m]
            e0, e1 = e_c[:, 0] + U * np.abs(d0), e_c[:, 1] + U * np.abs(d1)
            t1, t2, t3 = con[:, 0] * d0 * d0, con[:, 2] * d1 * d1, con[:, 1] * d0 * d1
            e_t1 = e_con[:, 0] * d0 * d0 + 2 * np.abs(con[:, 0] * d0) * e0 + 2 * U * np.abs(t1)
            e_t2 = e_con[:, 2] * d1 * d1 + 2 * np.abs(con[:, 2] * d1) * e1 + 2 * U * np.abs(t2)
            e_t3 = e_con[:, 1] * np.abs(d0 * d1) + np.abs(con[:, 1]) * (np.abs(d1) * e0 + np.abs(d0) * e1) + 2 * U * np.abs(t3)
            power = -0.5 * (t1 + t2) - t3
            e_p = 0.5 * (e_t1 + e_t2) + e_t3 + 0.5 * U * np.abs(t1 + t2) + U * np.abs(power)
            raw = op * np.exp(np.minimum(power, 80.0))
            e_raw = raw * (e_op / op + e_p + 4 * U)
            alpha = np.minimum(ALPHA_MAX, raw)
            e_a = np.where(raw - e_raw > ALPHA_MAX * (1 + U), U * ALPHA_MAX, e_raw + U * ALPHA_MAX * (raw >= ALPHA_MAX))
            one_m = 1.0 - alpha
            m_rel = (e_a + U * one_m) / one_m
            test_t = T[:m] * one_m
            e_tt = test_t * (T_rel[:m] + m_rel + U)
            ok = np.isfinite(power) & np.isfinite(raw)
            keep = ok & (power <= 0.0) & (alpha >= ALPHA_MIN) & (test_t >= T_MIN)
            sure_keep = (power < -e_p) & (alpha - e_a > ALPHA_MIN * (1 + U)) & (test_t - e_tt > T_MIN * (1 + U))
            sure_skip = (power > e_p) | (alpha + e_a < ALPHA_MIN * (1 - U)) | (test_t + e_tt < T_MIN * (1 - U))
            flagged[:m] |= ~(sure_keep | sure_skip) | ~ok
            wgt = np.where(keep, alpha * T[:m], 0.0)
            rel = np.where(keep, e_a / alpha + T_rel[:m] + 2 * U, 0.0)
            term = col * wgt[:, None]
            acc[:m] += term
            acc_abs[:m] += np.abs(term)
            err[:m] += np.abs(term) * rel[:, None] + e_col * wgt[:, None] + U * acc_abs[:m] * keep[:, None]
            T[:m] = np.where(keep, test_t, T[:m])
            T_rel[:m] = np.where(keep, T_rel[:m] + m_rel + U, T_rel[:m])
    image, bound, flag = np.zeros((npx, 3)), np.zeros((npx, 3)), np.zeros(npx, bool)
    image[order], bound[order], flag[order] = acc, err, flagged
    return image.reshape(H, W, 3), bound.reshape(H, W, 3), flag.reshape(H, W), done.reshape(H, W)
