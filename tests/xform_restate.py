"""numpy restatement of the splat transforms (include/gsplat/gs_abi.h "splat transforms").  TEST INFRASTRUCTURE ONLY.

Two halves, as the header has two layers:
  * apply(): the per-splat definition of gs_transform_splats on float32 [n, 80] records, every expression in f32 with one rounding
    per written operation, left to right, so that the kernel (k_xform.hip) can be held to it on the uint32 view;
  * an INDEPENDENT float64 construction of what gs_xform_compose must produce: the rotation matrix of a quaternion, the similarity
    matrix, and the SH band matrices D_1..D_3 as a least-squares fit of B_l(R^T d) against B_l(d) over a few hundred seeded
    directions -- nothing shared with the library's solve but the definition -- plus a float64 compute_color_from_sh
    (process_gaussians.wgsl:240-280) and the covariance of compute_cov3d (:127-163).
"""
import numpy as np

F = np.float32
POSITION, ORIENT, SIZE = 0x1, 0x2, 0x4
BANDS = ((1, 1, 3), (2, 4, 5), (3, 9, 7))  # (l, first coefficient k0, 2l + 1)

C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)
C0 = 0.28209479177387814

POS_FLOATS = [0, 1, 2]
SIZE_FLOATS = [4, 5, 6]
ORIENT_FLOATS = [8, 9, 10, 11] + [16 + 4 * k + c for k in range(1, 16) for c in range(3)]


class Xform:
    """The numbers of a gs_xform as numpy arrays (f32 by default; f64 for the yardstick of the end-to-end test)."""

    def __init__(self, flags, m, q, log_scale, sh1, sh2, sh3, dtype=F):
        self.flags = int(flags)
        self.m = np.asarray(m, dtype).reshape(12)
        self.q = np.asarray(q, dtype).reshape(4)
        self.log_scale = dtype(log_scale)
        self.sh = {1: np.asarray(sh1, dtype).reshape(3, 3), 2: np.asarray(sh2, dtype).reshape(5, 5), 3: np.asarray(sh3, dtype).reshape(7, 7)}
        self.dtype = dtype

    @staticmethod
    def from_struct(x):
        return Xform(x.flags, list(x.m), list(x.q), x.log_scale, list(x.sh1), list(x.sh2), list(x.sh3))

    def with_flags(self, flags):
        return Xform(flags, self.m, self.q, self.log_scale, self.sh[1], self.sh[2], self.sh[3], self.dtype)

    def transposed_sh(self):
        return Xform(self.flags, self.m, self.q, self.log_scale, self.sh[1].T, self.sh[2].T, self.sh[3].T, self.dtype)


def touched_floats(flags):
    return sorted((POS_FLOATS if flags & POSITION else []) + (ORIENT_FLOATS if flags & ORIENT else []) + (SIZE_FLOATS if flags & SIZE else []))


def apply(rec, x, sel=None):
    """The records after gs_transform_splats(x) on the rows where sel is true (None: all).  Arithmetic in x.dtype; the result is
    float32 [n, 80] (an f64 Xform rounds each record float once).  Untouched floats keep their bit patterns."""
    src = np.ascontiguousarray(rec, dtype=F).reshape(-1, 80)
    out = src.copy()
    n = src.shape[0]
    rows = np.arange(n) if sel is None else np.flatnonzero(sel)
    if rows.size == 0 or not x.flags:
        return out
    T = x.dtype
    s = src[rows].astype(T)
    new = {}
    with np.errstate(all="ignore"):
        if x.flags & POSITION:
            X, Y, Z = s[:, 0], s[:, 1], s[:, 2]
            m = x.m
            for r in range(3):
                new[r] = ((m[4 * r] * X + m[4 * r + 1] * Y) + m[4 * r + 2] * Z) + m[4 * r + 3]
        if x.flags & SIZE:
            for k in range(3):
                new[4 + k] = s[:, 4 + k] + x.log_scale
        if x.flags & ORIENT:
            ar, ax, ay, az = x.q
            br, bx, by, bz = s[:, 8], s[:, 9], s[:, 10], s[:, 11]
            new[8] = ((ar * br - ax * bx) - ay * by) - az * bz
            new[9] = ((ar * bx + ax * br) + ay * bz) - az * by
            new[10] = ((ar * by - ax * bz) + ay * br) + az * bx
            new[11] = ((ar * bz + ax * by) - ay * bx) + az * br
            for l, k0, w in BANDS:
                D = x.sh[l]
                for c in range(3):
                    cin = [s[:, 16 + 4 * (k0 + j) + c] for j in range(w)]
                    for i in range(w):
                        acc = D[i, 0] * cin[0]
                        for j in range(1, w):
                            acc = acc + D[i, j] * cin[j]
                        new[16 + 4 * (k0 + i) + c] = acc
    for col, v in new.items():
        out[rows, col] = v.astype(F)
    return out


# ---- float64: what gs_xform_compose must produce -------------------------------------------------------------------------------------
def rot_matrix(q):
    """The rotation compute_cov3d builds from a normalised (r, x, y, z), acting on column vectors."""
    r, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def sh_basis(l, d):
    """compute_color_from_sh's band-l terms at unit directions d [..., 3] -> [..., 2l + 1] (float64)."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, xz, yz = x * x, y * y, z * z, x * y, x * z, y * z
    if l == 1:
        t = [-C1 * y, C1 * z, -C1 * x]
    elif l == 2:
        t = [C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
    else:
        t = [C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
             C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)]
    return np.stack(t, axis=-1)


def directions(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


_FIT_DIRS = directions(300, 20240611)


def band_matrix(l, R):
    """D_l with D_l^T B_l(d) = B_l(R^T d): least squares over 300 seeded directions (float64)."""
    Y = sh_basis(l, _FIT_DIRS)            # [K, w]: rows B(d_k)^T
    Yr = sh_basis(l, _FIT_DIRS @ R)       # rows B(R^T d_k)^T  (d^T R = (R^T d)^T)
    D, res, rank, _ = np.linalg.lstsq(Y, Yr, rcond=None)  # Y D = Yr  <=>  D^T B(d_k) = B(R^T d_k)
    assert rank == 2 * l + 1
    return D


def compose64(rot=(1, 0, 0, 0), translate=(0, 0, 0), scale=1.0, pivot=None):
    """dict(q, m, log_scale, sh1, sh2, sh3, R) in float64."""
    q = np.asarray(rot, np.float64)
    q = q / np.linalg.norm(q)
    R = rot_matrix(q)
    s = float(scale)
    p = np.zeros(3) if pivot is None else np.asarray(pivot, np.float64)
    t = np.asarray(translate, np.float64)
    m = np.concatenate([s * R, (t + p - s * R @ p)[:, None]], axis=1)
    return dict(q=q, m=m.reshape(12), log_scale=np.log(s), R=R, sh1=band_matrix(1, R), sh2=band_matrix(2, R), sh3=band_matrix(3, R))


def xform64(c, flags=POSITION | ORIENT | SIZE):
    return Xform(flags, c["m"], c["q"], c["log_scale"], c["sh1"], c["sh2"], c["sh3"], dtype=np.float64)


def colour_sh(coef, d):
    """compute_color_from_sh in float64 without the final clamp: coef [16, 3] (coefficient, channel), unit d [K, 3] -> [K, 3]."""
    coef = np.asarray(coef, np.float64)
    res = C0 * coef[0][None, :] + 0.5
    for l, k0, w in BANDS:
        res = res + sh_basis(l, d) @ coef[k0:k0 + w]
    return res


def covariance(log_scales, rot):
    """compute_cov3d in float64: R(rot / |rot|) diag(exp(2 log-scale)) R^T."""
    R = rot_matrix(rot)
    S2 = np.diag(np.exp(2.0 * np.asarray(log_scales, np.float64)))
    return R @ S2 @ R.T


def qmul(a, b):
    ar, ax, ay, az = a
    br, bx, by, bz = b
    return np.array([ar * br - ax * bx - ay * by - az * bz, ar * bx + ax * br + ay * bz - az * by,
                     ar * by - ax * bz + ay * br + az * bx, ar * bz + ax * by - ay * bx + az * br])


def axis_angle(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])


def issue_rotations():
    """(name, quaternion) of the issue's rotation set: identity, +-90 and 180 degrees about each axis, 1e-4 rad about a skew axis, a
    quaternion of length 3, 32 seeded random rotations."""
    out = [("identity", np.array([1.0, 0, 0, 0]))]
    for k, ax in enumerate(np.eye(3)):
        for name, ang in (("+90", np.pi / 2), ("-90", -np.pi / 2), ("180", np.pi)):
            out.append(("%s%s" % ("xyz"[k], name), axis_angle(ax, ang)))
    out.append(("tiny_skew", axis_angle((0.3, -0.5, 0.81), 1e-4)))
    out.append(("length3", 3.0 * axis_angle((-0.2, 0.9, 0.4), 1.1)))
    rng = np.random.default_rng(77)
    for k in range(32):
        q = rng.normal(size=4)
        out.append(("random%d" % k, q / np.linalg.norm(q)))
    return out
