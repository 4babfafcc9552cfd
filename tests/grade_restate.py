"""numpy restatement of the colour grades (include/gsplat/gs_abi.h "colour grades").  TEST INFRASTRUCTURE ONLY.

  * compose64(): the double expressions gs_grade_compose must evaluate and their f32 roundings;
  * apply(): the per-splat definition of gs_grade_splats on float32 [n, 80] records, every expression in f32 with one rounding per
    written operation, left to right, so that the kernel (k_grade.hip) can be held to it on the uint32 view;
  * touched_floats(): the record floats a flag set writes.
"""
import numpy as np

F = np.float32
MATRIX, OFFSET, OPACITY = 0x1, 0x2, 0x4
C0 = 0.28209479177387814
LUMA = (0.2126, 0.7152, 0.0722)

SH_FLOATS = [16 + 4 * k + c for k in range(16) for c in range(3)]
DC_FLOATS = [16, 17, 18]
OPACITY_FLOAT = 12


class Grade:
    """The numbers of a gs_grade as numpy arrays (f32 by default; f64 for the yardstick of the convention test)."""

    def __init__(self, flags, a, dc, opacity_logit, dtype=F):
        self.flags = int(flags)
        self.a = np.asarray(a, dtype).reshape(3, 3)
        self.dc = np.asarray(dc, dtype).reshape(3)
        self.opacity_logit = dtype(opacity_logit)
        self.dtype = dtype

    @staticmethod
    def from_struct(g):
        return Grade(g.flags, list(g.a), list(g.dc), g.opacity_logit)

    def with_flags(self, flags):
        return Grade(flags, self.a, self.dc, self.opacity_logit, self.dtype)

    def transposed(self):
        return Grade(self.flags, self.a.T, self.dc, self.opacity_logit, self.dtype)


def touched_floats(flags):
    return sorted(set((SH_FLOATS if flags & MATRIX else []) + (DC_FLOATS if flags & OFFSET else []) + ([OPACITY_FLOAT] if flags & OPACITY else [])))


def compose64(gain=None, offset=None, saturation=1.0, black=0.0, white=1.0, opacity_gain=1.0):
    """dict(A, o, dc, opacity_logit) in float64, (a, dc32, opacity_logit32) their f32 roundings and the flags, for f32 INPUTS (each
    argument is rounded to f32 first, as the C call receives it)."""
    g = np.ones(3) if gain is None else np.asarray(gain, F).astype(np.float64)
    off = np.zeros(3) if offset is None else np.asarray(offset, F).astype(np.float64)
    sat, blk, wht, og = (float(F(v)) for v in (saturation, black, white, opacity_gain))
    s = 1.0 / (wht - blk)
    A = np.empty((3, 3))
    o = np.empty(3)
    dc = np.empty(3)
    for c in range(3):
        for j in range(3):
            delta = 1.0 if c == j else 0.0
            A[c, j] = (g[c] * (sat * delta + (1.0 - sat) * LUMA[j])) * s
        o[c] = off[c] - (g[c] * blk) * s
        dc[c] = ((((A[c, 0] + A[c, 1]) + A[c, 2]) * 0.5 + o[c]) - 0.5) / C0
    lg = float(np.log(og))
    a32, dc32, lg32 = A.astype(F), dc.astype(F), F(lg)
    flags = ((0 if np.array_equal(a32, np.eye(3, dtype=F)) else MATRIX) | (OFFSET if (dc32 != 0).any() else 0) |
             (0 if og == 1.0 else OPACITY))
    return dict(A=A, o=o, dc=dc, opacity_logit=lg, a=a32, dc32=dc32, opacity_logit32=lg32, flags=flags)


def grade64(c, flags=None):
    """The float64 Grade of a compose64 result."""
    return Grade(c["flags"] if flags is None else flags, c["A"], c["dc"], c["opacity_logit"], dtype=np.float64)


def apply(rec, x, sel=None):
    """The records after gs_grade_splats(x) on the rows where sel is true (None: all).  Arithmetic in x.dtype; the result is
    float32 [n, 80] (an f64 Grade rounds each record float once).  Untouched floats keep their bit patterns."""
    src = np.ascontiguousarray(rec, dtype=F).reshape(-1, 80)
    out = src.copy()
    rows = np.arange(src.shape[0]) if sel is None else np.flatnonzero(sel)
    if rows.size == 0 or not x.flags:
        return out
    s = src[rows].astype(x.dtype)
    a = x.a
    new = {}
    with np.errstate(all="ignore"):
        if x.flags & MATRIX:
            for k in range(16):
                r, g, b = (s[:, 16 + 4 * k + c] for c in range(3))
                for c in range(3):
                    new[16 + 4 * k + c] = (a[c, 0] * r + a[c, 1] * g) + a[c, 2] * b
        if x.flags & OFFSET:
            for c in range(3):
                v = new[16 + c] if x.flags & MATRIX else s[:, 16 + c]
                if x.dtype is F:
                    v = v.astype(F)  # (already f32: MATRIX's output is rounded before the offset is added)
                new[16 + c] = v + x.dc[c]
        if x.flags & OPACITY:
            new[OPACITY_FLOAT] = s[:, OPACITY_FLOAT] + x.opacity_logit
    for col, v in new.items():
        out[rows, col] = v.astype(F)
    return out


def colour_sh(rec, dirs):
    """compute_color_from_sh in float64 WITHOUT the final clamp: records [n, 80], unit dirs [n, 3] (one per record) -> [n, 3]."""
    import xform_restate as xr
    rec = np.asarray(rec, np.float64)
    coef = np.stack([rec[:, 16 + 4 * k:16 + 4 * k + 3] for k in range(16)], axis=1)  # [n, 16, 3]
    res = C0 * coef[:, 0, :] + 0.5
    for l, k0, w in xr.BANDS:
        res = res + np.einsum("nw,nwc->nc", xr.sh_basis(l, dirs), coef[:, k0:k0 + w, :])
    return res
