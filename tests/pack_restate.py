"""numpy restatement of the packed scenes (include/gsplat/gs_abi.h "packed scenes"): the codec, the Morton order and the file.
TEST INFRASTRUCTURE ONLY.

Every expression is f32 with one rounding per written operation (numpy float32 arithmetic, division and sqrt are IEEE); the exp is
oracle/np_oracle.expf.  A chunk's minima and maxima are taken in the total order of the bit patterns (-0 below +0).  Floats are only
ever compared on their uint32 view.
"""
import numpy as np

F = np.float32
U = np.uint32
C0 = F(0.28209479177387814)
HALF_SQRT2 = F(0.70710678118654752)
SQRT2 = F(1.41421356237309505)
CHUNK = 256
KEY_LAST = 1 << 30
MARKER = "comment gsplat-packed 1"
CHUNK_PROPS = ["min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_scale_x", "min_scale_y", "min_scale_z", "max_scale_x",
               "max_scale_y", "max_scale_z", "min_r", "min_g", "min_b", "max_r", "max_g", "max_b"]
VERTEX_PROPS = ["packed_position", "packed_rotation", "packed_scale", "packed_color"]


def rest_count(degree):
    return (degree + 1) ** 2 - 1


def chunk_count(n):
    return (n + CHUNK - 1) // CHUNK


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def wmax(a, b):
    return np.where(a < b, b, a)


def wmin(a, b):
    return np.where(b < a, b, a)


def fin(v):
    v = np.asarray(v, F)
    return np.where(np.isfinite(v), v, F(0)).astype(F)


def f2u(x):
    x = np.asarray(x, F).astype(np.float64)
    with np.errstate(invalid="ignore"):
        v = np.where(np.isnan(x), 0.0, np.clip(np.trunc(np.nan_to_num(x, nan=0.0, posinf=5e9, neginf=-5e9)), 0.0, 4294967295.0))
    return v.astype(np.uint64).astype(U)


def f2i(x):
    x = np.asarray(x, F).astype(np.float64)
    with np.errstate(invalid="ignore"):
        v = np.where(np.isnan(x), 0.0, np.clip(np.trunc(np.nan_to_num(x, nan=0.0, posinf=5e9, neginf=-5e9)), -2147483648.0, 2147483647.0))
    return v.astype(np.int64)


def unorm(v, b):
    T = F(2 ** b - 1)
    with np.errstate(all="ignore"):
        return f2u(wmin(T, wmax(F(0), np.asarray(v, F) * T + F(0.5))))


def norm(v, lo, hi):
    with np.errstate(all="ignore"):
        return np.where(hi > lo, (v - lo) / (hi - lo), F(0)).astype(F)


def lerp(lo, hi, t):
    with np.errstate(all="ignore"):
        return (lo * (F(1) - t) + hi * t).astype(F)


def dn(code, b):
    return (np.asarray(code, U).astype(F) / F(2 ** b - 1)).astype(F)


def okey(v):
    b = np.ascontiguousarray(v, F).view(U)
    return b ^ np.where(b >> U(31), U(0xFFFFFFFF), U(0x80000000)).astype(U)


def okey_value(k):
    k = np.asarray(k, U)
    return np.where(k >> U(31), k ^ U(0x80000000), ~k).astype(U).view(F)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(U)


# ---- encode -------------------------------------------------------------------------------------------------------------------------
def alpha(o):
    from oracle import np_oracle as npo
    o = np.asarray(o, F)
    with np.errstate(all="ignore"):
        pos = F(1) / (F(1) + npo.expf(-o))
        ez = npo.expf(o)
        neg = ez / (F(1) + ez)
    return np.where(np.isnan(o), F(0), np.where(o >= F(0), pos, neg)).astype(F)


def rotation_word(q):
    q = fin(np.asarray(q, F).reshape(-1, 4))
    with np.errstate(all="ignore"):
        ln = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        bad = ~(ln > F(0)) | ~np.isfinite(ln)
        qn = (q / np.where(bad, F(1), ln)[:, None]).astype(F)
    qn[bad] = np.array([1, 0, 0, 0], F)
    L = np.argmax(np.abs(qn), axis=1)  # the first of equal maxima: the lowest index
    rows = np.arange(qn.shape[0])
    qn = np.where((qn[rows, L] < F(0))[:, None], -qn, qn)
    others = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[L]
    t = qn[rows[:, None], others]
    code = unorm(t * HALF_SQRT2 + F(0.5), 10)
    return (L.astype(U) << U(30)) | (code[:, 0] << U(20)) | (code[:, 1] << U(10)) | code[:, 2]


def entries(rec):
    """(p, s, c float32[n, 3], rotation words, alpha codes, replaced floats) of float32[n, 80] records."""
    f = np.asarray(rec, F).reshape(-1, 80)
    p = fin(f[:, 0:3])
    s = wmax(F(-20), wmin(F(20), fin(f[:, 4:7]))).astype(F)
    c = (fin(f[:, 16:19]) * C0 + F(0.5)).astype(F)
    carried = f[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 16, 17, 18]]
    bad = int((~np.isfinite(carried)).sum()) + int(np.isnan(f[:, 12]).sum())
    return p, s, c, rotation_word(f[:, 8:12]), unorm(alpha(f[:, 12]), 8), bad


def pack_11_10_11(v, lo, hi):
    return (unorm(norm(v[:, 0], lo[:, 0], hi[:, 0]), 11) << U(21)) | (unorm(norm(v[:, 1], lo[:, 1], hi[:, 1]), 10) << U(11)) | \
        unorm(norm(v[:, 2], lo[:, 2], hi[:, 2]), 11)


def sh_bytes(rec, degree):
    f = np.asarray(rec, F).reshape(-1, 80)
    K = rest_count(degree)
    cols = [16 + 4 * (i + 1) + c for c in range(3) for i in range(K)]
    v = f[:, cols]
    with np.errstate(all="ignore"):
        b = f2u(wmin(F(255), wmax(F(0), (fin(v) / F(8) + F(0.5)) * F(256))))
    return b.astype(np.uint8).reshape(f.shape[0], 3 * K), int((~np.isfinite(v)).sum())


def encode(rec, degree):
    """(chunks float32[C, 18], vertices uint32[n, 4], sh uint8[n, 3K], nonfinite) of the records in the given order."""
    f = np.asarray(rec, F).reshape(-1, 80)
    n = f.shape[0]
    C = chunk_count(n)
    sh, bad_sh = sh_bytes(f, degree)
    if n == 0:
        return np.zeros((0, 18), F), np.zeros((0, 4), U), sh, 0
    p, s, c, rot, a8, bad = entries(f)
    starts = np.arange(0, n, CHUNK)
    of = np.repeat(np.arange(C), CHUNK)[:n]
    chunks = np.zeros((C, 18), F)
    lohi = []
    for part, v in enumerate((p, s, c)):
        k = okey(v)
        lo, hi = okey_value(np.minimum.reduceat(k, starts, axis=0)), okey_value(np.maximum.reduceat(k, starts, axis=0))
        chunks[:, 6 * part:6 * part + 3], chunks[:, 6 * part + 3:6 * part + 6] = lo, hi
        lohi.append((lo[of], hi[of]))
    verts = np.zeros((n, 4), U)
    verts[:, 0] = pack_11_10_11(p, *lohi[0])
    verts[:, 1] = rot
    verts[:, 2] = pack_11_10_11(s, *lohi[1])
    lo, hi = lohi[2]
    verts[:, 3] = (unorm(norm(c[:, 0], lo[:, 0], hi[:, 0]), 8) << U(24)) | (unorm(norm(c[:, 1], lo[:, 1], hi[:, 1]), 8) << U(16)) | \
        (unorm(norm(c[:, 2], lo[:, 2], hi[:, 2]), 8) << U(8)) | a8
    return chunks, verts, sh, bad + bad_sh


# ---- decode -------------------------------------------------------------------------------------------------------------------------
def logit_table64():
    """The table in float64, before its one rounding to f32."""
    a = np.arange(256, dtype=np.float64)
    x = a / 255.0
    x[0], x[255] = 0.5 / 255.0, 254.5 / 255.0
    return np.log(x / (1.0 - x))


def unpack_11_10_11(w, lo, hi):
    return np.stack([lerp(lo[:, 0], hi[:, 0], dn(w >> U(21), 11)), lerp(lo[:, 1], hi[:, 1], dn((w >> U(11)) & U(1023), 10)),
                     lerp(lo[:, 2], hi[:, 2], dn(w & U(2047), 11))], axis=1)


def decode(chunks, verts, sh, degree, table):
    """float32[n, 80] records; table: the 256 logits (the library's: gs_pack_logit_table)."""
    verts = np.asarray(verts, U).reshape(-1, 4)
    n = verts.shape[0]
    K = rest_count(degree)
    out = np.zeros((n, 80), F)
    if n == 0:
        return out
    b = np.asarray(chunks, F).reshape(-1, 18)[np.repeat(np.arange(chunk_count(n)), CHUNK)[:n]]
    out[:, 0:3] = unpack_11_10_11(verts[:, 0], b[:, 0:3], b[:, 3:6])
    out[:, 4:7] = unpack_11_10_11(verts[:, 2], b[:, 6:9], b[:, 9:12])
    w = verts[:, 1]
    t = np.stack([(dn((w >> U(20)) & U(1023), 10) - F(0.5)) * SQRT2, (dn((w >> U(10)) & U(1023), 10) - F(0.5)) * SQRT2,
                  (dn(w & U(1023), 10) - F(0.5)) * SQRT2], axis=1).astype(F)
    m = np.sqrt(wmax(F(0), F(1) - ((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]))).astype(F)
    L = (w >> U(30)).astype(np.int64)
    rows = np.arange(n)
    others = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[L]
    q = np.zeros((n, 4), F)
    q[rows[:, None], others] = t
    q[rows, L] = m
    out[:, 8:12] = q
    c = verts[:, 3]
    out[:, 12] = np.asarray(table, F)[c & U(255)]
    for k, sft in enumerate((24, 16, 8)):
        out[:, 16 + k] = (lerp(b[:, 12 + k], b[:, 15 + k], dn((c >> U(sft)) & U(255), 8)) - F(0.5)) / C0
    if K:
        by = np.asarray(sh, np.uint8).reshape(n, 3 * K).astype(F)
        val = (((by + F(0.5)) / F(256) - F(0.5)) * F(8)).astype(F)
        for ch in range(3):
            for i in range(K):
                out[:, 16 + 4 * (i + 1) + ch] = val[:, ch * K + i]
    return out


# ---- Morton order -------------------------------------------------------------------------------------------------------------------
def spread3(v):
    v = np.asarray(v, np.uint64) & np.uint64(1023)
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def morton_keys(pos):
    """uint32[m] keys of float32[m, 3] positions (the selection's, in ascending id order)."""
    pos = np.asarray(pos, F).reshape(-1, 3)
    ok = np.isfinite(pos).all(axis=1)
    keys = np.full(pos.shape[0], KEY_LAST, np.uint64)
    if ok.any():
        k = okey(pos[ok])
        lo, hi = okey_value(k.min(axis=0)), okey_value(k.max(axis=0))
        with np.errstate(all="ignore"):
            q = [np.minimum(1023, f2i(norm(pos[ok, a], lo[a], hi[a]) * F(1024))) for a in range(3)]
        keys[ok] = spread3(q[0]) | (spread3(q[1]) << np.uint64(1)) | (spread3(q[2]) << np.uint64(2))
    return keys.astype(U)


def morton_order(pos):
    """The positions of the sorted selection: a stable ascending sort by key."""
    return np.argsort(morton_keys(pos), kind="stable")


# ---- the file -----------------------------------------------------------------------------------------------------------------------
def header(n, degree):
    K = rest_count(degree)
    lines = ["ply", "format binary_little_endian 1.0", MARKER, "element chunk %d" % chunk_count(n)]
    lines += ["property float " + p for p in CHUNK_PROPS]
    lines += ["element vertex %d" % n] + ["property uint " + p for p in VERTEX_PROPS]
    if K:
        lines += ["element sh %d" % n] + ["property uchar f_rest_%d" % k for k in range(3 * K)]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def file_bytes(rec, degree):
    """The whole file of the records in the given order."""
    chunks, verts, sh, _ = encode(rec, degree)
    return header(np.asarray(rec).reshape(-1, 80).shape[0], degree) + chunks.tobytes() + verts.tobytes() + sh.tobytes()


def split_file(raw):
    """(n, degree, chunks, vertices, sh) of a file with exactly the format's header."""
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    n = int([ln for ln in lines if ln.startswith("element vertex ")][0].split(" ")[2])
    nrest = sum(1 for ln in lines if ln.startswith("property uchar f_rest_"))
    degree = {0: 0, 9: 1, 24: 2, 45: 3}[nrest]
    assert raw[:end] == header(n, degree), "the header is not exactly the format's"
    C, K = chunk_count(n), rest_count(degree)
    assert len(raw) == end + C * 72 + n * 16 + n * 3 * K, "the data is not exactly the implied size"
    o = end
    chunks = np.frombuffer(raw, F, C * 18, o).reshape(C, 18)
    o += C * 72
    verts = np.frombuffer(raw, U, n * 4, o).reshape(n, 4)
    o += n * 16
    sh = np.frombuffer(raw, np.uint8, n * 3 * K, o).reshape(n, 3 * K)
    return n, degree, chunks, verts, sh
