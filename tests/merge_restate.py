"""The cell merge (gs_abi.h "cell merge") restated in numpy.  TEST INFRASTRUCTURE ONLY: imports nothing of the library.

The f32 parts -- sigmoid, axis lengths, covariance, weight, cell coordinates -- are float32 numpy operations, one rounding each, with
oracle/np_oracle.py's expf and 3x3 helpers, written from the header's text and np_oracle.preprocess ("cov3d", "sigmoid").  The sums
are a loop over the member RANK, vectorised across the groups, in float64: every group adds its members in ascending index, one
operation at a time as the header writes them.  The finishing is an INDEPENDENT f64 model (numpy.linalg.eigh, the quaternion as the
dominant eigenvector of the rotation's 4x4 K matrix): the library's Jacobi is held against it by a margin, not bit for bit.
"""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
SH_COLS = np.array([16 + 4 * (j // 3) + j % 3 for j in range(48)])
PAD_COLS = np.array([c for c in range(80) if c not in (0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12) and c not in set(SH_COLS.tolist())])
CARRIED = np.array([c for c in range(80) if c not in set(PAD_COLS.tolist())])  # the 59 floats of a record that mean something
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # xx xy xz yy yz zz


def per_splat(rec):
    """(w float32[n], sig float32[n, 6]) of float32[n, 80] records."""
    from oracle import np_oracle as npo
    s = np.asarray(rec, F).reshape(-1, 80)
    with np.errstate(all="ignore"):
        sc = [npo.expf(s[:, 4 + k]) for k in range(3)]  # scale modifier 1
        q = [s[:, 8 + k] for k in range(4)]
        ln = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        r, x, y, z = (q[k] / ln for k in range(4))
        one, two = F(1.0), F(2.0)
        R = [[one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)],
             [two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)],
             [two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]]
        M = [[sc[rr] * R[c][rr] for rr in range(3)] for c in range(3)]
        Sig = npo.m3mul(npo.m3t(M), M)
        sig = np.stack([Sig[0][0], Sig[0][1], Sig[0][2], Sig[1][1], Sig[1][2], Sig[2][2]], 1).astype(F)
        o = s[:, 12]
        ez = npo.expf(o)
        cond = (o >= 0).astype(F)
        a = (cond * (F(1.0) / (F(1.0) + npo.expf(-o)))) + ((F(1.0) - cond) * (ez / (F(1.0) + ez)))
        A = npo.wmax(sc[0] * sc[1], npo.wmax(sc[0] * sc[2], sc[1] * sc[2]))
        w = (a * A).astype(F)
    return w, sig


def keep_of(state, mask, value, n):
    if not (mask | value):
        return np.ones(n, bool)
    return (np.asarray(state, np.uint8).astype(np.uint32) & mask) == value


def eligible_of(rec, keep):
    s = np.asarray(rec, F).reshape(-1, 80)
    w, sig = per_splat(s)
    with np.errstate(all="ignore"):
        return keep & np.isfinite(s[:, 0:3]).all(1) & np.isfinite(w) & (w > 0) & np.isfinite(sig).all(1)


def _okey(v):
    b = np.asarray(v, F).view(np.uint32).astype(np.uint64)
    return np.where(b >> 31, b ^ 0xFFFFFFFF, b ^ 0x80000000)


def _okey_value(k):
    k = np.uint64(k)
    b = (k ^ np.uint64(0x80000000)) if (k >> np.uint64(31)) else (k ^ np.uint64(0xFFFFFFFF))
    return np.array([b], np.uint64).astype(np.uint32).view(F)[0]


def _bits(v):
    return int(v).bit_length()


def grid_of(rec, keep, cell):
    """None when no splat passes the filter with a finite position; else {"lo", "inv_h", "g", "bx", "bxy", "none", "edge"}."""
    s = np.asarray(rec, F).reshape(-1, 80)
    m = keep & np.isfinite(s[:, 0:3]).all(1)
    if not m.any():
        return None
    p = s[m, 0:3]
    lo = np.array([_okey_value(_okey(p[:, k]).min()) for k in range(3)], F)
    hi = np.array([_okey_value(_okey(p[:, k]).max()) for k in range(3)], F)
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    h = F(cell)
    hmin = F(ext.max() / 1024.0 * 1.000001)
    if hmin > h:
        h = hmin
    if not h >= F(1e-30):
        h = F(1e-30) if ext.max() > 0.0 else F(1.0)
    if not np.isfinite(h):
        h = F(3.0e38)
    g = [int(min(np.floor(e / float(h)) + 1.0, 1024.0)) for e in ext]
    bx = _bits(g[0] - 1)
    bxy = bx + _bits(g[1] - 1)
    return {"lo": lo, "inv_h": F(1.0) / h, "g": g, "bx": bx, "bxy": bxy, "none": g[2] << bxy, "edge": float(h)}


def keys_of(rec, grid):
    s = np.asarray(rec, F).reshape(-1, 80)
    c = []
    with np.errstate(all="ignore"):
        for k in range(3):
            v = np.floor((s[:, k] - grid["lo"][k]) * grid["inv_h"])
            v = np.fmin(np.fmax(v, F(0.0)), F(grid["g"][k] - 1))
            c.append(np.nan_to_num(v, nan=0.0).astype(np.int64))
    return (c[2] << grid["bxy"]) | (c[1] << grid["bx"]) | c[0]


def merge(rec, state, cell, mask=0, value=0, min_members=2):
    """The pinned part of a merge: {"info", "group_of" uint32[n], "sums" float64[G, 64], "members" bool[n], "order" (the eligible ids
    in (key, id) order), "starts", "lens" (of the merged runs)}.  max_members is the caller's to check against info["largest"]."""
    s = np.ascontiguousarray(rec, F).reshape(-1, 80)
    n = s.shape[0]
    keep = keep_of(state, mask, value, n)
    info = {"eligible": 0, "groups": 0, "members": 0, "largest": 0, "cells": (0, 0, 0), "cell_edge": 0.0}
    out = {"info": info, "group_of": np.full(n, NONE, np.uint32), "sums": np.zeros((0, 64)), "members": np.zeros(n, bool),
           "order": np.zeros(0, np.int64), "starts": np.zeros(0, np.int64), "lens": np.zeros(0, np.int64)}
    grid = grid_of(s, keep, cell)
    if grid is None:
        return out
    info["cells"], info["cell_edge"] = tuple(grid["g"]), grid["edge"]
    ids = np.flatnonzero(eligible_of(s, keep))
    info["eligible"] = int(ids.size)
    if not ids.size:
        return out
    keys = keys_of(s[ids], grid)
    order = ids[np.argsort(keys, kind="stable")]
    _, starts, lens = np.unique(np.sort(keys, kind="stable"), return_index=True, return_counts=True)
    info["largest"] = int(lens.max())
    mg = lens >= min_members
    starts, lens = starts[mg], lens[mg]
    G = int(starts.size)
    info["groups"], info["members"] = G, int(lens.sum())
    out.update(order=order, starts=starts, lens=lens)
    if not G:
        return out
    w32, sig32 = per_splat(s)
    with np.errstate(all="ignore"):
        pos = s[:, 0:3].astype(np.float64)
    first = order[starts]
    c = pos[first]
    acc = np.zeros((G, 64))
    for m in range(int(lens.max())):
        act = np.flatnonzero(lens > m)
        i = order[starts[act] + m]
        out["group_of"][i] = act.astype(np.uint32)
        out["members"][i] = True
        w = w32[i].astype(np.float64)
        d = pos[i] - c[act]
        acc[act, 0] += w
        for k in range(3):
            acc[act, 1 + k] += w * d[:, k]
        for e, (k, l) in enumerate(PAIRS):
            t = d[:, k] * d[:, l]
            t = sig32[i, e].astype(np.float64) + t
            t = w * t
            acc[act, 4 + e] += t
        acc[act, 10:58] += w[:, None] * s[i][:, SH_COLS].astype(np.float64)
    acc[:, 58], acc[:, 59], acc[:, 60:63], acc[:, 63] = lens, first, c, 0.0
    out["sums"] = acc
    return out


def marked(state, members, op, bits):
    st = np.array(state, np.uint8, copy=True)
    m = members
    if op == 1:
        st[m] |= np.uint8(bits)
    elif op == 2:
        st[m] &= np.uint8(~bits & 0xFF)
    elif op == 3:
        st[m] ^= np.uint8(bits)
    elif op == 4:
        st[m] = np.uint8(bits)
    return st


# ---- the finishing: an independent f64 model -------------------------------------------------------------------------------------------
def _quat_of(Rm):
    """(r, x, y, z), unit, r >= 0, of a rotation matrix: the dominant eigenvector of its K matrix."""
    K = np.array([[Rm[0, 0] - Rm[1, 1] - Rm[2, 2], Rm[1, 0] + Rm[0, 1], Rm[2, 0] + Rm[0, 2], Rm[2, 1] - Rm[1, 2]],
                  [Rm[1, 0] + Rm[0, 1], Rm[1, 1] - Rm[0, 0] - Rm[2, 2], Rm[2, 1] + Rm[1, 2], Rm[0, 2] - Rm[2, 0]],
                  [Rm[2, 0] + Rm[0, 2], Rm[2, 1] + Rm[1, 2], Rm[2, 2] - Rm[0, 0] - Rm[1, 1], Rm[1, 0] - Rm[0, 1]],
                  [Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1], Rm[0, 0] + Rm[1, 1] + Rm[2, 2]]]) / 3.0
    _, v = np.linalg.eigh(K)
    x, y, z, r = v[:, -1]
    q = np.array([r, x, y, z])
    return -q if r < 0 else q


def rotation_of(q):
    """The projection's rotation matrix [row][column] of a quaternion (r, x, y, z) of any length, in f64."""
    r, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def model(sums):
    """The f64 model of the finishing: {"pos" [G, 3], "C" [G, 3, 3], "alpha" [G], "sh" [G, 48], "rec" float32[G, 80]: the model's own
    result rounded to f32 -- the yardstick}."""
    a = np.asarray(sums, np.float64).reshape(-1, 64)
    G = a.shape[0]
    out = {"pos": np.zeros((G, 3)), "C": np.zeros((G, 3, 3)), "alpha": np.zeros(G), "sh": np.zeros((G, 48)), "rec": np.zeros((G, 80), F)}
    for g in range(G):
        W = a[g, 0]
        mu = a[g, 1:4] / W
        Mm = np.zeros((3, 3))
        for e, (k, l) in enumerate(PAIRS):
            Mm[k, l] = Mm[l, k] = a[g, 4 + e]
        C = Mm / W - np.outer(mu, mu)
        lam, vec = np.linalg.eigh(C)
        lam, vec = lam[::-1], vec[:, ::-1]
        lam = np.maximum(lam, 1e-30)
        if np.linalg.det(vec) < 0:
            vec[:, 2] = -vec[:, 2]
        alpha = min(0.99, W / np.sqrt(lam[0] * lam[1]))
        out["pos"][g], out["C"][g], out["alpha"][g], out["sh"][g] = a[g, 60:63] + mu, C, alpha, a[g, 10:58] / W
        rec = out["rec"][g]
        rec[0:3] = out["pos"][g]
        rec[4:7] = 0.5 * np.log(lam)
        rec[8:12] = _quat_of(vec)
        rec[12] = np.log(alpha / (1.0 - alpha))
        rec[SH_COLS] = out["sh"][g]
    return out


def finish_errors(rec, mdl):
    """(cov, opacity): per group, the relative Frobenius error of R(q) diag(exp(2 s)) R(q)^T of the f32 records against the model's C,
    and the relative error of sigmoid(logit) against the model's alpha."""
    r = np.asarray(rec, F).reshape(-1, 80).astype(np.float64)
    cov, opa = np.zeros(r.shape[0]), np.zeros(r.shape[0])
    for g in range(r.shape[0]):
        Rm = rotation_of(r[g, 8:12])
        back = Rm @ np.diag(np.exp(2.0 * r[g, 4:7])) @ Rm.T
        cov[g] = np.linalg.norm(back - mdl["C"][g]) / np.linalg.norm(mdl["C"][g])
        opa[g] = abs(1.0 / (1.0 + np.exp(-r[g, 12])) - mdl["alpha"][g]) / mdl["alpha"][g]
    return cov, opa


def record_distance(a, b, mdl):
    """(cov, opacity): per group, the distance between two sets of f32 records in the measures of finish_errors: the Frobenius norm of
    the difference of their reconstructed covariances over the norm of the model's C, and the difference of their opacities over the
    model's alpha."""
    ra, rb = (np.asarray(x, F).reshape(-1, 80).astype(np.float64) for x in (a, b))
    cov, opa = np.zeros(ra.shape[0]), np.zeros(ra.shape[0])
    for g in range(ra.shape[0]):
        back = []
        for r in (ra[g], rb[g]):
            Rm = rotation_of(r[8:12])
            back.append(Rm @ np.diag(np.exp(2.0 * r[4:7])) @ Rm.T)
        cov[g] = np.linalg.norm(back[0] - back[1]) / np.linalg.norm(mdl["C"][g])
        opa[g] = abs(1.0 / (1.0 + np.exp(-ra[g, 12])) - 1.0 / (1.0 + np.exp(-rb[g, 12]))) / mdl["alpha"][g]
    return cov, opa


def ulps(a, b):
    """Distance in f32 steps between two float32 arrays of finite numbers (the total order of the bit patterns)."""
    return np.abs(_okey(np.asarray(a, F)).astype(np.int64) - _okey(np.asarray(b, F)).astype(np.int64))


# ---- the verb --------------------------------------------------------------------------------------------------------------------------
def simplified(rec, state, records, members, new_state):
    """(records, state plane, id map) after simplify(): the splats that are in no merged group, in order, then the merged records.
    The id map is the compaction's: the kept splats' old indices, then N_old + group for the merged ones (their indices between the
    insertion and the compaction)."""
    s = np.asarray(rec, F).reshape(-1, 80)
    kept = np.flatnonzero(~members).astype(np.uint32)
    G = len(records)
    st = np.concatenate([np.asarray(state, np.uint8)[kept], np.full(G, new_state, np.uint8)])
    ids = np.concatenate([kept, (s.shape[0] + np.arange(G)).astype(np.uint32)])
    return np.concatenate([s[kept], np.asarray(records, F).reshape(-1, 80)]), st, ids
