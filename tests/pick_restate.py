"""CPU restatement of gs_pick (include/gsplat/gs_abi.h): per-pixel splat queries on one frame's lists.

Input: the C oracle's GaussianData, sorted values and ranges (what oracle.render(...) returns) and a list of canvas pixels.
The arithmetic is the expression tree of tests/aux_restate.py (compute_tiles.wgsl:44-66, one f32 rounding per operation,
np_oracle.expf / np_oracle.wmin): power and alpha are evaluated vectorised over the pixel's whole tile list; the entries
with `power <= 0 and alpha >= 1/255` are then walked in list order by a scalar f32 loop that applies test, cond and the T
update AS WRITTEN (cond = 0 included) and keeps the books gs_pick reports.  There is no early exit: every candidate of the
list is visited, so an accepted entry behind a rejected one is found.  The entries left out of the loop have cond = 0 and,
alpha being in [0, 0.99], change neither T nor D; test_pick.py proves that by holding `alpha` and `depth_acc` to
aux_restate, which applies every entry.
"""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
OK, OUTSIDE_SLAB = 0, 1

RESULT_DTYPE = np.dtype([("status", np.uint32), ("list_length", np.uint32), ("hit_count", np.uint32), ("first_id", np.uint32),
                         ("first_depth", np.float32), ("max_id", np.uint32), ("max_weight", np.float32), ("median_id", np.uint32),
                         ("median_depth", np.float32), ("alpha", np.float32), ("depth_acc", np.float32), ("reserved", np.uint32)])
CONTRIB_DTYPE = np.dtype([("id", np.uint32), ("weight", np.float32)])


def restate(gdata, sorted_values, rng, W, H, ts, xy, max_contrib=0, cols=None):
    """Returns (results [n] RESULT_DTYPE, contrib [n, max_contrib] CONTRIB_DTYPE, classes) where classes is a dict of boolean
    arrays [n]: "rejected_then_accepted" (an accepted entry follows one rejected by test < 1e-4)."""
    from oracle import np_oracle as npo
    ntx = int(np.ceil(F(W) / F(ts)))
    c0, c1 = cols if cols is not None else (0, ntx)
    px0, px1 = c0 * ts, min(W, c1 * ts)
    g = np.ascontiguousarray(gdata).view(np.float32).reshape(-1, 16)
    vals = np.asarray(sorted_values)
    rng = np.asarray(rng).astype(np.int64)
    xy = np.asarray(xy).astype(np.int64).reshape(-1, 2)
    n = xy.shape[0]
    res = np.zeros(n, RESULT_DTYPE)
    con = np.zeros((n, max_contrib), CONTRIB_DTYPE)
    con["id"] = NONE
    res["first_id"] = res["max_id"] = res["median_id"] = NONE
    rta = np.zeros(n, bool)
    c255 = F(1.0 / 255.0)
    one, half, eps = F(1.0), F(0.5), F(0.0001)
    with np.errstate(all="ignore"):
        for q in range(n):
            x, y = int(xy[q, 0]), int(xy[q, 1])
            assert 0 <= x < W and 0 <= y < H
            if not (px0 <= x < px1):
                res["status"][q] = OUTSIDE_SLAB
                continue
            tile = x // ts + (y // ts) * ntx
            start = int(rng[tile - 1]) if tile > 0 else 0
            end = int(rng[tile])
            res["list_length"][q] = end - start
            ids = vals[start:end].astype(np.int64)
            rec = g[ids]
            dx = rec[:, 0] * F(W) - F(x)
            dy = rec[:, 1] * F(H) - F(y)
            cx, cy, cz, zz, op = (rec[:, c] for c in (4, 5, 6, 7, 11))
            power = F(-0.5) * (cx * dx * dx + cz * dy * dy) - cy * dx * dy
            alpha = npo.wmin(F(0.99), op * npo.expf(power)).astype(F)
            cand = np.flatnonzero((power <= 0) & (alpha >= c255))
            T, D = F(1.0), F(0.0)
            hits = 0
            max_w = F(0.0)
            rejected = False
            for e in cand:
                a, z, gid = F(alpha[e]), F(zz[e]), int(ids[e])
                test = F(T * F(one - a))
                cond = F(1.0) if test >= eps else F(0.0)
                w = F(a * T)
                D = F(D + F(F(F(cond * z) * a) * T))
                Tn = F(F(cond * test) + F(F(one - cond) * T))
                if cond == one:
                    if rejected:
                        rta[q] = True
                    if hits < max_contrib:
                        con[q, hits] = (gid, w)
                    if hits == 0:
                        res["first_id"][q], res["first_depth"][q] = gid, z
                    if hits == 0 or w > max_w:
                        max_w = w
                        res["max_id"][q], res["max_weight"][q] = gid, w
                    hits += 1
                    if res["median_id"][q] == NONE and Tn <= half:
                        res["median_id"][q], res["median_depth"][q] = gid, z
                else:
                    rejected = True
                T = Tn
            res["hit_count"][q] = hits
            res["alpha"][q] = F(one - T)
            res["depth_acc"][q] = D
    return res, con, {"rejected_then_accepted": rta}


def restate_ref(ref, W, H, ts, xy, max_contrib=0, cols=None):
    """restate() of an oracle.render(...) result."""
    return restate(ref["gdata"], ref["sorted_values"], ref["ranges"], W, H, ts, xy, max_contrib, cols)
