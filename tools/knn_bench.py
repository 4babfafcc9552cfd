#!/usr/bin/env python3
"""GPU box: what a nearest-neighbour search costs at config B size (6.1 M synthetic splats, a state plane), beside the neighbour count
over the same candidates and beside the host route it replaces.

  python tools/knn_bench.py [--out profiles/nearest.txt] [--n N] [--reps 7] [--mean 10] [--k 8] [--no-host] [--radius R] [--search-only]

A radius with a mean count of about `--mean` is found by bisection, as tools/neigh_bench.py does.  At that radius, in ONE run:

  gs_neigh_count (limit 2^32-1) -- the yardstick for the grid build and the candidate rate over the same candidates;
  gs_knn_search at that radius and k;
  nearest.distances() end to end with its rounds (the radius-free search), from its default start;
  the host route: export_splats (320 B per splat) + scipy.spatial.cKDTree.query(k + 1) + state_ids of the outliers.

Every device call is timed on the host around the call (it returns when the device is done): 2 warm-ups, then the median / min / max
of `reps` calls.  The BUILD (bounds, keys, sort, records, cell table, candidates, the two read-backs) is the time of the same call
refused by max_candidates = 1, which does all of that and stops before the query pass; the QUERY PASS is the difference; the
candidate rate is candidates / query pass.  distances() is timed over 3 calls after one, the host route once (it takes seconds).
The search's resolved distances are compared with the tree's (float64) as a check of the comparison itself.

--radius R skips the bisection; --search-only stops after the count's and the search's lines (an A/B of the query kernel).  The
query kernel's uniform path alone -- every splat in one cell -- is --n 131072 --radius 1000 --search-only, as for
tools/surface_bench.py (profiles/surface.txt); the default scene at 6.1 M splats is its per-lane path.
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-wgpu_amd"))
sys.path.insert(0, ROOT)

N, W, H, TS = 6_100_000, 1920, 1080, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mean", type=float, default=10.0)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (export + k-d tree + state_ids)")
    ap.add_argument("--radius", type=float, default=0.0, help="skip the bisection and take this radius")
    ap.add_argument("--search-only", action="store_true", help="the count and the search at the radius, nothing else")
    a = ap.parse_args()
    import numpy as np
    import torch
    import gsplat
    from gsplat import _abi, nearest, neighbours, synth
    n, reps, k = a.n, max(3, a.reps), a.k
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sp = synth.bicycle_like_torch(n, synth.BASE_SEED + 1, "cuda")
    torch.cuda.synchronize()
    pg = gsplat.PackedGaussians.__new__(gsplat.PackedGaussians)
    pg.numGaussians, pg.gaussiansBuffer, pg.sphericalHarmonicsDegree = n, sp, 3
    r = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, pg, TS, flags=_abi.GS_FLAG_SPLAT_STATE)
    NONE = neighbours.LIMIT_NONE

    def timed(fn, reps=reps, warm=2):
        for _ in range(warm):
            fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    def refused(fn):  # everything before the query pass
        try:
            fn()
        except _abi.GsError as e:
            assert e.code == _abi.GS_ERR_CAPACITY
            return
        raise AssertionError("the budget of 1 was not refused")

    # the radius: bisection on the mean count (a radius beyond the default budget counts as too large)
    lo, hi, radius, mean = 1e-3, 2.0, None, None
    if a.radius > 0.0:
        neighbours.count(r, a.radius)
        radius, mean = a.radius, float(neighbours.read(r).mean(dtype=np.float64))
    for _ in range(0 if radius else 16):
        mid = math.sqrt(lo * hi)
        try:
            neighbours.count(r, mid)
            m = float(neighbours.read(r).mean(dtype=np.float64))
        except _abi.GsError as e:
            assert e.code == _abi.GS_ERR_CAPACITY
            m = float("inf")
        print("  bisection: radius %.6g -> mean count %s" % (mid, m), flush=True)
        if m > a.mean:
            hi = mid
        else:
            lo, radius, mean = mid, mid, m
    fmt = "%10.1f / %10.1f / %10.1f"
    say("nearest neighbours (gs_knn_search / nearest.distances), tools/knn_bench.py")
    say("%s: N = %d, every splat a source and a query, k = %d" % (torch.cuda.get_device_name(0), n, k))
    say("host end to end around each call (it returns when the device is done): median / min / max of %d calls after 2 warm-ups, us" % reps)
    info = neighbours.count(r, radius)
    cells = info["cells"][0] * info["cells"][1] * info["cells"][2]
    say("radius %.6g: mean count %.2f; grid %s = %d cells of edge %.6g; candidates %d (%.1f per query)"
        % (radius, mean, "x".join(str(v) for v in info["cells"]), cells, info["cell_edge"], info["candidates"], info["candidates"] / n))
    cbuild = timed(lambda: refused(lambda: neighbours.count(r, radius, max_candidates=1)))
    cfull = timed(lambda: neighbours.count(r, radius, NONE))
    cq = cfull[0] - cbuild[0]
    crate = info["candidates"] / (cq * 1e-6)
    say("  gs_neigh_count: build            " + fmt % cbuild)
    say("  gs_neigh_count, limit 2^32-1     " + fmt % cfull + "   query pass = %.1f us: %.3g candidates / s" % (cq, crate))
    kinfo = nearest.search(r, k, radius)
    assert kinfo["candidates"] == info["candidates"] and kinfo["cells"] == info["cells"]
    kbuild = timed(lambda: refused(lambda: nearest.search(r, k, radius, max_candidates=1)))
    kfull = timed(lambda: nearest.search(r, k, radius))
    kq = kfull[0] - kbuild[0]
    krate = kinfo["candidates"] / (kq * 1e-6)
    say("  gs_knn_search: build             " + fmt % kbuild)
    say("  gs_knn_search, k = %-2d            " % k + fmt % kfull + "   query pass = %.1f us: %.3g candidates / s" % (kq, krate))
    say("  the search's candidate rate is %.2f of the count's over the same %d candidates; unresolved at this radius: %d of %d (%.1f %%)"
        % (krate / crate, info["candidates"], kinfo["unresolved"], n, 100.0 * kinfo["unresolved"] / n))
    for kk in (1, 32):
        if kk != k:
            full = timed(lambda: nearest.search(r, kk, radius), reps=3, warm=1)
            say("  gs_knn_search, k = %-2d            " % kk + fmt % full + "   query pass = %.1f us: %.3g candidates / s   (3 calls)"
                % (full[0] - kbuild[0], kinfo["candidates"] / ((full[0] - kbuild[0]) * 1e-6)))
    if a.search_only:
        r.destroy()
        return
    if krate < 0.25 * crate:
        say("  BELOW a quarter of the count's rate.  What bounds it: k = 1 keeps one slot and hardly inserts, so a k = 1 rate near the count's")
        say("  puts the loss on the LDS insertions and rescans; a k = 1 rate as low puts it on the gather of the per-lane walk")
    say("bytes moved (algorithmic): the build is the count's (profiles/neighbours.txt); the query pass reads N x 16 B of query records and the")
    say("  candidates' 16 B records (%.0f MB, served by the caches) and writes N x 8 B; k x 1 KB of LDS per workgroup holds the slots"
        % (info["candidates"] * 16 / 1e6))
    # the radius-free search, end to end
    out = {}

    def free():
        out.update(nearest.distances(r, k))
    d = timed(free, reps=3, warm=1)
    say("nearest.distances(k = %d), default start, end to end (3 calls after 1)   " % k + fmt % d)
    say("  rounds %d, last radius %.6g, unresolved %d, candidates over all rounds %d" % (out["rounds"], out["radius"], out["unresolved"], out["candidates"]))
    for start in (radius, 4 * out["radius"] / 2 ** (out["rounds"] - 1)):  # the radius above, and four times the default start
        o2 = {}
        d_ = timed(lambda: o2.update(nearest.distances(r, k, radius=start)), reps=3, warm=1)
        say("  ... started from radius %-9.6g " % start + fmt % d_ + "   rounds %d, candidates %d" % (o2["rounds"], o2["candidates"]))
    d2, _ = nearest.read(r)
    dist =np.sqrt(d2[np.isfinite(d2)].astype(np.float64))
    say("  k-th nearest distance: mean %.6g, std %.6g, median %.6g, max %.6g" % (dist.mean(), dist.std(), np.median(dist), dist.max()))
    # the rounds one by one, from the default start: where the time of distances() goes
    rad = out["radius"] / 2 ** (out["rounds"] - 1)
    say("  the rounds from the default start, one call each: radius, queried, candidates, unresolved, us")
    for i in range(out["rounds"]):
        t0 = time.perf_counter()
        ri = nearest.search(r, k, rad, refine=i > 0)
        us = (time.perf_counter() - t0) * 1e6
        say("    %-9.6g %9d %13d %9d %10.1f" % (rad, ri["queried"], ri["candidates"], ri["unresolved"], us))
        rad *= 2.0
    lo2 = float(np.float32(dist.mean() + 2 * dist.std()) ** 2)
    sel = timed(lambda: nearest.select(r, lo2, float("inf"), op=_abi.GS_STATE_TOGGLE), reps=21)
    say("  gs_state_knn, 5 B per splat      " + fmt % sel)
    if not a.no_host:
        from scipy.spatial import cKDTree
        workers = min(16, os.cpu_count() or 1)
        t0 = time.perf_counter()
        rec = r.export_splats()
        t1 = time.perf_counter()
        pos = np.ascontiguousarray(rec[:, 0:3], dtype=np.float64)
        tree = cKDTree(pos)
        t2 = time.perf_counter()
        dd, _ = tree.query(pos, k + 1, workers=workers)
        t3 = time.perf_counter()
        kth = dd[:, k]
        ids = np.flatnonzero(kth > kth.mean() + 2 * kth.std()).astype(np.uint32)
        r.state_ids(ids, _abi.GS_STATE_SET, _abi.GS_SPLAT_SELECTED)
        t4 = time.perf_counter()
        say("the host route, once, s: export_splats (%.2f GB) %.2f + cKDTree build %.2f + query(k + 1 = %d, %d workers) %.2f + state_ids of %d outliers %.2f = %.2f"
            % (rec.nbytes / 1e9, t1 - t0, t2 - t1, k + 1, workers, t3 - t2, ids.size, t4 - t3, t4 - t0))
        say("  against distances() %.3f s: %.0f x" % (d[0] * 1e-6, (t4 - t0) / (d[0] * 1e-6)))
        fin = np.isfinite(d2)
        rel = np.abs(np.sqrt(d2[fin].astype(np.float64)) - kth[fin]) / np.maximum(kth[fin], 1e-30)
        say("  check: the search's k-th distances against the tree's (f64), largest relative difference %.3g over %d resolved" % (rel.max(), int(fin.sum())))
    r.destroy()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
