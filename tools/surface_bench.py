#!/usr/bin/env python3
"""GPU box: what a surface estimate costs at config B size (6.1 M synthetic splats, a state plane), beside the neighbour count over
the same candidates and beside the host route it replaces.

  python tools/surface_bench.py [--out profiles/surface.txt] [--n N] [--reps 7] [--means 10,30] [--no-host] [--trace-run]

For each mean count of `--means` a radius is found by bisection, as tools/neigh_bench.py does.  At that radius, in ONE run:

  gs_neigh_count (limit 2^32-1) -- the yardstick for the grid build and the candidate rate over the same candidates;
  gs_surface_estimate without and with GS_SURFACE_KEEP_SUMS, and with GS_SURFACE_ORIENT;
  gs_surface_read, gs_state_surface beside gs_state_knn;
  the host route, once: export_splats (320 B per splat) + scipy.spatial.cKDTree + a PCA per point over its k nearest + state_ids.

Every device call is timed on the host around the call (it returns when the device is done): 2 warm-ups, then the median / min / max
of `reps` calls.  The BUILD (bounds, keys, sort, records, cell table, candidates, the two read-backs) is the time of the same call
refused by max_candidates = 1, which does all of that and stops before anything is written; what remains of an estimate is its
init, query and finishing kernels.  --trace-run does three estimates per radius and nothing else: run it under
`rocprofv3 --kernel-trace --stats` for the kernels one by one (the query pass alone, the finishing pass alone).
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
    ap.add_argument("--means", default="10,30")
    ap.add_argument("--radii", default=None, help="skip the bisection: the radii to use, one per mean")
    ap.add_argument("--no-host", action="store_true", help="skip the host route (export + k-d tree + PCA + state_ids)")
    ap.add_argument("--trace-run", action="store_true", help="three estimates per radius and nothing else (for a kernel trace)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import gsplat
    from gsplat import _abi, nearest, neighbours, surface, synth
    n, reps = a.n, max(3, a.reps)
    means = [float(v) for v in a.means.split(",")]
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

    def radius_for_mean(target):  # bisection on the mean count (a radius beyond the default budget counts as too large)
        lo, hi, radius, mean = 1e-3, 2.0, None, None
        for _ in range(16):
            mid = math.sqrt(lo * hi)
            try:
                neighbours.count(r, mid)
                m = float(neighbours.read(r).mean(dtype=np.float64))
            except _abi.GsError as e:
                assert e.code == _abi.GS_ERR_CAPACITY
                m = float("inf")
            print("  bisection: radius %.6g -> mean count %s" % (mid, m), flush=True)
            if m > target:
                hi = mid
            else:
                lo, radius, mean = mid, mid, m
        return radius, mean

    if a.radii:
        radii = [(float(v), None) for v in a.radii.split(",")]
    else:
        radii = [radius_for_mean(m) for m in means]
    if a.trace_run:
        for radius, _ in radii:
            for _ in range(3):
                neighbours.count(r, radius, NONE)
                surface.estimate(r, radius)
                surface.estimate(r, radius, keep_sums=True)
            surface.select(r, "planarity", 0.5, float("inf"), op=_abi.GS_STATE_TOGGLE)
            nearest.select(r, 0.0, 1.0, op=_abi.GS_STATE_TOGGLE)
        r.destroy()
        return
    fmt = "%10.1f / %10.1f / %10.1f"
    say("surface (gs_surface_estimate / gs_state_surface), tools/surface_bench.py")
    say("%s: N = %d, every splat a source and a query" % (torch.cuda.get_device_name(0), n))
    say("host end to end around each call (it returns when the device is done): median / min / max of %d calls after 2 warm-ups, us" % reps)
    for radius, mean in radii:
        info = neighbours.count(r, radius)
        if mean is None:
            mean = float(neighbours.read(r).mean(dtype=np.float64))
        cells = info["cells"][0] * info["cells"][1] * info["cells"][2]
        say("radius %.6g: mean count %.2f; grid %s = %d cells of edge %.6g; candidates %d (%.1f per query)"
            % (radius, mean, "x".join(str(v) for v in info["cells"]), cells, info["cell_edge"], info["candidates"], info["candidates"] / n))
        cbuild = timed(lambda: refused(lambda: neighbours.count(r, radius, max_candidates=1)))
        cfull = timed(lambda: neighbours.count(r, radius, NONE))
        cq = cfull[0] - cbuild[0]
        crate = info["candidates"] / (cq * 1e-6)
        say("  gs_neigh_count: build                  " + fmt % cbuild)
        say("  gs_neigh_count, limit 2^32-1           " + fmt % cfull + "   query pass = %.1f us: %.3g candidates / s" % (cq, crate))
        sinfo = surface.estimate(r, radius)
        assert sinfo["candidates"] == info["candidates"] and sinfo["cells"] == info["cells"]
        sbuild = timed(lambda: refused(lambda: surface.estimate(r, radius, max_candidates=1)))
        say("  gs_surface_estimate: build             " + fmt % sbuild)
        for name, kw in (("                   ", {}), (", KEEP_SUMS       ", dict(keep_sums=True)), (", ORIENT          ", dict(toward=(0.0, 0.0, 0.0)))):
            full = timed(lambda: surface.estimate(r, radius, **kw))
            sq = full[0] - sbuild[0]
            say("  gs_surface_estimate%s " % name + fmt % full + "   init + query + finish = %.1f us: %.3g candidates / s, %.2f x the count's query pass"
                % (sq, info["candidates"] / (sq * 1e-6), sq / cq))
        say("  unresolved (count < 3) at this radius: %d of %d (%.1f %%)" % (sinfo["unresolved"], n, 100.0 * sinfo["unresolved"] / n))
        rd = timed(lambda: surface.read(r), reps=3, warm=1)
        say("  gs_surface_read, 28 B per splat        " + fmt % rd + "   (3 calls)")
    normal, eig, count = surface.read(r)
    ok = count >= 3
    with np.errstate(all="ignore"):
        pla = (eig[:, 1] - eig[:, 2]) / eig[:, 0]
    say("  planarity over the %d resolved: median %.3f, above 0.5: %.1f %%" % (int(ok.sum()), float(np.median(pla[ok])), 100.0 * float((pla[ok] >= 0.5).mean())))
    sel = timed(lambda: surface.select(r, "planarity", 0.5, float("inf"), op=_abi.GS_STATE_TOGGLE), reps=21)
    say("  gs_state_surface PLANARITY, 17 B per splat " + fmt % sel)
    sel = timed(lambda: surface.select(r, "facing", 0.9, float("inf"), axis=(0, 1, 0), op=_abi.GS_STATE_TOGGLE), reps=21)
    say("  gs_state_surface FACING, 17 B per splat    " + fmt % sel)
    nearest.search(r, 8, radii[0][0])
    sel = timed(lambda: nearest.select(r, 0.0, 1.0, op=_abi.GS_STATE_TOGGLE), reps=21)
    say("  gs_state_knn, 5 B per splat                " + fmt % sel)
    est_us = timed(lambda: surface.estimate(r, radii[-1][0]), reps=3, warm=0)[0]
    if not a.no_host:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            cKDTree = None
        workers = min(16, os.cpu_count() or 1)
        k = int(round(means[-1]))
        t0 = time.perf_counter()
        rec = r.export_splats()
        t1 = time.perf_counter()
        pos = np.ascontiguousarray(rec[:, 0:3], dtype=np.float64)
        if cKDTree is not None:
            tree = cKDTree(pos)
            t2 = time.perf_counter()
            _, idx = tree.query(pos, k + 1, workers=workers)
            t3 = time.perf_counter()
            planar = np.zeros(n, bool)
            for c0 in range(0, n, 1 << 19):  # a PCA per point over its k nearest, in chunks that fit the host
                nb = pos[idx[c0:c0 + (1 << 19), 1:]]
                nb -= nb.mean(axis=1, keepdims=True)
                lam = np.linalg.eigvalsh(np.einsum("nka,nkb->nab", nb, nb) / k)
                planar[c0:c0 + (1 << 19)] = (lam[:, 1] - lam[:, 0]) >= 0.5 * lam[:, 2]
            t4 = time.perf_counter()
            ids = np.flatnonzero(planar).astype(np.uint32)
            r.state_ids(ids, _abi.GS_STATE_SET, _abi.GS_SPLAT_SELECTED)
            t5 = time.perf_counter()
            say("the host route, once, s: export_splats (%.2f GB) %.2f + cKDTree build %.2f + query(k + 1 = %d, %d workers) %.2f + PCA per point %.2f + state_ids of %d planar %.2f = %.2f"
                % (rec.nbytes / 1e9, t1 - t0, t2 - t1, k + 1, workers, t3 - t2, t4 - t3, ids.size, t5 - t4, t5 - t0))
            say("  against gs_surface_estimate + gs_state_surface at the last radius, %.4f s: %.0f x" % ((est_us + sel[0]) * 1e-6, (t5 - t0) / ((est_us + sel[0]) * 1e-6)))
        else:
            say("scipy is not installed: no k-d tree; export_splats took %.2f s" % (t1 - t0))
    r.destroy()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
