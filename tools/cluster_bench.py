#!/usr/bin/env python3
"""GPU box: what a labelling of clusters costs at config B size (6.1 M synthetic splats, a state plane), beside a neighbour count
of the same scene and radius and beside the only route there was before (export, host connected components, state_ids).

  python tools/cluster_bench.py [--out profiles/clusters.txt] [--n N] [--reps 7] [--mean 10] [--big 0.15] [--no-host]

Two radii: the one with a mean neighbour count of about `--mean` (by bisection, as tools/neigh_bench.py finds it) and `--big`, at
which the scene's core is one cluster with hundreds of links per splat.  Every call is timed on the host around the call (it returns
when the device is done): 2 warm-ups, then the median / min / max of `reps` calls.  The BUILD (bounds, keys, sort, records, cell
table, candidates, the two read-backs) is the time of the same call refused by max_candidates = 1; what a labelling adds to it is
ROUNDS x (edge pass + flatten + one word read back) + sizes + commit, and the yardstick for one edge pass is gs_neigh_count's query
pass at limit 2^32-1 in the same run: the same candidates, the same records.  The per-kernel times come from a run of this tool
under rocprofv3 --kernel-trace --stats (profiles/clusters.txt says how).  The host route is timed once, with scipy's k-d tree.
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
    ap.add_argument("--radius", type=float, default=0.0, help="skip the bisection and take this radius")
    ap.add_argument("--big", type=float, default=0.15)
    ap.add_argument("--no-host", action="store_true", help="skip the export / host components / state_ids route")
    a = ap.parse_args()
    import numpy as np
    import torch
    import gsplat
    from gsplat import _abi, clusters, neighbours, synth
    n, reps = a.n, max(3, a.reps)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sp = synth.bicycle_like_torch(n, synth.BASE_SEED + 1, "cuda")
    torch.cuda.synchronize()
    pg = gsplat.PackedGaussians.__new__(gsplat.PackedGaussians)
    pg.numGaussians, pg.gaussiansBuffer, pg.sphericalHarmonicsDegree = n, sp, 3
    r = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, pg, TS, flags=_abi.GS_FLAG_SPLAT_STATE)
    SEL = _abi.GS_SPLAT_SELECTED

    def timed(fn, k=reps):
        for _ in range(2):
            fn()
        t = []
        for _ in range(k):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    def refused(radius):  # everything before the first round
        try:
            clusters.label(r, radius, max_candidates=1)
        except _abi.GsError as e:
            assert e.code == _abi.GS_ERR_CAPACITY
            return
        raise AssertionError("the budget of 1 was not refused")

    radius = a.radius
    if not radius:  # bisection on the mean count, as tools/neigh_bench.py
        lo, hi = 1e-3, 2.0
        for _ in range(16):
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
                lo, radius = mid, mid
    fmt = "%10.1f / %10.1f / %10.1f"
    say("clusters (gs_cluster_label / gs_state_cluster / gs_state_cluster_linked), tools/cluster_bench.py")
    say("%s: N = %d, every splat a member" % (torch.cuda.get_device_name(0), n))
    say("host end to end around each call (it returns when the device is done): median / min / max of %d calls after 2 warm-ups, us" % reps)
    for rad in (radius, a.big):
        info = clusters.label(r, rad)
        labels, sizes = clusters.read(r)
        neighbours.count(r, rad)
        c = neighbours.read(r)
        say("radius %.6g: mean neighbour count %.2f; %d clusters, largest %d, %d singletons; grid %s of edge %.6g; candidates %d (%.1f per member); rounds %d"
            % (rad, float(c.mean(dtype=np.float64)), info["clusters"], info["largest"], int((sizes == 1).sum()), "x".join(str(v) for v in info["cells"]),
               info["cell_edge"], info["candidates"], info["candidates"] / n, info["rounds"]))
        build = timed(lambda: refused(rad))
        full = timed(lambda: clusters.label(r, rad))
        cnt = timed(lambda: neighbours.count(r, rad))
        say("  build (bounds, keys, sort, records, table, candidates)   " + fmt % build)
        say("  gs_cluster_label                                         " + fmt % full + "   after the build: %.1f us in %d rounds, sizes and commit"
            % (full[0] - build[0], info["rounds"]))
        say("  gs_neigh_count, limit 2^32-1                             " + fmt % cnt + "   query pass = %.1f us: %.3g candidates / s"
            % (cnt[0] - build[0], info["candidates"] / ((cnt[0] - build[0]) * 1e-6)))
        say("  (labelling - build) / (rounds x query pass) = %.2f" % ((full[0] - build[0]) / (info["rounds"] * (cnt[0] - build[0]))))
        clusters.label(r, rad)  # the planes the selections below read
    say("the selections, on the planes of radius %.6g" % a.big)
    by_size = lambda: clusters.select(r, 1, 200, op=_abi.GS_STATE_TOGGLE, bits=SEL)
    nei = lambda: neighbours.select(r, 0, 3, op=_abi.GS_STATE_TOGGLE, bits=SEL)
    say("  gs_state_neigh, 5 B per splat                " + fmt % timed(nei, 21))
    say("  gs_state_cluster, 5 B per splat              " + fmt % timed(by_size, 21))
    r.clear_selection()
    r.select_sphere((0.0, 0.0, 0.0), 0.5)
    seeds = r.state_count(SEL, SEL)
    linked = lambda: clusters.select_linked(r, (SEL, SEL), op=_abi.GS_STATE_SET, bits=0x80)
    say("  gs_state_cluster_linked, %d seeds, 13 B per splat + the flag gather   " % seeds + fmt % timed(linked, 21))
    if not a.no_host:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
        say("the route there was, once, at radius %.6g (float64 distances: not the header's definition, a cost comparison only)" % radius)
        r.clear_selection()
        t0 = time.perf_counter()
        rec = r.export_splats()
        t1 = time.perf_counter()
        pairs = cKDTree(rec[:, 0:3].astype(np.float64)).query_pairs(radius, output_type="ndarray")
        t2 = time.perf_counter()
        k, comp = connected_components(coo_matrix((np.ones(len(pairs), np.uint8), (pairs[:, 0], pairs[:, 1])), shape=(n, n)), directed=False)
        small = np.flatnonzero(np.bincount(comp)[comp] <= 200).astype(np.uint32)
        t3 = time.perf_counter()
        r.state_ids(small, _abi.GS_STATE_SET, SEL)
        t4 = time.perf_counter()
        say("  export_splats (320 B per splat) %.0f ms, k-d tree pairs (%d) %.0f ms, components (%d) and sizes %.0f ms, state_ids (%d ids) %.0f ms: %.0f ms"
            % ((t1 - t0) * 1e3, len(pairs), (t2 - t1) * 1e3, k, (t3 - t2) * 1e3, small.size, (t4 - t3) * 1e3, (t4 - t0) * 1e3))
        r.clear_selection()
        clusters.label(r, radius)
        t0 = time.perf_counter()
        clusters.label(r, radius)
        m = clusters.select(r, 1, 200)
        t1 = time.perf_counter()
        say("  gs_cluster_label + gs_state_cluster for the same question: %.1f ms (%d selected; the host route found %d)" % ((t1 - t0) * 1e3, m, small.size))
    r.destroy()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
