#!/usr/bin/env python3
"""GPU box: what a neighbour count costs at config B size (6.1 M synthetic splats, a state plane), and the work budget it implies.

  python tools/neigh_bench.py [--out profiles/neighbours.txt] [--n N] [--reps 7] [--mean 10]

A radius with a mean count of about `--mean` is found by bisection.  At that radius, for limit 16 and 2^32-1, every call is timed
on the host around the call (it returns when the device is done): 2 warm-ups, then the median / min / max of `reps` calls.  The BUILD
(bounds, keys, sort, records, cell table, candidates, the two read-backs) is the time of the same call refused by max_candidates = 1,
which does all of that and stops before the query pass; the QUERY PASS is the difference.  The candidate rate is candidates / query
pass at limit 2^32-1; the default budget is the largest power of two that rate finishes in 1 s, the slice the largest in 50 ms.
gs_state_neigh is timed next to gs_state_coverage in the same run.
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
    a = ap.parse_args()
    import numpy as np
    import torch
    import gsplat
    from gsplat import _abi, neighbours, synth
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
    NONE, SEL = neighbours.LIMIT_NONE, _abi.GS_SPLAT_SELECTED

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

    def refused(radius):  # everything before the query pass
        try:
            neighbours.count(r, radius, max_candidates=1)
        except _abi.GsError as e:
            assert e.code == _abi.GS_ERR_CAPACITY
            return
        raise AssertionError("the budget of 1 was not refused")

    # the radius: bisection on the mean count (a radius beyond the default budget counts as too large)
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
        if m > a.mean:
            hi = mid
        else:
            lo, radius, mean = mid, mid, m
    fmt = "%10.1f / %10.1f / %10.1f"
    say("neighbourhoods (gs_neigh_count / gs_state_neigh), tools/neigh_bench.py")
    say("%s: N = %d, every splat a source and a query" % (torch.cuda.get_device_name(0), n))
    say("host end to end around each call (it returns when the device is done): median / min / max of %d calls after 2 warm-ups, us" % reps)
    info = neighbours.count(r, radius)
    c = neighbours.read(r)
    cells = info["cells"][0] * info["cells"][1] * info["cells"][2]
    say("radius %.6g: mean count %.2f, max %d; grid %s = %d cells of edge %.6g; candidates %d (%.1f per query)"
        % (radius, mean, int(c.max()), "x".join(str(v) for v in info["cells"]), cells, info["cell_edge"], info["candidates"], info["candidates"] / n))
    build = timed(lambda: refused(radius))
    say("  build (bounds, keys, sort, records, table, candidates)   " + fmt % build)
    rate = None
    for limit in (16, NONE):
        full = timed(lambda: neighbours.count(r, radius, limit))
        q_us = full[0] - build[0]
        tests = info["candidates"]
        say("  count, limit %-10d                                 " % limit + fmt % full
            + "   query pass = %.1f us" % q_us + ("" if limit != NONE else ": %.3g candidates / s" % (tests / (q_us * 1e-6))))
        if limit == NONE:
            rate = tests / (q_us * 1e-6)
    passes = (sum((v - 1).bit_length() for v in info["cells"][:2]) + info["cells"][2].bit_length() + 7) // 8
    blocks = min(cells, 1 << 24)
    build_bytes = n * (13 + 13 + 8 + 4 + 16 * passes + 8 + 12 + 20 + 16) + 8 * blocks
    say("bytes moved (algorithmic): build %.0f MB = N x (13 bounds + 21 keys + 4 + %d x 16 sort + 40 records + 16 candidates) + 8 x %d table entries;"
        % (build_bytes / 1e6, passes, blocks))
    say("  query pass %.0f MB of records and counts (N x 20) and %.0f MB of candidate records (16 B each, served by the caches)"
        % (n * 20 / 1e6, info["candidates"] * 16 / 1e6))
    say("for comparison, in the same run")
    cov = lambda: r.state_coverage(_abi.GS_STATE_TOGGLE, SEL, min_hits=1)
    nei = lambda: neighbours.select(r, 0, 3, op=_abi.GS_STATE_TOGGLE, bits=SEL)
    say("  gs_state_coverage, 17 B per splat   " + fmt % timed(cov, 21))
    say("  gs_state_neigh, 5 B per splat       " + fmt % timed(nei, 21))
    budget = 1 << int(math.floor(math.log2(rate * 1.0)))
    piece = 1 << int(math.floor(math.log2(rate * 0.05)))
    say("work budget from the rate %.3g candidates / s:" % rate)
    say("  GS_NEIGH_DEFAULT_CANDIDATES = 2^%d (the largest power of two done in 1 s: %.2f s)" % (budget.bit_length() - 1, budget / rate))
    say("  GS_NEIGH_SLICE_CANDIDATES   = 2^%d (the largest power of two done in 50 ms: %.1f ms)" % (piece.bit_length() - 1, piece / rate * 1e3))
    r.destroy()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
