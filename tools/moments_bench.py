#!/usr/bin/env python3
"""GPU box: what the moments cost at config B size (6.1 M synthetic splats, a state plane).

  python tools/moments_bench.py [--out profiles/moments.txt] [--n N] [--reps 21] [--kernels-only]

Every call is timed on the host around the call (each returns when the device is done): 3 warm-ups, then the median / min / max of
`reps` calls in microseconds.  Timed: moments of (X, Y, Z) over every splat and over a 10 % selection, of one plane, of one record
kind; attributes.bounds() -- three summary passes over the same 12 B of position per splat, the yardstick -- in the same run and
alternated with the (X, Y, Z) moments pair by pair; and the route there was before, export_splats + numpy mean / cov.
--kernels-only makes a few calls of each and nothing else: the run to put under a kernel trace for the per-kernel times.
"""
import argparse
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
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import gsplat
    from gsplat import _abi, attributes, moments, synth
    n, reps = a.n, max(20, a.reps)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sp = synth.bicycle_like_torch(n, synth.BASE_SEED + 1, "cuda")
    torch.cuda.synchronize()
    pg = gsplat.PackedGaussians.__new__(gsplat.PackedGaussians)
    pg.numGaussians, pg.gaussiansBuffer, pg.sphericalHarmonicsDegree = n, sp, 3
    r = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, pg, TS, flags=_abi.GS_FLAG_SPLAT_STATE)
    plane = np.zeros(n, np.uint8)
    plane[::10] = _abi.GS_SPLAT_SELECTED
    r.write_state(plane)
    SELECTED = attributes.SELECTED
    xyz = [attributes.attr(k) for k in (_abi.GS_ATTR_POS_X, _abi.GS_ATTR_POS_Y, _abi.GS_ATTR_POS_Z)]
    logit = [attributes.attr(_abi.GS_ATTR_OPACITY_LOGIT)]
    calls = [("moments(X, Y, Z), every splat, 12 B per splat      ", lambda: moments.moments(r, xyz)),
             ("moments(X, Y, Z), 1 in 10, 13 B per splat          ", lambda: moments.moments(r, xyz, SELECTED)),
             ("moments(X), every splat, 4 B per splat             ", lambda: moments.moments(r, xyz[:1])),
             ("moments(OPACITY_LOGIT), every splat, 16 + 4 + 4 B  ", lambda: moments.moments(r, logit)),
             ("attributes.bounds(), every splat, 3 x 4 B per splat", lambda: attributes.bounds(r, (0, 0))),
             ("attributes.bounds(), 1 in 10, 3 x 5 B per splat    ", lambda: attributes.bounds(r, SELECTED))]
    if a.kernels_only:
        for _, fn in calls:
            for _ in range(8):
                fn()
        r.destroy()
        return

    def timed(fn, k=reps):
        for _ in range(3):
            fn()
        t = []
        for _ in range(k):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    fmt = "%9.1f / %9.1f / %9.1f"
    say("moments (gs_attr_moments), tools/moments_bench.py")
    say("%s: N = %d, a state plane with one splat in ten selected" % (torch.cuda.get_device_name(0), n))
    say("host end to end around each call (it returns when the device is done): median / min / max of %d calls after 3 warm-ups, us" % reps)
    for label, fn in calls:
        say("  " + label + "  " + fmt % timed(fn))
    mo, bo = calls[0][1], calls[4][1]
    tm, tb = [], []
    for fn in (mo, bo) * 3:
        fn()
    for k in range(4 * reps):  # alternated, pair by pair, the order swapped every pair
        for fn, t in ((mo, tm), (bo, tb))[:: 1 if k % 2 == 0 else -1]:
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
    tm.sort()
    tb.sort()
    ratio = tm[len(tm) // 2] / tb[len(tb) // 2]
    say("  alternated, %d pairs: moments(X, Y, Z) median %.1f, bounds() median %.1f us: moments / bounds = %.3f"
        % (len(tm), tm[len(tm) // 2], tb[len(tb) // 2], ratio))

    def old_route():  # export, numpy in float64
        p = r.export_splats()[:, 0:3].astype(np.float64)
        return p.mean(axis=0), np.cov(p.T, bias=True)
    old_t = timed(old_route, 5)
    say("  the route before: export_splats + numpy mean / cov    " + fmt % old_t + "   (5 calls; %.2f GB to the host)" % (n * 320 / 1e9))
    c_old, v_old = old_route()
    c_new, v_new = moments.centroid(r, (0, 0)), moments.covariance(r, (0, 0))
    say("  numpy's float64 centroid and covariance differ from the exact ones by at most %.2e and %.2e"
        % (np.abs(c_old - c_new).max(), np.abs(v_old - v_new).max()))
    say("what was to be checked")
    say("  the (X, Y, Z) moments read once what bounds() reads in three passes, and add 64-bit integer work that bounds() does not have:")
    say("  they should take no longer than twice bounds() in the same run.  Measured moments / bounds = %.3f: %s."
        % (ratio, "they do not" if ratio <= 2.0 else "THEY DO -- see the note below"))
    r.destroy()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
