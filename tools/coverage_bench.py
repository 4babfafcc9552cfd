#!/usr/bin/env python3
"""GPU box: what a coverage accumulation costs at config B (6.1 M splats, 1080p, tile 16), one GPU, one process.

  python tools/coverage_bench.py [--n N] [--out FILE]

After one frame of the product path (fused blend, tight binning), over the WHOLE canvas:
  accumulate_coverage()           host end-to-end microseconds per call (the call returns when the device is done) and the
                                  accepted (pixel, entry) pairs it adds
  the same frame's blend          gs_stats.stage_us[blend] of a GS_FLAG_TIMING context rendering the same camera: the kernel that
                                  walks the same lists for the same pixels, beside the two numbers above
  the gs_pick route               the same region the only way possible without the planes: ceil(|P| / 65536) gs_pick calls with
                                  max_contrib = 256, every contributor record copied to the host
  state_coverage / read_coverage  the streaming pass over the planes and their copy to the host

No time is asserted anywhere; the numbers go to profiles/coverage.txt with the box they were measured on.
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
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--out", help="also append the report to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import gsplat
    from gsplat import _abi, synth
    n = a.n
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sp = synth.bicycle_like_torch(n, synth.BASE_SEED + 1, "cuda")
    torch.cuda.synchronize()
    pg = gsplat.PackedGaussians.__new__(gsplat.PackedGaussians)
    pg.numGaussians, pg.gaussiansBuffer, pg.sphericalHarmonicsDegree = n, sp, 3
    u = synth.orbit_camera(0, W, H).uniforms(W, H)

    def timed(fn, reps=10):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    r = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, pg, TS, flags=_abi.GS_FLAG_SPLAT_STATE | _abi.GS_FLAG_TIMING)
    r.set_option(_abi.GS_OPT_FRAMES_IN_FLIGHT, 1)
    for _ in range(3):  # the first frame grows the capacities
        r.render_uniforms(u)
        r.wait()
    st = r.stats()
    blend = st["stage_us"]["blend"]
    say("%s, config B: N = %d, %d x %d, tile %d; one frame of the product path (tight binning %d, %d instances)"
        % (torch.cuda.get_device_name(0), n, W, H, TS, st["tight_binning"], st["num_intersections"]))
    say("host end to end, median / min / max (us)")
    r.reset_coverage()
    pixels = r.accumulate_coverage()
    p = r.read_coverage()
    pairs = int(p["hits"].astype(np.uint64).sum())
    say("  accumulate_coverage(), whole canvas   %d pixels, %d accepted pairs, %d covered splats (most pairs of one splat: %d)"
        % (pixels, pairs, int((p["hits"] > 0).sum()), int(p["hits"].max())))
    ta = timed(lambda: r.accumulate_coverage())
    say("                                        %10.1f / %10.1f / %10.1f" % ta)
    say("  the same frame's blend (stage_us)     %10.1f   -- accumulate / blend = %.2f; %.0f accepted pairs per ns" % (blend, ta[0] / blend, pairs / (ta[0] * 1e3)))
    x0, y0, x1, y1 = W // 4, H // 4, 3 * W // 4, 3 * H // 4
    tq = timed(lambda: r.accumulate_coverage((x0, y0, x1, y1)))
    say("  accumulate_coverage, the central quarter (%d pixels)   %10.1f / %10.1f / %10.1f" % (((x1 - x0) * (y1 - y0),) + tq))
    mask = (np.add.outer(np.arange(H) // 3, np.arange(W) // 3) % 2 == 0).astype(np.uint8)
    tm = timed(lambda: r.accumulate_coverage(mask=mask))
    say("  accumulate_coverage, whole canvas AND a 3-pixel checkerboard mask (2 MB uploaded per call)   %10.1f / %10.1f / %10.1f" % tm)
    say("  state_coverage (17 B per splat)       %10.1f / %10.1f / %10.1f" % timed(lambda: r.state_coverage(_abi.GS_STATE_ASSIGN, 0, covered=False)))
    say("  read_coverage (%.1f MB to the host)   %10.1f / %10.1f / %10.1f" % ((p.nbytes / 1e6,) + timed(lambda: r.read_coverage(), reps=5)))
    say("  reset_coverage                        %10.1f / %10.1f / %10.1f" % timed(lambda: r.reset_coverage()))
    # the gs_pick route over the whole canvas: rows of the canvas, 65536 queries per call, every contributor record to the host
    rows = _abi.GS_PICK_MAX_QUERIES // W
    calls = 0
    hit_sum = 0
    t0 = time.perf_counter()
    for ya in range(0, H, rows):
        yb = min(H, ya + rows)
        yy, xx = np.meshgrid(np.arange(ya, yb, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
        res, con = r.pick(np.stack([xx.ravel(), yy.ravel()], axis=1), 256)
        hit_sum += int(res["hit_count"].astype(np.uint64).sum())
        calls += 1
    tp = (time.perf_counter() - t0) * 1e6
    say("  the gs_pick route: %d calls with max_contrib = 256 (%.0f MB of contributor records to the host)   %10.1f us   = %.0fx accumulate_coverage"
        % (calls, W * H * 256 * 8 / 1e6, tp, tp / ta[0]))
    say("    (its hit_count sums to %d: %s the planes' hits)" % (hit_sum, "equal to" if hit_sum == pairs else "NOT equal to"))
    r.destroy()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
