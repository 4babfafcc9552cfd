#!/usr/bin/env python3
"""GPU box: what gs_transform_splats costs at config B (6.1 M splats), one GPU, one process.  Run it under a time limit:

  timeout 600 python tools/xform_bench.py [--n N] [--out FILE]

Host end-to-end times (the call returns when the device is done) of a translate-only, a rotate, a scale and a full similarity
transform, each for "everything" (the (0, 0) filter: dense, no selection) and for a 1 % sphere selection ((SELECTED, SELECTED):
the splat edits' selection runs first), with the GB/s implied by the traffic gs_abi.h states per matched splat (POSITION 24 B,
ORIENT 392 B, SIZE 28 B, plus 1 B of state per resident splat with a filter).  The yardstick, in the same run: gs_export_splats_device
of the same selection -- the same gather pattern, bytes of the same order (244 B read + 320 B written per splat).

No time is asserted anywhere; the numbers go to profiles/transform_ops.txt with the box they were measured on.
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-wgpu_amd"))
sys.path.insert(0, ROOT)

N, W, H, TS = 6_100_000, 1920, 1080, 16
BYTES = {1: 24, 2: 392, 4: 28}  # read + written per matched splat and part (gs_abi.h "splat transforms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--out", help="also append the report to this file")
    a = ap.parse_args()
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
    centre = sp[:, 0:3].median(dim=0).values
    d = (sp[:, 0:3] - centre).norm(dim=1)
    radius = float(torch.quantile(d[:: max(1, n // 1_000_000)], 0.01))  # about 1 % of the splats
    centre = [float(v) for v in centre.cpu()]
    del d
    r = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, pg, TS, flags=_abi.GS_FLAG_SPLAT_STATE)
    SEL = _abi.GS_SPLAT_SELECTED
    m = r.select_sphere(centre, radius)
    L = _abi.load()
    cnt = ctypes.c_uint64()

    def timed(fn, reps=10):
        fn()
        fn()  # two warm-up calls: with the ten timed ones an even number, so the alternating scale steps below cancel
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    q = (0.9, 0.1, -0.3, 0.2)
    # scale steps alternate 1.25 / 0.8 over the twelve calls of timed(): the log-scales end where they were (up to rounding; the
    # speed does not depend on the values)
    kinds = [("translate", dict(translate=(0.01, -0.02, 0.03)), None), ("rotate", dict(rot=q, pivot=centre), None),
             ("scale", dict(scale=1.25, pivot=centre), dict(scale=0.8, pivot=centre)),
             ("full", dict(rot=q, translate=(0.01, -0.02, 0.03), scale=1.25, pivot=centre),
              dict(rot=q, translate=(0.01, -0.02, 0.03), scale=0.8, pivot=centre))]
    say("%s, N = %d, sphere selection %d splats (%.2f %%); host end to end, median / min / max (us), GB/s of the stated traffic at the median"
        % (torch.cuda.get_device_name(0), n, m, 100.0 * m / n))
    rates = {}
    for label, mask, value, k in (("everything (0, 0)", 0, 0, n), ("selection (SEL, SEL)", SEL, SEL, m)):
        for name, kw, kw2 in kinds:
            xs = [_abi.compose_xform(**kw)] + ([_abi.compose_xform(**kw2)] if kw2 else [])
            state = {"i": 0}

            def call():
                x = xs[state["i"] % len(xs)]
                state["i"] += 1
                _abi.check(L.gs_transform_splats(r._ctx, mask, value, ctypes.byref(x), ctypes.byref(cnt)))

            t = timed(call)
            assert cnt.value == k
            per = sum(b for f, b in BYTES.items() if xs[0].flags & f)
            total = k * per + (n if mask | value else 0)
            rates[(label, name)] = total / t[0] / 1e3
            say("  %-20s %-9s flags %d  %4d B/splat  %8.3f GB  %10.1f / %10.1f / %10.1f   %7.1f GB/s"
                % (label, name, xs[0].flags, per, total / 1e9, t[0], t[1], t[2], rates[(label, name)]))
    # the yardstick: gs_export_splats_device of the same two selections
    for label, mask, value, k in (("everything (0, 0)", 0, 0, n), ("selection (SEL, SEL)", SEL, SEL, m)):
        dst = torch.empty((k, 80), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def export():
            _abi.check(L.gs_export_splats_device(r._ctx, mask, value, dst.data_ptr(), k, ctypes.byref(cnt), None))

        t = timed(export)
        total = k * 564 + (n if mask | value else 0)
        rate = total / t[0] / 1e3
        say("  %-20s export_splats_device   564 B/splat  %8.3f GB  %10.1f / %10.1f / %10.1f   %7.1f GB/s"
            % (label, total / 1e9, t[0], t[1], t[2], rate))
        say("    full transform / export, GB/s: %.2f" % (rates[(label, "full")] / rate))
        del dst
    r.destroy()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
