#!/usr/bin/env python3
"""GPU box: what gs_grade_splats costs at config B (6.1 M splats), one GPU, one process.  Run it under a time limit:

  timeout 600 python tools/grade_bench.py [--n N] [--out FILE]

Host end-to-end times (the call returns when the device is done) of a MATRIX | OFFSET | OPACITY grade for "everything" (the (0, 0)
filter: dense, no selection) and for a 10 % sphere selection ((SELECTED, SELECTED): the splat edits' selection runs first), with the
bytes/s implied by the traffic gs_abi.h states per matched splat (MATRIX 384 B, OPACITY 8 B, OFFSET nothing more beside MATRIX;
plus 1 B of state per resident splat with a filter).  Two yardsticks in the same run, on the same context:
  * gs_transform_splats with ORIENT alone on the same two selections: 392 B per matched splat, the same read-modify-write of the
    SH record and far more arithmetic -- the grade should not be slower per matched splat;
  * the route a grade replaces: gs_export_splats to the host, a numpy edit of the 48 SH floats and the logit of every record,
    gs_upload_splats of the result (once: it takes seconds).

No time is asserted anywhere; the numbers go to profiles/grade.txt with the box they were measured on.
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
GRADE_BYTES = 384 + 8  # MATRIX 192 + 192, OPACITY 4 + 4 (gs_abi.h "colour grades")
ORIENT_BYTES = 392     # 16 + 180 each way (gs_abi.h "splat transforms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--out", help="also append the report to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import gsplat
    from gsplat import _abi, colours, synth
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
    radius = float(torch.quantile(d[:: max(1, n // 1_000_000)], 0.10))  # about 10 % of the splats
    centre = [float(v) for v in centre.cpu()]
    del d
    r = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, pg, TS, flags=_abi.GS_FLAG_SPLAT_STATE)
    del pg, sp
    SEL = _abi.GS_SPLAT_SELECTED
    m = r.select_sphere(centre, radius)
    L = _abi.load()
    cnt = ctypes.c_uint64()

    def timed(fn, reps=10):
        fn()
        fn()  # two warm-up calls: with the ten timed ones an even number, so the alternating steps below cancel
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    # the grade and (nearly) its inverse alternate over the twelve calls of timed(): the coefficients end about where they were (the
    # speed does not depend on the values, but a hundredfold gain would overflow them)
    look = dict(gain=(1.1, 0.9, 1.0), offset=(0.05, 0.05, 0.05), saturation=0.5, black=0.02, white=0.9, opacity_gain=0.5)
    back = dict(gain=(1 / 1.1, 1 / 0.9, 1.0), offset=(-0.05, -0.05, -0.05), saturation=2.0, black=-0.02, white=1.1, opacity_gain=2.0)
    grades = [colours.compose(**look), colours.compose(**back)]
    assert all(g.flags == 7 for g in grades)
    q, qi = (0.9, 0.1, -0.3, 0.2), (0.9, -0.1, 0.3, -0.2)
    orients = [_abi.compose_xform(rot=q, pivot=centre), _abi.compose_xform(rot=qi, pivot=centre)]
    for x in orients:
        x.flags = _abi.GS_XFORM_ORIENT  # ORIENT alone: the rot quaternion and SH bands 1..3
    say("%s, N = %d, sphere selection %d splats (%.2f %%); host end to end, median / min / max (us), GB/s of the stated traffic at the median"
        % (torch.cuda.get_device_name(0), n, m, 100.0 * m / n))
    med = {}
    for label, mask, value, k in (("everything (0, 0)", 0, 0, n), ("selection (SEL, SEL)", SEL, SEL, m)):
        for name, structs, call, per in (("grade  MATRIX|OFFSET|OPACITY", grades, L.gs_grade_splats, GRADE_BYTES),
                                         ("transform  ORIENT", orients, L.gs_transform_splats, ORIENT_BYTES)):
            state = {"i": 0}

            def once():
                x = structs[state["i"] % 2]
                state["i"] += 1
                _abi.check(call(r._ctx, mask, value, ctypes.byref(x), ctypes.byref(cnt)))

            t = timed(once)
            assert cnt.value == k
            total = k * per + (n if mask | value else 0)
            med[(label, name)] = t[0]
            say("  %-20s %-28s %4d B/splat  %8.3f GB  %10.1f / %10.1f / %10.1f   %7.1f GB/s   %7.4f ns per matched splat"
                % (label, name, per, total / 1e9, t[0], t[1], t[2], total / t[0] / 1e3, 1e3 * t[0] / k))
        g_us, o_us = med[(label, "grade  MATRIX|OFFSET|OPACITY")], med[(label, "transform  ORIENT")]
        say("    grade / ORIENT, time per matched splat: %.3f" % (g_us / o_us))
    # the route a grade replaces, once: export to the host, edit every record with numpy, upload again
    g = grades[0]
    A = np.array(list(g.a), np.float32).reshape(3, 3)
    dc = np.array(list(g.dc), np.float32)
    t0 = time.perf_counter()
    rec = r.export_splats()
    t1 = time.perf_counter()
    shv = rec[:, 16:80].reshape(-1, 16, 4)
    shv[:, :, 0:3] = shv[:, :, 0:3] @ A.T
    shv[:, 0, 0:3] += dc
    rec[:, 12] += np.float32(g.opacity_logit)
    t2 = time.perf_counter()
    _abi.check(L.gs_upload_splats(r._ctx, rec.ctypes.data, n))
    _abi.check(L.gs_wait(r._ctx))
    t3 = time.perf_counter()
    say("  the route it replaces, everything: gs_export_splats %.1f ms + numpy edit %.1f ms + gs_upload_splats %.1f ms = %.1f ms  (%.0f x the grade)"
        % (1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (t3 - t0),
           1e6 * (t3 - t0) / med[("everything (0, 0)", "grade  MATRIX|OFFSET|OPACITY")]))
    r.destroy()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
