#!/usr/bin/env python3
"""GPU box: what scoring plane hypotheses costs at config B size (6.1 M synthetic splats, a state plane, one splat in ten selected).

  python tools/consensus_bench.py [--out profiles/consensus.txt] [--n N] [--reps 21] [--trace DIR] [--kernels-only]

Every call is timed on the host around the call (each returns when the device is done): 3 warm-ups, then the median / min / max of
`reps` calls in microseconds.  Timed in ONE run: consensus.score of 64, 1024 and 4096 planes (find_plane's own candidates: planes
through random splat triples) over every splat and over the selection; whole find_plane and select_plane calls; the per-hypothesis
route there was before, attributes.histogram(PLANE, -d, d, bins=1) once per plane, 64 and 1024 times; and, once, export + numpy for
64 planes.  The counts of the three routes are compared.
--kernels-only makes KERNEL_CALLS calls of each score configuration, in the order of CONFIGS, and nothing else: the run to put
under `rocprofv3 --kernel-trace`.  --trace DIR reads that run's kernel trace (*kernel_trace.csv below DIR) and reports the kernel's
own time per configuration beside the end-to-end time.
"""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-wgpu_amd"))
sys.path.insert(0, ROOT)

N, W, H, TS = 6_100_000, 1920, 1080, 16
DISTANCE = 0.1
TABLES = (64, 1024, 4096)
CONFIGS = [(h, sel) for h in TABLES for sel in (False, True)]  # the order of the --kernels-only run
KERNEL_CALLS = 5
# the issue's estimate: 10 VALU instructions per 64 tests (3 mul, 3 add, 2 compares, the ballot's bookkeeping), 1024 SIMDs, 1.34 ns per
# wave instruction (tools/microbench/README.md)
VALU_PER_64, SIMDS, NS_PER_INST = 10.0, 1024, 1.34
# the compiler's resource report for gs_consensus_kernel<PLANE> (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, build.py's flags)
KERNEL_RESOURCES = "gs_consensus_kernel<PLANE>: 114 VGPRs, 0 AGPRs, 106 SGPRs, no scratch, 16388 B of LDS per workgroup, occupancy 4 waves per SIMD"


def estimate_us(tests):
    return tests / 64.0 * VALU_PER_64 / SIMDS * NS_PER_INST * 1e-3


def kernel_times(trace_dir):
    """{config index: [us]} of the gs_consensus_kernel dispatches of a --kernels-only run, KERNEL_CALLS per configuration in order."""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if "gs_consensus_kernel" in row.get("Kernel_Name", ""):
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    rows.sort()
    if len(rows) != len(CONFIGS) * KERNEL_CALLS:
        return None, len(rows)
    return {k: [(e - s) / 1e3 for s, e in rows[k * KERNEL_CALLS:(k + 1) * KERNEL_CALLS]] for k in range(len(CONFIGS))}, len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --kernels-only")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import gsplat
    from gsplat import _abi, attributes, consensus, synth
    n, reps = a.n, max(5, a.reps)
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
    d = np.float32(DISTANCE)
    # find_plane's own candidates: planes through random triples of resident splats
    ids = np.random.default_rng(0).integers(0, n, (TABLES[-1], 3)).astype(np.uint32)
    table = consensus.planes_through(consensus._positions(r, ids.reshape(-1)).reshape(-1, 9))
    table = table[np.isfinite(table).all(axis=1)]
    table = np.ascontiguousarray(np.resize(table, (TABLES[-1], 4)))
    where_of = lambda sel: SELECTED if sel else (0, 0)  # noqa: E731
    if a.kernels_only:
        for h, sel in CONFIGS:
            for _ in range(KERNEL_CALLS):
                consensus.score(r, consensus.PLANE, table[:h], -d, d, where_of(sel))
        r.destroy()
        return

    def timed(fn, k=reps, warm=3):
        for _ in range(warm):
            fn()
        t = []
        for _ in range(k):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    fmt = "%11.1f / %11.1f / %11.1f"
    kt, found = kernel_times(a.trace) if a.trace else (None, 0)
    say("consensus (gs_attr_consensus, gsplat.consensus), tools/consensus_bench.py")
    say("%s: N = %d, a state plane with one splat in ten selected; planes through random splat triples, distance %g" % (torch.cuda.get_device_name(0), n, DISTANCE))
    say(KERNEL_RESOURCES)
    say("host end to end around each call (it returns when the device is done): median / min / max of %d calls after 3 warm-ups, us" % reps)
    if a.trace:
        say("kernel: gs_consensus_kernel's own time from a kernel trace of a run of its own (--kernels-only, %d calls per line): median, us%s"
            % (KERNEL_CALLS, "" if kt else "   [NOT AVAILABLE: %d dispatches found, %d expected]" % (found, len(CONFIGS) * KERNEL_CALLS)))
    say("estimate: %g VALU instructions per 64 tests on %d SIMDs at %.2f ns per wave instruction (the issue's figure, not a measurement)" % (VALU_PER_64, SIMDS, NS_PER_INST))
    e2e = {}
    for k, (h, sel) in enumerate(CONFIGS):
        w = where_of(sel)
        counts, matched = consensus.score(r, consensus.PLANE, table[:h], -d, d, w)
        t = timed(lambda: consensus.score(r, consensus.PLANE, table[:h], -d, d, w))
        e2e[(h, sel)] = t[0]
        tests = float(matched) * h
        line = "  score h = %4d, %s  " % (h, "1 in 10    " if sel else "every splat") + fmt % t
        if kt:
            ku = sorted(kt[k])[len(kt[k]) // 2]
            line += "   kernel %9.1f   %6.2f G tests/s   estimate %8.1f   kernel / estimate %5.2f" % (ku, tests / ku * 1e-3, estimate_us(tests), ku / estimate_us(tests))
        else:
            line += "   %6.2f G tests/s end to end   estimate %8.1f" % (tests / t[0] * 1e-3, estimate_us(tests))
        say(line + "   (%d matched, best count %d)" % (matched, int(counts.max())))
    # the whole calls
    say("  find_plane(trials = 1024), every splat             " + fmt % timed(lambda: consensus.find_plane(r, DISTANCE, 1024, 1), 7))
    say("  find_plane(trials = 1024), 1 in 10                 " + fmt % timed(lambda: consensus.find_plane(r, DISTANCE, 1024, 1, SELECTED), 7))
    say("  select_plane(trials = 1024, refine = 2), every splat" + fmt % timed(lambda: consensus.select_plane(r, DISTANCE, 1024, 1), 7, 1))
    g = consensus.select_plane(r, DISTANCE, 1024, 1)
    say("    its result: %d inliers after %d refinement rounds, plane %s" % (g["count"], g["refined"], np.array2string(g["plane"], precision=4)))
    r.write_state(plane)
    # the per-hypothesis route: one histogram pass per plane
    attrs = [attributes.attr(consensus.PLANE, p) for p in table[:1024]]
    hi_open = np.nextafter(d, np.float32(np.inf))  # the histogram's range is half open: the next f32 above d makes d itself inclusive

    def route(k):
        return [int(attributes.histogram(r, attrs[j], -d, hi_open, bins=1)[0][0]) for j in range(k)]
    t64 = timed(lambda: route(64), 7, 1)
    t1024 = timed(lambda: route(1024), 3, 1)
    say("the per-hypothesis route, in the same run: attributes.histogram(PLANE, -d, d, bins = 1) once per plane, every splat")
    say("  64 calls                                           " + fmt % t64)
    say("  extrapolated to 1024 calls (x 16, an EXTRAPOLATION)   %11.1f" % (t64[0] * 16))
    say("  1024 calls, measured                               " + fmt % t1024)
    same = route(64) == [int(c) for c in consensus.score(r, consensus.PLANE, table[:64], -d, d)[0]]
    say("  check: the 64 histogram counts equal score's: %s" % ("yes" if same else "NO"))
    # export + numpy, h = 64, once
    t0 = time.perf_counter()
    pos = np.ascontiguousarray(r.export_splats()[:, 0:3])
    t1 = time.perf_counter()
    want = np.zeros(64, np.uint64)
    for first in range(0, n, 1 << 18):
        x, y, z = (pos[first:first + (1 << 18), k][:, None] for k in range(3))
        v = ((table[None, :64, 0] * x + table[None, :64, 1] * y) + table[None, :64, 2] * z) + table[None, :64, 3]
        want += ((v >= -d) & (v <= d)).sum(axis=0).astype(np.uint64)
    t2 = time.perf_counter()
    same = bool((want == consensus.score(r, consensus.PLANE, table[:64], -d, d)[0]).all())
    say("export + numpy for h = 64, once: export_splats %.2f s (%.2f GB to the host), numpy f32 %.2f s; its counts equal score's: %s"
        % (t1 - t0, n * 320 / 1e9, t2 - t1, "yes" if same else "NO"))
    say("what was to be checked")
    ok = e2e[(1024, False)] < t1024[0] and e2e[(1024, False)] < t64[0] * 16
    say("  score at h = 1024 over every splat is faster than the per-hypothesis route of this run: %.1f us against %.1f us measured (%.1f extrapolated): %s"
        % (e2e[(1024, False)], t1024[0], t64[0] * 16, "it is, %.0f x" % (t1024[0] / e2e[(1024, False)]) if ok else "IT IS NOT"))
    r.destroy()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
