#!/usr/bin/env python3
"""GPU box: what the cell merge and the simplify verbs cost at config B size (6.1 M synthetic splats), and what they do to the frame.

  python tools/simplify_bench.py [--out profiles/simplify.txt] [--n N] [--reps 7] [--trace DIR] [--kernels-only]

Every call is timed on the host around the call (each returns when the device is done): 2 warm-ups, then the median / min / max of
`reps` calls in milliseconds.  Reported from ONE run: the count-only probe; gs_cell_merge_device into a buffer allocated once (the
library call alone: simplify.merge_cells without `groups` adds a count-only probe to size its buffer, the line above it), at the
three edges that leave roughly 1/2, 1/4 and 1/10 of the splats (found with count-only probes, reported); the whole simplify verb at
each of them, once each on a context of its own (it changes the scene); beside that compact(0, 0) on the same scene, and once the
route there was before: export_splats to the host, a numpy moment merge (bincount sums, batched eigh: NOT the pinned arithmetic, a
timing comparator only) and a new upload; and for each edge the PSNR of the benchmark view (orbit camera 3, 1920x1080) of the
simplified scene against the unsimplified frame.
--kernels-only makes KERNEL_CALLS merges at each of the three edges, in order, and nothing else: the run to put under `rocprofv3
--kernel-trace`.  --trace DIR reads that run's kernel trace (*kernel_trace.csv below DIR) and reports gs_merge_sums_kernel's and
gs_merge_finish_kernel's own times per edge beside the end-to-end time.
"""
import argparse
import csv
import glob
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-wgpu_amd"))
sys.path.insert(0, ROOT)

N, W, H, TS = 6_100_000, 1920, 1080, 16
FACTORS = (2, 4, 10)
KERNEL_CALLS = 5
# the compiler's resource report (tools/kernel_resources.py k_merge.hip: hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, build.py's flags)
KERNEL_RESOURCES = ("gs_merge_keys_kernel: 25 VGPRs, 33 SGPRs, no scratch, no LDS, occupancy 8 waves per SIMD",
                    "gs_merge_sums_kernel: 51 VGPRs, 0 AGPRs, 96 SGPRs, no scratch, no LDS, occupancy 8 waves per SIMD",
                    "gs_merge_finish_kernel: 182 VGPRs, 0 AGPRs, 32 SGPRs, no scratch, no LDS, occupancy 2 waves per SIMD")


def kernel_times(trace_dir, name):
    """[(start ns, end ns)] of every dispatch of kernel `name` in the trace of a --kernels-only run, in time order; the caller cuts
    the list per edge (KERNEL_CALLS merges of one or more trips each)."""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if name in row.get("Kernel_Name", ""):
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    rows.sort()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --kernels-only")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import ctypes
    import numpy as np
    import torch
    import gsplat
    from gsplat import _abi, simplify, synth
    n, reps = a.n, max(3, a.reps)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        if a.out:  # written through: a later step that fails leaves what was measured
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    sp = synth.bicycle_like_torch(n, synth.BASE_SEED + 1, "cuda")
    torch.cuda.synchronize()

    def renderer():
        pg = gsplat.PackedGaussians.__new__(gsplat.PackedGaussians)
        pg.numGaussians, pg.gaussiansBuffer, pg.sphericalHarmonicsDegree = n, sp, 3
        return gsplat.Renderer(gsplat.Canvas(W, H), None, 0, pg, TS, flags=_abi.GS_FLAG_SPLAT_STATE)

    r = renderer()
    probes = [0]

    def left(edge):  # (0, None): a cell is fuller than max_members, the edge is too coarse to merge at all
        probes[0] += 1
        try:
            i = simplify.count(r, edge)
        except _abi.GsError as err:
            if err.code != _abi.GS_ERR_CAPACITY:
                raise
            return 0, None
        return n - i["members"] + i["groups"], i

    # the three edges: bisect the edge geometrically for n / factor splats left
    _, i0 = left(1e-30)
    finest = i0["cell_edge"]
    edges = []
    for factor in FACTORS:
        lo, hi = finest, finest * 1024.0
        for _ in range(14):
            mid = math.sqrt(lo * hi)
            if left(mid)[0] > n / factor:
                lo = mid
            else:
                hi = mid
        edges.append(float(np.float32(hi)))

    def merge_into(buf, edge):
        p, info = simplify._params(edge, 0, 0, 2, 0, 0, 0), _abi.GsMergeInfo()
        _abi.check(r._L.gs_cell_merge_device(r._ctx, ctypes.byref(p), buf.data_ptr(), buf.shape[0], None, None, ctypes.byref(info)))
        return info

    bufs = [torch.empty((left(e)[1]["groups"], 80), dtype=torch.float32, device="cuda") for e in edges]
    torch.cuda.synchronize()
    if a.kernels_only:
        for e, b in zip(edges, bufs):
            for _ in range(KERNEL_CALLS):
                merge_into(b, e)
        r.destroy()
        return

    def timed(fn, k=reps, warm=2):
        for _ in range(warm):
            fn()
        t = []
        for _ in range(k):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    fmt = "%9.2f / %9.2f / %9.2f"
    say("cell merge and simplify (gs_cell_merge[_device], gsplat.simplify), tools/simplify_bench.py")
    say("%s: N = %d synthetic splats, filter (0, 0), min_members 2; the finest grid's edge is %g" % (torch.cuda.get_device_name(0), n, finest))
    for k in KERNEL_RESOURCES:
        say(k)
    say("host end to end around each call (it returns when the device is done): median / min / max of %d calls after 2 warm-ups, ms" % reps)
    say("  count-only at edge %-10g                      " % edges[1] + fmt % timed(lambda: simplify.count(r, edges[1])))
    sums_rows = kernel_times(a.trace, "gs_merge_sums_kernel") if a.trace else []
    fin_rows = kernel_times(a.trace, "gs_merge_finish_kernel") if a.trace else []
    for k, (e, b) in enumerate(zip(edges, bufs)):
        info = merge_into(b, e)
        t = timed(lambda: merge_into(b, e))
        line = "  merge at edge %-10g (%8d groups of %8d members, largest %5d: %8d splats left, 1/%.2f) " % (
            e, info.groups, info.members, info.largest, n - info.members + info.groups, n / float(n - info.members + info.groups)) + fmt % t
        if a.trace:
            trips = (int(info.groups) + (1 << 18) - 1) >> 18
            want = trips * KERNEL_CALLS
            have = len(sums_rows) == len(fin_rows) == sum(((b2.shape[0] + (1 << 18) - 1) >> 18) * KERNEL_CALLS for b2 in bufs)
            if have:
                at = sum(((b2.shape[0] + (1 << 18) - 1) >> 18) * KERNEL_CALLS for b2 in bufs[:k])
                ks = sum((e1 - s1) for s1, e1 in sums_rows[at:at + want]) / 1e6 / KERNEL_CALLS
                kf = sum((e1 - s1) for s1, e1 in fin_rows[at:at + want]) / 1e6 / KERNEL_CALLS
                bytes_ = float(info.members) * 236.0 + float(info.groups) * 512.0
                line += "   sums kernel %7.3f ms (%5.2f TB/s of its 236 B per member + 512 B per group)   finish kernel %7.3f ms" % (ks, bytes_ / ks * 1e-9, kf)
            else:
                line += "   [kernel times NOT AVAILABLE: %d / %d dispatches in the trace]" % (len(sums_rows), len(fin_rows))
        say(line)
    if not a.trace:
        say("  (the sums kernel alone: not measured in this run; see --trace)")
    # the frame of the unsimplified scene
    u = synth.orbit_camera(3, W, H).uniforms(W, H)
    r.render_uniforms(u)
    r.wait()
    ref = r.read_rgba8()[..., :3].astype(np.float64)
    say("  compact(0, 0) on the same scene                    " + fmt % timed(lambda: r.compact(0, 0), 5, 1))
    say("the verb, once per edge on a context of its own, and the benchmark view (orbit camera 3) against the unsimplified frame")
    for e in edges:
        r2 = renderer()
        r2.render_uniforms(u)
        r2.wait()
        t0 = time.perf_counter()
        info, ids = simplify.simplify(r2, e)
        t1 = time.perf_counter()
        r2.render_uniforms(u)
        r2.wait()
        img = r2.read_rgba8()[..., :3].astype(np.float64)
        mse = float(((img - ref) ** 2).mean())
        say("  simplify at edge %-10g %8d -> %8d splats  %9.2f ms   PSNR %6.2f dB" % (e, n, r2.numGaussians, (t1 - t0) * 1e3, 10.0 * math.log10(255.0 ** 2 / mse) if mse else float("inf")))
        r2.destroy()
    r2 = renderer()
    t0 = time.perf_counter()
    out = simplify.simplify_to(r2, n // 4)
    t1 = time.perf_counter()
    say("  simplify_to(N / 4): %d probes, edge %g, %d splats  %9.2f ms" % (out["probes"], out["edge"] or 0.0, out["splats"], (t1 - t0) * 1e3))
    r2.destroy()
    # the route there was before, once, at the middle edge
    e = edges[1]
    t0 = time.perf_counter()
    rec = r.export_splats()
    t1 = time.perf_counter()
    pos = rec[:, 0:3].astype(np.float64)
    lo = pos.min(0)
    cell = np.floor((pos - lo) / e).astype(np.int64)
    key = (cell[:, 2] << 40) | (cell[:, 1] << 20) | cell[:, 0]
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    G = cnt.size
    sc = np.exp(rec[:, 4:7].astype(np.float64))
    srt = np.sort(sc, 1)
    w = 1.0 / (1.0 + np.exp(-rec[:, 12].astype(np.float64))) * srt[:, 1] * srt[:, 2]
    Wg = np.bincount(inv, w, G)
    mu = np.stack([np.bincount(inv, w * pos[:, k], G) for k in range(3)], 1) / Wg[:, None]
    d = pos - mu[inv]
    q = rec[:, 8:12].astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rr, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - rr * z), 2 * (x * z + rr * y)], 1),
                  np.stack([2 * (x * y + rr * z), 1 - 2 * (x * x + z * z), 2 * (y * z - rr * x)], 1),
                  np.stack([2 * (x * z - rr * y), 2 * (y * z + rr * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    Sig = np.einsum("nik,nk,njk->nij", R, sc * sc, R) + d[:, :, None] * d[:, None, :]
    C = np.stack([np.bincount(inv, w * Sig[:, i, j], G) for i in range(3) for j in range(3)], 1).reshape(G, 3, 3) / Wg[:, None, None]
    lam, vec = np.linalg.eigh(C)
    merged = np.zeros((G, 80), np.float32)
    merged[:, 0:3] = mu
    merged[:, 4:7] = 0.5 * np.log(np.maximum(lam[:, ::-1], 1e-30))
    merged[:, 8] = 1.0  # (the orientation is left out of the comparator: it only has to cost what a host would pay at least)
    al = np.minimum(0.99, Wg / np.sqrt(np.maximum(lam[:, 2] * lam[:, 1], 1e-60)))
    merged[:, 12] = np.log(al / (1 - al))
    for c in range(16, 80):
        if c % 4 != 3:
            merged[:, c] = np.bincount(inv, w * rec[:, c], G) / Wg
    t2 = time.perf_counter()
    r3 = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(merged), TS, flags=_abi.GS_FLAG_SPLAT_STATE)
    t3 = time.perf_counter()
    say("the route there was before, once, at edge %g (every cell merged, singletons too: %d splats): export_splats %.2f s (%.2f GB to the host), "
        "numpy %.2f s, a new context and upload %.2f s" % (e, G, t1 - t0, n * 320 / 1e9, t2 - t1, t3 - t2))
    r3.destroy()
    r.destroy()


if __name__ == "__main__":
    main()
