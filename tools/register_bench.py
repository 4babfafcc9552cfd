#!/usr/bin/env python3
"""GPU box: what a registration step costs at config B size (6.1 M synthetic splats, a state plane, one splat in ten selected).

  python tools/register_bench.py [--out profiles/register.txt] [--n N] [--reps 21] [--kernels-only]

Every call is timed on the host around the call (each returns when the device is done): 3 warm-ups, then the median / min / max of
`reps` calls in microseconds.  Timed in ONE run: pair_moments over every splat and over the selection, on the ctx's own nearest plane;
gs_attr_moments of (X, Y, Z), the yardstick kernel (the same accumulators, 9 instead of 21, no gather); a whole register.step (search,
pair moments, fit, transform) of the selection onto the rest; and the route there was before for the same step: export_splats, a host
k-d tree (scipy, when it is installed), a numpy Kabsch, and the re-upload with the state plane written back.  Beside them, in the
same run, the point-to-plane metric: pair_plane_moments over every splat and over the selection on the ctx's own nearest and surface
normal planes, a whole register.plane_step, and register.align under both metrics from one displaced start (0.1 degrees, 0.3 of the
radius: within the radius everywhere in the scene) with the steps each takes and what is left of the displacement.
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
# the compiler's resource report for gs_pairs_kernel (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, build.py's flags)
KERNEL_RESOURCES = "gs_pairs_kernel: 158 VGPRs, 0 AGPRs, 85 SGPRs, no scratch, no spill, 3376 B of LDS per workgroup, occupancy 3 waves per SIMD"
PLANE_RESOURCES = "gs_plane_pairs_kernel<0, 29>: 214 VGPRs, 0 AGPRs, 88 SGPRs, no scratch, no spill, 4656 B of LDS per workgroup, occupancy 2 waves per SIMD"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import ctypes
    import numpy as np
    import torch
    import gsplat
    from gsplat import _abi, attributes, moments, nearest, register, surface, synth
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
    SELECTED, REST = attributes.SELECTED, register.UNSELECTED
    xyz = [attributes.attr(k) for k in (_abi.GS_ATTR_POS_X, _abi.GS_ATTR_POS_Y, _abi.GS_ATTR_POS_Z)]
    # one search of every splat among all at the library's own starting radius: the plane the two pair_moments timings read
    info = nearest.distances(r, 1, max_rounds=1)
    radius = info["radius"]
    every, tenth = register.pair_moments(r, (0, 0)), register.pair_moments(r, SELECTED)
    # the normals the plane metric reads: one estimate over every splat at three times that radius
    sinfo = surface.estimate(r, 3.0 * radius)
    pivot = moments.centroid(r, SELECTED).astype(np.float32)
    pevery, ptenth = register.pair_plane_moments(r, (0, 0), pivot=pivot), register.pair_plane_moments(r, SELECTED, pivot=pivot)
    calls = [("pair_plane_moments, every splat, 16 B + a 28 B gather      ", lambda: register.pair_plane_moments(r, (0, 0), pivot=pivot)),
             ("pair_plane_moments, 1 in 10, 17 B + a gather for 1/10      ", lambda: register.pair_plane_moments(r, SELECTED, pivot=pivot)),
             ("pair_moments, every splat, 16 B + a 12 B gather per splat ", lambda: register.pair_moments(r, (0, 0))),
             ("pair_moments, 1 in 10, 17 B per splat + a gather for 1/10 ", lambda: register.pair_moments(r, SELECTED)),
             ("moments(X, Y, Z), every splat, 12 B per splat (yardstick) ", lambda: moments.moments(r, xyz)),
             ("moments(X, Y, Z), 1 in 10, 13 B per splat                 ", lambda: moments.moments(r, xyz, SELECTED))]
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

    fmt = "%11.1f / %11.1f / %11.1f"
    say("registration (gs_pair_moments, gsplat.register), tools/register_bench.py")
    say("%s: N = %d, a state plane with one splat in ten selected" % (torch.cuda.get_device_name(0), n))
    say(KERNEL_RESOURCES)
    say(PLANE_RESOURCES)
    say("the nearest plane: one search of every splat among all at radius %.4g, %d of %d unresolved (NONE: unpaired)" % (radius, info["unresolved"], n))
    say("  paired: %d of %d matched (every splat), %d of %d (1 in 10)" % (every["paired"], every["matched"], tenth["paired"], tenth["matched"]))
    say("the normal plane: one estimate of every splat among all at radius %.4g, %d of %d unresolved (NaN: unpaired)" % (3.0 * radius, sinfo["unresolved"], n))
    say("  plane metric paired: %d of %d matched (every splat), %d of %d (1 in 10)" % (pevery["paired"], pevery["matched"], ptenth["paired"], ptenth["matched"]))
    pos = r.export_splats()[:, 0:3].copy()
    near = nearest.read(r)[1]
    same = all(register.host_pair_moments(pos, near, plane, w) == m for w, m in (((0, 0), every), (SELECTED, tenth)))
    nrm = surface.read(r)[0]
    psame = all(register.host_pair_plane_moments(pos, near, nrm, plane, w, pivot=pivot) == m for w, m in (((0, 0), pevery), (SELECTED, ptenth)))
    del pos, nrm
    say("  check: both plane records equal gs_pair_plane_moments_host's on the exported positions and the planes read back: %s" % ("yes" if psame else "NO"))
    say("  check: both records equal gs_pair_moments_host's on the exported positions and the plane read back, hi and lo of every sum: %s"
        % ("yes" if same else "NO"))
    say("host end to end around each call (it returns when the device is done): median / min / max of %d calls after 3 warm-ups, us" % reps)
    for label, fn in calls:
        say("  " + label + "  " + fmt % timed(fn))
    # a whole step: the selection onto the rest.  Every step moves the selection by its fit, so the repeats are the steps of one ICP.
    step_radius = radius
    ts = []
    first = None
    for k in range(8):
        t0 = time.perf_counter()
        f = register.step(r, step_radius, SELECTED, REST)
        ts.append((time.perf_counter() - t0) * 1e6)
        first = first or f
    ts = sorted(ts[1:])
    say("  register.step (search + pair moments + fit + transform)     " + fmt % (ts[len(ts) // 2], ts[0], ts[-1]) + "   (7 steps after 1)")
    say("    the first step: %d queries among %d sources, %d candidates, %d paired, rms %.4g" %
        (first["search"]["queried"], first["search"]["sources"], first["search"]["candidates"], first["paired"], first["rms"]))

    # a whole plane step likewise: the normals of the rest, once, then the steps of one point-to-plane ICP
    surface.estimate(r, 3.0 * radius, source=REST, query=REST)
    ts, first = [], None
    for k in range(8):
        t0 = time.perf_counter()
        f = register.plane_step(r, step_radius, SELECTED, REST, damping=1e-6)
        ts.append((time.perf_counter() - t0) * 1e6)
        first = first or f
    ts = sorted(ts[1:])
    say("  register.plane_step (search + centroid + plane moments + fit + transform) " + fmt % (ts[len(ts) // 2], ts[0], ts[-1]) + "   (7 steps after 1)")
    say("    the first step: %d paired, rms %.4g, rms_plane %.4g, predicted %.4g" % (first["paired"], first["rms"], first["rms_plane"], first["predicted"]))

    def old_route():  # the same step through the host
        t0 = time.perf_counter()
        rec = r.export_splats()
        st = r.read_state()
        t1 = time.perf_counter()
        mov = (st & 2) != 0
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            cKDTree = None
        pairs = None
        if cKDTree is not None:
            fixed = np.flatnonzero(~mov)
            d, j = cKDTree(rec[fixed, 0:3]).query(rec[mov, 0:3], k=1, distance_upper_bound=step_radius)
            ok = np.isfinite(d)
            p, q = rec[mov, 0:3][ok].astype(np.float64), rec[fixed[j[ok]], 0:3].astype(np.float64)
            pm, qm = p.mean(axis=0), q.mean(axis=0)
            U, D, Vt = np.linalg.svd((p - pm).T @ (q - qm))
            d3 = np.sign(np.linalg.det(Vt.T @ U.T))
            R = Vt.T @ np.diag([1.0, 1.0, d3]) @ U.T
            rec[mov, 0:3] = ((rec[mov, 0:3].astype(np.float64) - pm) @ R.T + qm).astype(np.float32)  # (positions only: no SH rotation)
            pairs = int(ok.sum())
        t2 = time.perf_counter()
        _abi.check(r._L.gs_upload_splats(r._ctx, rec.ctypes.data, n))
        r.write_state(st)
        t3 = time.perf_counter()
        return (t1 - t0, t2 - t1, t3 - t2), pairs
    (t_exp, t_host, t_up), pairs = old_route()
    say("  the route before, once: export_splats + read_state %.2f s, %s %.2f s, upload + write_state %.2f s: %.2f s in all (%.2f GB each way)"
        % (t_exp, "k-d tree + numpy Kabsch (%d pairs)" % pairs if pairs is not None else "no host k-d tree installed:", t_host, t_up,
           t_exp + t_host + t_up, n * 320 / 1e9))
    r.destroy()
    # align under both metrics from one displaced start: the selection IS part of the cloud it is aligned to, so the truth is where it was
    say("register.align(radius=%.4g, max_iters=20, tol=1e-3) under both metrics: the selection turned by 0.1 degrees about its centroid and shifted by 0.3 of the radius" % radius)
    for metric in ("point", "plane"):
        q = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, pg, TS, flags=_abi.GS_FLAG_SPLAT_STATE)
        q.write_state(plane)
        truth = q.export_splats(2, 2)[:, 0:3].astype(np.float64)
        c = moments.centroid(q, SELECTED)
        h = np.radians(0.05)
        q.transform(_abi.compose_xform(rot=(np.cos(h), 0.3 * np.sin(h), -0.5 * np.sin(h), 0.81 * np.sin(h)), translate=(0.2 * radius, -0.2 * radius, 0.1 * radius), pivot=c))
        err = lambda: float(np.sqrt(((q.export_splats(2, 2)[:, 0:3].astype(np.float64) - truth) ** 2).sum(axis=1).mean()))  # noqa: E731
        e0 = err()
        t0 = time.perf_counter()
        steps = register.align(q, radius, max_iters=20, tol=1e-3, metric=metric, damping=1e-6, normal_radius=3.0 * radius)
        dt = time.perf_counter() - t0
        last = steps[-1] if steps else None
        say("  metric=%-5s: %2d steps in %.1f ms; displacement rms %.4g -> %.4g; last step: %d paired, rms %.4g%s" %
            (metric, len(steps), dt * 1e3, e0, err(), last["paired"] if last else 0, last["rms"] if last else float("nan"),
             ", rms_plane %.4g" % last["rms_plane"] if last and metric == "plane" else ""))
        q.destroy()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
