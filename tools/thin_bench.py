#!/usr/bin/env python3
"""GPU box: what a thinning sample costs at config B size (6.1 M synthetic splats, a state plane), beside the neighbour count over the
same candidates, beside `gsplat.simplify` to the same counts, and beside the host route it replaces.

  python tools/thin_bench.py [--out profiles/thin.txt] [--n N] [--reps 5] [--mean 10] [--no-host] [--no-frames]

A radius with a mean neighbour count of about `--mean` is found by bisection, as tools/neigh_bench.py does; the second radius is 3 x
it.  At each radius, in ONE run:

  gs_neigh_count (limit 2^32-1) -- the yardstick: its build, and its query pass over the same candidates;
  gs_thin_sample in the hash order: the whole call, the build (the same call refused by max_candidates = 1), and every ROUND -- the
  call capped at k rounds is refused after exactly k of them, so round k costs t(k) - t(k - 1); what remains of the whole call after
  the last round is the assign pass, the commit and their read-back;
  the same with an opacity priority, and in index order (its rounds only, or the default cap's refusal);
  gs_state_thin (the kept ones) beside gs_state_neigh.

Then the rounds the hash order needs over seeds 0..4 (what GS_THIN_DEFAULT_ROUNDS is set from), `decimate` to about 1/2, 1/4 and 1/10
of the splats with an opacity and a coverage priority beside `simplify` to the same counts with the benchmark view's PSNR against the
undecimated frame, and once the route there was before: export_splats + scipy.spatial.cKDTree + a sequential greedy + state_ids.
Every device call is timed on the host around the call (it returns when the device is done): 1 warm-up, then the median / min / max.
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
RESOURCES = ("gs_thin_round_kernel: 31 VGPRs, 106 SGPRs, 7 waves per SIMD, no LDS, no scratch (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)",
             "gs_thin_assign_kernel: 36 VGPRs, 102 SGPRs, 7 waves per SIMD, no LDS, no scratch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mean", type=float, default=10.0)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (export + k-d tree + greedy + state_ids)")
    ap.add_argument("--no-frames", action="store_true", help="skip decimate / simplify and their frames")
    a = ap.parse_args()
    import numpy as np
    import torch
    import gsplat
    from gsplat import _abi, attributes, neighbours, simplify, synth, thin
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
    NONE = neighbours.LIMIT_NONE
    logit = attributes.attr(_abi.GS_ATTR_OPACITY_LOGIT)
    cover = attributes.attr(_abi.GS_ATTR_COVER_SUM)

    def timed(fn, k=reps, warm=1):
        for _ in range(warm):
            fn()
        t = []
        for _ in range(k):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    def refused(fn):
        try:
            fn()
        except _abi.GsError as e:
            assert e.code == _abi.GS_ERR_CAPACITY
            return
        raise AssertionError("the call was not refused")

    lo, hi, radius = 1e-3, 2.0, None
    for _ in range(14):
        mid = math.sqrt(lo * hi)
        try:
            neighbours.count(r, mid)
            m = float(neighbours.read(r).mean(dtype=np.float64))
        except _abi.GsError as e:
            assert e.code == _abi.GS_ERR_CAPACITY
            m = float("inf")
        if m > a.mean:
            hi = mid
        else:
            lo, radius = mid, mid
    fmt = "%9.2f / %9.2f / %9.2f"
    say("thinning (gs_thin_sample / gs_state_thin, gsplat.thin), tools/thin_bench.py")
    say("%s: N = %d synthetic splats, every splat a member" % (torch.cuda.get_device_name(0), n))
    for k in RESOURCES:
        say(k)
    say("host end to end around each call (it returns when the device is done): median / min / max of %d calls after 1 warm-up, ms" % reps)
    for rad in (radius, 3.0 * radius):
        info = neighbours.count(r, rad, NONE)
        mean = float(neighbours.read(r).mean(dtype=np.float64))
        say("radius %.6g: mean count %.2f; grid %s of edge %.6g; candidates %d (%.1f per member)"
            % (rad, mean, "x".join(str(v) for v in info["cells"]), info["cell_edge"], info["candidates"], info["candidates"] / n))
        cbuild = timed(lambda: refused(lambda: neighbours.count(r, rad, max_candidates=1)))
        cfull = timed(lambda: neighbours.count(r, rad, NONE))
        cq = cfull[0] - cbuild[0]
        say("  gs_neigh_count: build                     " + fmt % cbuild)
        say("  gs_neigh_count, limit 2^32-1              " + fmt % cfull + "   query pass = %.2f ms: %.3g candidates / s" % (cq, info["candidates"] / (cq * 1e-3)))
        for name, kw in (("hash order", {}), ("hash order, OPACITY_LOGIT priority", dict(priority=logit))):
            ti = thin.sample(r, rad, **kw)
            assert ti["candidates"] == info["candidates"]
            build = timed(lambda: refused(lambda: thin.sample(r, rad, max_candidates=1, **kw)))
            full = timed(lambda: thin.sample(r, rad, **kw))
            say("  gs_thin_sample, %s: %d kept of %d (1/%.2f), largest covers %d, %d rounds" % (name, ti["kept"], ti["members"], ti["members"] / ti["kept"],
                                                                                                 ti["largest"], ti["rounds"]))
            say("    build (+ rank, init)                    " + fmt % build)
            say("    the whole call                          " + fmt % full)
            prev, per = build[0], []
            for k in range(1, ti["rounds"]):
                t = timed(lambda: refused(lambda: thin.sample(r, rad, max_rounds=k, **kw)), 3, 0)[0]
                per.append(t - prev)
                prev = t
            if ti["rounds"] > 1:
                say("    rounds 1 .. %d, ms each (capped calls' differences; the first includes rank and init): %s" % (ti["rounds"] - 1, " ".join("%.2f" % v for v in per)))
                say("    first round = %.2f x the count's query pass; the last round, assign, commit and read-back together %.2f ms" % (per[0] / cq, full[0] - prev))
        try:  # (the index order of this scene is not a spatial order: it may well fit the default cap)
            say("  index order: %d rounds" % thin.sample(r, rad, order="index")["rounds"])
        except _abi.GsError as e:
            assert e.code == _abi.GS_ERR_CAPACITY
            say("  index order: refused by the default cap of %d rounds, as the header says it may be" % _abi.GS_THIN_DEFAULT_ROUNDS)
        thin.sample(r, rad)
        sel = timed(lambda: thin.select_kept(r, op=_abi.GS_STATE_TOGGLE), 21)
        say("  gs_state_thin (kept), 5 B per splat        " + fmt % sel)
        neighbours.count(r, rad, NONE)
        sel = timed(lambda: neighbours.select(r, 1, NONE, op=_abi.GS_STATE_TOGGLE), 21)
        say("  gs_state_neigh, 5 B per splat              " + fmt % sel)
    rounds = []
    for rad in (radius, 3.0 * radius):
        rounds.append([thin.sample(r, rad, seed=s)["rounds"] for s in range(5)])
    say("rounds of the hash order, seeds 0..4: %s at radius %.6g, %s at %.6g; the most %d -> GS_THIN_DEFAULT_ROUNDS = %d is %.1f x it"
        % (rounds[0], radius, rounds[1], 3.0 * radius, max(map(max, rounds)), _abi.GS_THIN_DEFAULT_ROUNDS, _abi.GS_THIN_DEFAULT_ROUNDS / max(map(max, rounds))))
    if not a.no_frames:
        u = synth.orbit_camera(3, W, H).uniforms(W, H)
        r.render_uniforms(u)
        r.wait()
        ref = r.read_rgba8()[..., :3].astype(np.float64)

        def psnr(rr):
            rr.render_uniforms(u)
            rr.wait()
            mse = float(((rr.read_rgba8()[..., :3].astype(np.float64) - ref) ** 2).mean())
            return 10.0 * math.log10(255.0 ** 2 / mse) if mse else float("inf")

        say("decimate beside simplify, each once on a context of its own; the benchmark view (orbit camera 3) against the undecimated frame")
        say("(the synthetic scene says little about a capture: its splats are not a surface sampled redundantly)")
        for factor in (2, 4, 10):
            for name, prio in (("OPACITY_LOGIT", logit), ("COVER_SUM after 4 views", cover)):
                r2 = renderer()
                if prio is cover:
                    for v in range(4):
                        r2.render_uniforms(synth.orbit_camera(v, W, H).uniforms(W, H))
                        r2.wait()
                        r2.accumulate_coverage()
                t0 = time.perf_counter()
                out = thin.decimate_to(r2, n // factor, priority=prio)
                t1 = time.perf_counter()
                say("  decimate_to(N / %-2d), %-24s %8d -> %8d splats at radius %-9.4g %2d probes %9.2f ms   PSNR %6.2f dB"
                    % (factor, name + ":", n, r2.numGaussians, out["radius"] or 0.0, out["probes"], (t1 - t0) * 1e3, psnr(r2)))
                r2.destroy()
            r2 = renderer()
            t0 = time.perf_counter()
            out = simplify.simplify_to(r2, n // factor)
            t1 = time.perf_counter()
            say("  simplify_to(N / %-2d):                          %8d -> %8d splats at edge %-11.4g %2d probes %9.2f ms   PSNR %6.2f dB"
                % (factor, n, r2.numGaussians, out["edge"] or 0.0, out["probes"], (t1 - t0) * 1e3, psnr(r2)))
            r2.destroy()
    if not a.no_host:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            cKDTree = None
        ti = thin.sample(r, radius)
        dev = timed(lambda: thin.sample(r, radius), 3, 0)[0] + timed(lambda: thin.select_kept(r), 3, 0)[0]
        t0 = time.perf_counter()
        rec = r.export_splats()
        t1 = time.perf_counter()
        if cKDTree is not None:
            pos = np.ascontiguousarray(rec[:, 0:3], dtype=np.float64)
            tree = cKDTree(pos)
            t2 = time.perf_counter()
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import thin_restate as tr
            order = np.argsort(tr.hash32_array(np.arange(n)).astype(np.int64) * -1, kind="stable")
            state = np.zeros(n, np.uint8)  # 0 undecided, 1 kept, 2 dropped
            nb = tree.query_ball_point(pos, radius, workers=min(16, os.cpu_count() or 1))
            t3 = time.perf_counter()
            for i in order:
                if not state[i]:
                    state[i] = 1
                    for j in nb[i]:
                        if not state[j]:
                            state[j] = 2
            t4 = time.perf_counter()
            ids = np.flatnonzero(state == 1).astype(np.uint32)
            r.state_ids(ids, _abi.GS_STATE_SET, _abi.GS_SPLAT_SELECTED)
            t5 = time.perf_counter()
            say("the route there was before, once, at radius %.6g, s: export_splats (%.2f GB) %.2f + cKDTree build %.2f + query_ball_point %.2f + sequential greedy "
                "%.2f + state_ids of %d kept %.2f = %.2f   (f64 distances: %d kept against the device's %d)"
                % (radius, rec.nbytes / 1e9, t1 - t0, t2 - t1, t3 - t2, t4 - t3, ids.size, t5 - t4, t5 - t0, ids.size, ti["kept"]))
            say("  against gs_thin_sample + gs_state_thin, %.4f s: %.0f x" % (dev * 1e-3, (t5 - t0) / (dev * 1e-3)))
        else:
            say("scipy is not installed: no k-d tree; export_splats took %.2f s" % (t1 - t0))
    r.destroy()


if __name__ == "__main__":
    main()
