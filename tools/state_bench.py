#!/usr/bin/env python3
"""GPU box: what the splat-state layer costs at config B (6.1 M splats, 1080p, tile 16).

  python tools/state_bench.py                  host latencies and the projection's cost of the state byte
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/state_bench.py --kernels
                                                a run of its own: every region kind a few times, and a device copy of the same
                                                bytes beside them; kernel times are read from the trace's *_kernel_stats.csv
  python tools/state_bench.py --report DIR     13 N (+N) bytes over the kernel times of a trace under DIR, beside the copy rate

Numbers go to profiles/state_ops.txt.
"""
import argparse
import csv
import glob
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-wgpu_amd"))
sys.path.insert(0, ROOT)

N, W, H, TS = 6_100_000, 1920, 1080, 16


def report(d):
    """Kernel means of a rocprofv3 --kernel-trace --stats run: bytes over time per region kind, and the copy kernel's rate."""
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under " + d)
    rows = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            rows[r["Name"]] = (float(r["AverageNs"]), int(r["Calls"]))
    kinds = ["all", "sphere", "box", "screen_rect", "screen_mask"]
    copy = [(ns, c, k) for k, (ns, c) in rows.items() if "xor" in k.lower()]
    print("kernel means (rocprofv3 --kernel-trace --stats), N = %d" % N)
    for name, (ns, calls) in sorted(rows.items()):
        if "gs_state_region_kernel" not in name:
            continue
        k = int(re.search(r"gs_state_region_kernel<(\d)>", name).group(1))
        rd = (13 if k else 1) * N  # ALL reads the state byte only
        print("  region %-12s %8.1f us x %3d   %6.0f GB/s read (%2d N bytes), %6.0f GB/s with the N bytes written"
              % (kinds[k], ns / 1e3, calls, rd / ns, 13 if k else 1, (rd + N) / ns))
    for name, (ns, calls) in sorted(rows.items()):
        if "gs_state_count_kernel" in name or "gs_state_ids_kernel" in name:
            print("  %-19s %8.1f us x %3d" % (name.split("(")[0][:19], ns / 1e3, calls))
    for ns, calls, name in copy:
        print("  streaming copy of 13 N bytes (torch.bitwise_xor) %8.1f us x %3d   %6.0f GB/s read (+ as much written)" % (ns / 1e3, calls, 13 * N / ns))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true", help="only launch the state kernels and the copy (for a kernel trace)")
    ap.add_argument("--report", help="directory of a finished kernel trace")
    ap.add_argument("--n", type=int, default=N)
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    import numpy as np
    import torch
    import gsplat
    from gsplat import _abi, synth
    n = a.n
    sp = synth.bicycle_like_torch(n, synth.BASE_SEED + 1, "cuda")
    torch.cuda.synchronize()
    pg = gsplat.PackedGaussians.__new__(gsplat.PackedGaussians)
    pg.numGaussians, pg.gaussiansBuffer, pg.sphericalHarmonicsDegree = n, sp, 3
    u = synth.orbit_camera(0, W, H).uniforms(W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = (((xx - W / 2) ** 2 + (yy - 0.45 * H) ** 2 < (0.3 * H) ** 2) & ((xx // 8 + yy // 8) % 2 == 0)).astype(np.uint8)
    SEL, HID = _abi.GS_SPLAT_SELECTED, _abi.GS_SPLAT_HIDDEN

    def mk(flags):
        return gsplat.Renderer(gsplat.Canvas(W, H), None, 0, pg, TS, flags=flags)

    r = mk(_abi.GS_FLAG_SPLAT_STATE | _abi.GS_FLAG_TIMING)
    regions = [("all", lambda op: r.state_region(_abi.GS_REGION_ALL, op, SEL)),
               ("sphere", lambda op: r.select_sphere((0.0, 0.0, 0.0), 1.0, op)),
               ("box", lambda op: r.select_box((-1.0, -0.5, -1.0), (0.5, 1.0, 1.5), op)),
               ("screen_rect", lambda op: r.select_rect(W // 4, H // 4, 3 * W // 4, 3 * H // 4, u, op)),
               ("screen_mask", lambda op: r.select_mask(mask, u, op))]
    if a.kernels:
        src = torch.zeros((13 * n + 3) // 4, dtype=torch.int32, device="cuda")  # 13 N bytes through a plain streaming kernel
        dst = torch.empty_like(src)
        for _ in range(10):
            for _, fn in regions:
                fn(_abi.GS_STATE_TOGGLE)  # every call changes every matched byte: 13 N read, the matched bytes written
            r.state_count(SEL, SEL)
            torch.bitwise_xor(src, 1, out=dst)  # (an elementwise kernel nothing else here launches; a memcpy is no kernel of the trace)
            torch.cuda.synchronize()
        r.destroy()
        return

    def timed(fn, reps=20):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    print("config B: N = %d, %d x %d, tile %d" % (n, W, H, TS))
    print("host end-to-end latency of a state call (median / min / max of 20, us; the call returns when the device is done):")
    for name, fn in regions:
        m = fn(_abi.GS_STATE_SET)
        print("  select %-12s matched %8d   %8.1f / %8.1f / %8.1f" % ((name, m) + timed(lambda: fn(_abi.GS_STATE_TOGGLE))))
    r.clear_selection()
    r.select_rect(W // 4, H // 4, 3 * W // 4, 3 * H // 4, u)
    print("  hide_selected                          %8.1f / %8.1f / %8.1f" % timed(r.hide_selected))
    print("  state_count                            %8.1f / %8.1f / %8.1f" % timed(lambda: r.state_count(HID, HID)))
    ids = np.unique(np.random.default_rng(1).integers(0, n, 100000)).astype(np.uint32)
    print("  state_ids (%6d ids)                 %8.1f / %8.1f / %8.1f" % ((ids.size,) + timed(lambda: r.state_ids(ids, _abi.GS_STATE_TOGGLE, 0x10))))
    snap = r.read_state()
    print("  read_state                             %8.1f / %8.1f / %8.1f" % timed(r.read_state, 5))
    print("  write_state                            %8.1f / %8.1f / %8.1f" % timed(lambda: r.write_state(snap), 5))
    host = sp.cpu().numpy()
    L = _abi.load()
    t0 = time.perf_counter()
    _abi.check(L.gs_upload_splats(r._ctx, host.ctypes.data, n))
    print("  gs_upload_splats of the %.2f GB it replaces: %.1f us (zeroes the plane)" % (host.nbytes / 1e9, (time.perf_counter() - t0) * 1e6))
    del host
    # the projection with and without the state byte: an all-zero plane against a context without the flag, alternated
    p = mk(_abi.GS_FLAG_TIMING)
    cams = [synth.orbit_camera(k, W, H).uniforms(W, H) for k in range(8)]
    for x in (r, p):
        for c in cams[:3]:
            x.render_uniforms(c)
            x.wait()
    print("projection stage mean over 64 frames (us), alternated: flagged (all-zero plane) / unflagged / ratio")
    for rnd in range(4):
        out = []
        for x in (r, p, p, r)[:: 1 if rnd % 2 == 0 else -1]:
            x.set_option(_abi.GS_OPT_RESET_TIMING, 0)
            for k in range(64):
                x.render_uniforms(cams[k % 8])
                x.wait()
            out.append((x is r, x.stats()["stage_us_mean"]["preprocess"], x.stats()["frame_us_mean"]))
        fl = [v for f, v, _ in out if f]
        un = [v for f, v, _ in out if not f]
        print("  round %d: flagged %s  unflagged %s  ratio of means %.4f   (frame: %s)"
              % (rnd, ["%.1f" % v for v in fl], ["%.1f" % v for v in un], sum(fl) / sum(un), ["%.0f" % t for _, _, t in out]))
    r.destroy()
    p.destroy()


if __name__ == "__main__":
    main()
