#!/usr/bin/env python3
"""GPU box: what the splat edits cost at config B (6.1 M splats, half of them hidden), one GPU, one process.

  python tools/export_bench.py [--n N] [--out FILE]

Host end-to-end times (the calls return when the device is done) of
  list_state                      gs_state_list of the visible half
  export_splats(device=True)      gs_export_splats_device of the visible half, beside a device-to-device copy of the same
                                  output bytes (torch .copy_, i.e. hipMemcpy DtoD)
  compact                         gs_compact(HIDDEN, 0), beside the only way to reach the same context state without it:
                                  gs_upload_splats of the host-filtered records + gs_state_write (the host-side filter itself,
                                  a numpy gather of 1 GB, is timed separately: a host that streamed its scene in has no
                                  records to filter)
  save_ply                        gs_export_ply of the visible half to a temporary file

No time is asserted anywhere; the numbers go to profiles/export_ops.txt with the box they were measured on.
"""
import argparse
import os
import sys
import tempfile
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
    HID = _abi.GS_SPLAT_HIDDEN
    plane = np.where(np.random.default_rng(5).integers(0, 2, n) == 1, HID, 0).astype(np.uint8)  # half the splats, scattered
    keep = np.flatnonzero(plane == 0)
    m = keep.size

    def mk():
        r = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, pg, TS, flags=_abi.GS_FLAG_SPLAT_STATE)
        r.write_state(plane)
        return r

    def timed(fn, reps=10):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    say("%s, N = %d, %d hidden, %d kept; host end to end, median / min / max (us)" % (torch.cuda.get_device_name(0), n, n - m, m))
    r = mk()
    say("  list_state(HIDDEN, 0)            %d ids                  %10.1f / %10.1f / %10.1f" % ((m,) + timed(lambda: r.list_state(HID, 0))))
    say("  state_count(HIDDEN, 0)           (one pass, no list)        %10.1f / %10.1f / %10.1f" % timed(lambda: r.state_count(HID, 0)))
    L = _abi.load()
    import ctypes
    dst = torch.empty((m, 80), dtype=torch.float32, device="cuda")
    src = torch.empty_like(dst)
    cnt = ctypes.c_uint64()
    torch.cuda.synchronize()

    def export_dev():
        _abi.check(L.gs_export_splats_device(r._ctx, HID, 0, dst.data_ptr(), m, ctypes.byref(cnt), None))

    def copy_dd():
        dst.copy_(src)
        torch.cuda.synchronize()

    te, tc = timed(export_dev), timed(copy_dd)
    say("  export_splats_device(HIDDEN, 0)  %.2f GB out (244 B in, 320 B out per splat)  %10.1f / %10.1f / %10.1f" % ((dst.nbytes / 1e9,) + te))
    say("  device-to-device copy of the same %.2f GB                                       %10.1f / %10.1f / %10.1f" % ((dst.nbytes / 1e9,) + tc))
    say("    export / copy = %.2f; the export moves %.0f GB/s of read + written bytes" % (te[0] / tc[0], m * 564 / te[0] / 1e3))

    def export_all():
        _abi.check(L.gs_export_splats_device(r._ctx, 0, 0, big.data_ptr(), n, ctypes.byref(cnt), None))

    del src
    big = torch.empty((n, 80), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    say("  export_splats_device(0, 0)       every splat, no selection launches            %10.1f / %10.1f / %10.1f" % timed(export_all))
    del big, dst
    torch.cuda.empty_cache()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "half.ply")
        t0 = time.perf_counter()
        wrote = r.save_ply(path, HID, 0)
        dt = time.perf_counter() - t0
        say("  save_ply(HIDDEN, 0)              %d records, %.2f GB file: %.1f ms (%.2f GB/s; the file system decides)"
            % (wrote, os.path.getsize(path) / 1e9, dt * 1e3, os.path.getsize(path) / dt / 1e9))
    # compaction against the filtered upload
    tcs = []
    for _ in range(3):
        t0 = time.perf_counter()
        ids = r.compact(HID, 0)
        tcs.append((time.perf_counter() - t0) * 1e3)
        assert ids.size == m
        r.destroy()
        r = mk()
    say("  compact(HIDDEN, 0)               %d -> %d splats: %s ms" % (n, m, " / ".join("%.1f" % t for t in tcs)))
    host = sp.cpu().numpy()
    t0 = time.perf_counter()
    filtered = np.ascontiguousarray(host[keep])
    tf = (time.perf_counter() - t0) * 1e3
    st = np.ascontiguousarray(plane[keep])
    tus = []
    for _ in range(3):
        t0 = time.perf_counter()
        _abi.check(L.gs_upload_splats(r._ctx, filtered.ctypes.data, m))
        _abi.check(L.gs_state_write(r._ctx, st.ctypes.data, m))
        tus.append((time.perf_counter() - t0) * 1e3)
    say("  gs_upload_splats of the %.2f GB of host-filtered records + gs_state_write: %s ms (+ %.1f ms for the host's numpy filter)"
        % (filtered.nbytes / 1e9, " / ".join("%.1f" % t for t in tus), tf))
    say("    compact is %.1fx the filtered upload's speed, and needs no host copy of the scene" % (min(tus) / min(tcs)))
    r.destroy()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
