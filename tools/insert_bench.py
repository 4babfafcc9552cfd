#!/usr/bin/env python3
"""GPU box: what the splat insertion costs at config B (6.1 M resident splats), one GPU, one process.  Run it under a time limit:

  timeout 600 python tools/insert_bench.py [--n N] [--reps K] [--pause S] [--no-settle] [--out FILE]

Host end-to-end times (every call returns when the device is done) of
  * gs_append_splats_device of 10 % more records from a device tensor,
  * gs_duplicate_splats of a 10 % sphere selection,
  * gs_append_ply of a 10 % file (written once with gs_ply_save, read from the page cache afterwards; beside it gs_upload_ply of
    the same file into a context of its own: the two calls share the streaming loop, the difference is the grow pass),
each from the same N resident splats: between two timed calls the context is brought back to N by an untimed gs_compact that drops
the new splats (they carry a state byte of their own).  Every call builds a scene of N + m splats beside the old one: the grow pass
reads and writes 245 B per RESIDENT splat, the tail 320 B read + 245 B written per record (append), 245 B each way per copy
(duplicate) or the file's vertices (ply); GB/s is that stated traffic over the median.  Two things in the same run, on the same
context:
  * the yardstick, gs_compact(0, 0): it moves the same 245 B per resident splat each way, plus an index gather that the insertion's
    prefix does not have, and re-sizes the same work arrays.  The spread of its repeats is printed: a difference inside it is none;
  * the route the calls replace, once: gs_export_splats of everything to the host, numpy concatenate, gs_upload_splats.

Before every timed call two small untimed copies are made (settle; --no-settle leaves them out) and --pause S sleeps S seconds: a
call that follows the compaction's multi-gigabyte free within milliseconds sometimes takes 45 to 75 ms longer (profiles/insert.txt).

No time is asserted anywhere; the numbers go to profiles/insert.txt with the box they were measured on.
"""
import argparse
import ctypes
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-wgpu_amd"))
sys.path.insert(0, ROOT)

N, W, H, TS = 6_100_000, 1920, 1080, 16
SCENE_BYTES = 245  # 4 plane floats, 32 B geometry, 192 B SH, the state byte
MARK = 0x80        # the state byte of the timed insertions: what the untimed compaction drops again


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pause", type=float, default=0.0, help="seconds to sleep before every timed call, after the settling copies")
    ap.add_argument("--no-settle", action="store_true", help="leave out the untimed copies before every timed call (see settle)")
    ap.add_argument("--out", help="also append the report to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import gsplat
    from gsplat import _abi, synth
    n, m = a.n, a.n // 10
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sp = synth.bicycle_like_torch(n, synth.BASE_SEED + 1, "cuda")
    tail = synth.bicycle_like_torch(m, synth.BASE_SEED + 2, "cuda").contiguous()
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
    msel = r.select_sphere(centre, radius)
    L = _abi.load()
    first, cnt = ctypes.c_uint64(), ctypes.c_uint64()
    tmp = tempfile.mkdtemp(prefix="insert_bench_")
    ply = os.path.join(tmp, "tail.ply")
    _abi.save_ply(ply, tail.cpu().numpy(), 3)
    ply_bytes = os.path.getsize(ply)

    def restore():
        _abi.check(L.gs_compact(r._ctx, MARK, 0, ctypes.byref(cnt), None))
        assert cnt.value == n

    probe = torch.zeros(4, device="cuda")
    pinned = torch.zeros(4 << 20, dtype=torch.float32).pin_memory()

    def settle():
        """Untimed, before every timed call: one small device-to-host and one 16 MB host-to-device copy.  The call before has just freed
        gigabytes of device memory; copies queued behind whatever the driver still does with it would be charged to the next call."""
        probe.cpu()
        pinned.cuda(non_blocking=True)
        torch.cuda.synchronize()
        if a.pause:
            time.sleep(a.pause)

    def timed(fn, after=None):
        t = []
        for k in range(a.reps + 2):  # two warm-up calls
            if not a.no_settle:
                settle()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if after:
                after()
            if k >= 2:
                t.append((t1 - t0) * 1e6)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    def append_device():
        _abi.check(L.gs_append_splats_device(r._ctx, tail.data_ptr(), m, MARK, ctypes.byref(first)))

    def duplicate():
        _abi.check(L.gs_duplicate_splats(r._ctx, SEL, SEL, MARK, ctypes.byref(first), ctypes.byref(cnt), None))

    def append_ply():
        _abi.check(L.gs_append_ply(r._ctx, ply.encode(), MARK, ctypes.byref(first), ctypes.byref(cnt)))

    def compact_all():
        _abi.check(L.gs_compact(r._ctx, 0, 0, ctypes.byref(cnt), None))

    # the stream alone: gs_upload_ply of the same file into a context of its own (the two calls share the streaming loop)
    r2 = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, gsplat.PackedGaussians(np.zeros((1, 80), np.float32)), TS)

    def upload_ply():
        _abi.check(L.gs_upload_ply(r2._ctx, ply.encode(), ctypes.byref(cnt)))

    say("%s, N = %d resident, m = %d appended (10 %%), sphere selection %d splats (%.2f %%), .ply %d vertices, %.1f MB"
        % (torch.cuda.get_device_name(0), n, m, msel, 100.0 * msel / n, m, ply_bytes / 1e6))
    say("host end to end, %d repeats after 2 warm-up calls%s: median / min / max (us); GB/s of the stated traffic at the median"
        % (a.reps, (", NO settling copies" if a.no_settle else "") + (", %.2f s pause before each" % a.pause if a.pause else "")))
    grow = 2 * SCENE_BYTES * n
    rows = (("gs_compact(0, 0)  [yardstick]", compact_all, None, grow + 2 * n + 8 * n),  # + the selection: 2 N B read, 4 B per id each way
            ("gs_append_splats_device 10 %", append_device, restore, grow + (320 + SCENE_BYTES) * m),
            ("gs_duplicate_splats 10 %", duplicate, restore, grow + 2 * SCENE_BYTES * msel + 2 * n + 8 * msel),
            ("gs_append_ply 10 %", append_ply, restore, grow + ply_bytes + SCENE_BYTES * m),
            ("gs_upload_ply of that file alone", upload_ply, None, ply_bytes + SCENE_BYTES * m))
    med = {}
    for name, fn, after, traffic in rows:
        t = timed(fn, after)
        med[name] = t
        say("  %-32s %8.3f GB  %10.1f / %10.1f / %10.1f   %7.1f GB/s" % (name, traffic / 1e9, t[0], t[1], t[2], traffic / t[0] / 1e3))
    y = med[rows[0][0]]
    say("  yardstick spread (max - min) / median: %.3f" % ((y[2] - y[1]) / y[0]))
    for name, _, _, _ in rows[1:4]:
        say("  %-32s / gs_compact(0, 0), medians: %.3f" % (name, med[name][0] / y[0]))
    say("  gs_append_ply - gs_upload_ply of the same file, medians: %.1f us" % (med[rows[3][0]][0] - med[rows[4][0]][0]))
    # the route the calls replace, once: everything to the host, concatenate, upload again
    host_tail = tail.cpu().numpy()
    t0 = time.perf_counter()
    rec = r.export_splats()
    t1 = time.perf_counter()
    both = np.concatenate([rec, host_tail])
    t2 = time.perf_counter()
    _abi.check(L.gs_upload_splats(r._ctx, both.ctypes.data, n + m))
    _abi.check(L.gs_wait(r._ctx))
    t3 = time.perf_counter()
    say("  the route they replace: gs_export_splats %.1f ms + numpy concatenate %.1f ms + gs_upload_splats %.1f ms = %.1f ms  (%.0f x the device append)"
        % (1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (t3 - t0), 1e6 * (t3 - t0) / med[rows[1][0]][0]))
    r.destroy()
    r2.destroy()
    os.remove(ply)
    os.rmdir(tmp)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
