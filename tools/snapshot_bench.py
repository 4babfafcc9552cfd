#!/usr/bin/env python3
"""GPU box: what snapshots and write-back cost at config B (6.1 M resident splats), one GPU, one process.  Run it under a time limit:

  timeout 600 python tools/snapshot_bench.py [--n N] [--reps K] [--out FILE]

Host end-to-end times (every call returns when the device is done) of, for each part (POSITION, GEOMETRY, SH, STATE) and for RECORD,
on a 10 % sphere selection:
  * gs_snapshot_take      (the selection over the state plane, the allocation of the snapshot, the gather; the free is not timed),
  * gs_snapshot_restore   (the scatter),
  * gs_snapshot_swap      (both ways in one pass),
  * gs_write_splats_device of the selection's own records, ids and state bytes from device tensors (the ascending-ids check, its
    read-back, the scatter).
GB is the traffic the header states, GB/s that over the median -- a rate of the CALL, not of a kernel:
  take    2 B of state per RESIDENT splat (count + scatter of the selection) + per matched splat the part's bytes read and written,
          4 B of id written by the selection, 4 + 4 B for its copy into the snapshot and 4 B read by the gather;
  restore the part's bytes read and written + 4 B of id (+ 4 B of the derived plane with GEOMETRY);
  swap    twice the part's bytes read and written + 4 B of id (+ 4 B with GEOMETRY);
  write   the 16-byte columns of the part read (16 / 48 / 256 B, RECORD 320; STATE 1 B), the part's bytes written, 4 B of id twice
          (check and scatter).
Beside them, once, the route they replace: gs_export_splats of the selection to the host and gs_upload_splats of everything from a
host array (which also drops the frame, the shadows, a captured graph and every per-splat plane).

No time is asserted anywhere; the numbers go to profiles/snapshots.txt with the box they were measured on.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", help="also append the report to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import gsplat
    from gsplat import _abi, snapshots, synth
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
    # the selection's own records, ids and state bytes on the device: what the timed write-back puts back (the scene does not change)
    rec, ids = r.export_splats(SEL, SEL, with_ids=True, device=True)
    states = torch.full((m,), SEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    written = ctypes.c_uint64()

    def timed(fn, after=None):
        t = []
        for k in range(a.reps + 2):  # two warm-up calls
            t0 = time.perf_counter()
            out = fn()
            t1 = time.perf_counter()
            if after:
                after(out)
            if k >= 2:
                t.append((t1 - t0) * 1e6)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    say("%s, N = %d resident, sphere selection %d splats (%.2f %%)" % (torch.cuda.get_device_name(0), n, m, 100.0 * m / n))
    say("host end to end, %d repeats after 2 warm-up calls: median / min / max (us); GB/s of the stated traffic at the median" % a.reps)
    P = snapshots
    cases = (("POSITION", P.POSITION, 12, 16), ("GEOMETRY", P.GEOMETRY, 32, 48), ("SH", P.SH, 192, 256), ("STATE", P.STATE, 1, 1),
             ("RECORD", P.RECORD, 236, 320))
    for name, parts, pb, cols in cases:
        smax = 4 if parts & P.GEOMETRY else 0
        keep = P.take(r, SEL, SEL, parts)
        assert keep.info()["count"] == m
        rows = (("take", lambda: P.take(r, SEL, SEL, parts), lambda s: s.free(), 2 * n + (2 * pb + 16) * m),
                ("restore", keep.restore, None, (2 * pb + 4 + smax) * m),
                ("swap", keep.swap, None, (4 * pb + 4 + smax) * m),
                ("write (device)", lambda: _abi.check(L.gs_write_splats_device(r._ctx, ids.data_ptr(), m, rec.data_ptr(), states.data_ptr(), parts,
                                                                                ctypes.byref(written))), None, (cols + pb + 8) * m))
        for what, fn, after, traffic in rows:
            t = timed(fn, after)
            say("  %-9s %-15s %8.4f GB  %9.1f / %9.1f / %9.1f   %7.1f GB/s   %d B of snapshot" %
                (name, what, traffic / 1e9, t[0], t[1], t[2], traffic / t[0] / 1e3, keep.info()["device_bytes"]))
        keep.free()
    # the route they replace, once: the selection to the host, and everything uploaded again from a host array
    everything = r.export_splats()
    t0 = time.perf_counter()
    host_sel = r.export_splats(SEL, SEL)
    t1 = time.perf_counter()
    _abi.check(L.gs_upload_splats(r._ctx, everything.ctypes.data, n))
    _abi.check(L.gs_wait(r._ctx))
    t2 = time.perf_counter()
    say("  the route they replace: gs_export_splats of the selection %.1f ms (%.3f GB to the host) + gs_upload_splats of everything %.1f ms (%.3f GB) = %.1f ms"
        % (1e3 * (t1 - t0), host_sel.nbytes / 1e9, 1e3 * (t2 - t1), everything.nbytes / 1e9, 1e3 * (t2 - t0)))
    r.destroy()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
