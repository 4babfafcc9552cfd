#!/usr/bin/env python3
"""GPU box: what the packed scenes cost at config B (6.1 M resident splats), one GPU, one process.  Run it under a time limit:

  timeout 900 python tools/packed_bench.py [--n N] [--reps K] [--dir DIR] [--no-psnr] [--out FILE]

Host end-to-end times (every call returns when the device is done and the file is closed; the files go to --dir, the system's
temporary directory by default, and are read back from the page cache) of
  * gs_export_packed per order (index, morton) and per SH degree (0..3), beside gs_export_ply at degree 3 in the same run,
  * gs_upload_packed of the degree-3 and degree-0 Morton files, beside gs_upload_ply of the .ply, each into a context of its own,
the sizes of the files, and the PSNR (over the rgba8 image's three colour channels) of a config-B frame of the re-loaded packed scene
against the original scene's frame, per order and degree: Morton chunks have tighter bounds, so their positions are finer.  The PSNR
describes the FORMAT, not the code: the codec is held to its definition bit for bit by tests/test_packed.py.

The kernels' own times come from a trace of their own: `rocprofv3 --kernel-trace --stats -- python tools/packed_bench.py --reps 2
--no-psnr`; the encode kernel reads 60 B and writes 16.3 B per splat, the SH kernel reads 4 x 3K B and writes 3K B.

--oracle needs no GPU: the smoke scene (20 000 splats, 320 x 192) through the HOST codec and the CPU oracle's renderer, in index and
in Morton order (tests/pack_restate.py's), all fields and one field at a time -- what the format costs where a frame is not noise.

No time is asserted anywhere; the numbers go to profiles/packed.txt with the box they were measured on.
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


def oracle_psnr(say):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pack_restate as pr
    from gsplat import packed, synth
    from oracle import gs_oracle
    gs_oracle.build()
    n, w, h = 20000, 320, 192
    s = synth.bicycle_like(n)
    u = synth.orbit_camera(5, w, h).uniforms(w, h)
    ref = gs_oracle.render(s, u, w, h, 16)["rgba8"][..., :3].astype(np.float64)

    def psnr(rec):
        mse = float(((gs_oracle.render(np.ascontiguousarray(rec), u, w, h, 16)["rgba8"][..., :3].astype(np.float64) - ref) ** 2).mean())
        return "identical" if mse == 0.0 else "%.2f dB" % (10 * np.log10(255.0 ** 2 / mse))
    order = pr.morton_order(s[:, :3])
    parts = (("position", [0, 1, 2]), ("log-scale", [4, 5, 6]), ("rotation", [8, 9, 10, 11]), ("opacity", [12]), ("band 0", [16, 17, 18]),
             ("SH rest", [16 + 4 * k + c for k in range(1, 16) for c in range(3)]))
    say("CPU oracle, %d splats, %d x %d, orbit camera 5, degree 3: PSNR against the original's frame" % (n, w, h))
    say("  %-34s %s" % ("original records in Morton order", psnr(s[order])))
    for name, rec in (("index", s), ("morton", s[order])):
        dec = packed.decode(*packed.encode(rec, 3)[:3], 3)
        say("  %-34s %s" % ("packed %s, every field" % name, psnr(dec)))
        for pname, cols in parts:
            x = np.array(rec, copy=True)
            x[:, cols] = dec[:, cols]
            say("  %-34s %s" % ("packed %s, %s only" % (name, pname), psnr(x)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--oracle", action="store_true", help="no GPU: the small-scene PSNR table through the CPU oracle, nothing else")
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", help="where the files go (default: a fresh temporary directory)")
    ap.add_argument("--no-psnr", action="store_true")
    ap.add_argument("--out", help="also append the report to this file")
    a = ap.parse_args()
    if a.oracle:
        lines = []
        oracle_psnr(lambda s: (print(s, flush=True), lines.append(s)))
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import gsplat
    from gsplat import _abi, packed, synth
    n = a.n
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sp = synth.bicycle_like_torch(n, synth.BASE_SEED + 1, "cuda")
    torch.cuda.synchronize()
    pg = gsplat.PackedGaussians.__new__(gsplat.PackedGaussians)
    pg.numGaussians, pg.gaussiansBuffer, pg.sphericalHarmonicsDegree = n, sp, 3
    r = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, pg, TS)
    del pg, sp
    one = gsplat.PackedGaussians(np.zeros((1, 80), np.float32))
    r2 = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, one, TS)
    L = _abi.load()
    tmp = a.dir or tempfile.mkdtemp(prefix="packed_bench_")
    cnt = ctypes.c_uint64()
    u = synth.orbit_camera(5, W, H).uniforms(W, H)

    def timed(fn):
        t = []
        for k in range(a.reps + 1):  # one warm-up call
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if k >= 1:
                t.append((t1 - t0) * 1e3)
        t.sort()
        return t[len(t) // 2], t[0], t[-1]

    def frame(x):
        x.render_uniforms(u)
        x.wait()
        return x.read_rgba8()[..., :3].astype(np.float64)

    say("%s, N = %d resident splats, files in %s" % (torch.cuda.get_device_name(0), n, tmp))
    say("host end to end, %d repeats after 1 warm-up call: median / min / max (ms); MB of file; GB/s of file at the median" % a.reps)
    ply = os.path.join(tmp, "scene.ply")
    t = timed(lambda: _abi.check(L.gs_export_ply(r._ctx, ply.encode(), 0, 0, 3, ctypes.byref(cnt))))
    size = os.path.getsize(ply)
    say("  %-34s %9.1f / %9.1f / %9.1f   %8.1f MB  %6.2f GB/s" % ("gs_export_ply degree 3", t[0], t[1], t[2], size / 1e6, size / t[0] / 1e6))
    files = {}
    for order in ("index", "morton"):
        for degree in (0, 1, 2, 3):
            path = os.path.join(tmp, "scene_%s_%d.packed.ply" % (order, degree))
            info = {}
            t = timed(lambda: info.update(packed.save(r, path, 0, 0, degree, order)))
            files[(order, degree)] = path
            say("  %-34s %9.1f / %9.1f / %9.1f   %8.1f MB  %6.2f GB/s   nonfinite %d"
                % ("gs_export_packed %s degree %d" % (order, degree), t[0], t[1], t[2], info["file_bytes"] / 1e6, info["file_bytes"] / t[0] / 1e6,
                   info["nonfinite"]))
    t = timed(lambda: _abi.check(L.gs_upload_ply(r2._ctx, ply.encode(), ctypes.byref(cnt))))
    say("  %-34s %9.1f / %9.1f / %9.1f   %8.1f MB  %6.2f GB/s" % ("gs_upload_ply degree 3", t[0], t[1], t[2], size / 1e6, size / t[0] / 1e6))
    for degree in (3, 0):
        path = files[("morton", degree)]
        t = timed(lambda: packed.upload(r2, path))
        sz = os.path.getsize(path)
        say("  %-34s %9.1f / %9.1f / %9.1f   %8.1f MB  %6.2f GB/s" % ("gs_upload_packed morton degree %d" % degree, t[0], t[1], t[2], sz / 1e6, sz / t[0] / 1e6))
    if not a.no_psnr:
        ref = frame(r)
        say("PSNR of the frame (orbit camera 5, %d x %d, rgb of the rgba8 image) of the re-loaded scene against the original's:" % (W, H))
        packed.upload(r2, files[("morton", 3)])  # (any file: the .ply round trip below is the yardstick, exact)
        _abi.check(L.gs_upload_ply(r2._ctx, ply.encode(), ctypes.byref(cnt)))
        mse = float(((frame(r2) - ref) ** 2).mean())
        say("  %-34s %s" % (".ply degree 3", "identical" if mse == 0.0 else "%.2f dB" % (10 * np.log10(255.0 ** 2 / mse))))
        # the order alone: the original records, unquantised, uploaded in the Morton order (the frame's sort is by depth bucket, then
        # by index: a permutation changes which of two splats of one bucket is blended first)
        _, ids = packed.save(r, files[("morton", 0)], 0, 0, 0, "morton", with_ids=True)
        rec = r.export_splats(device=True)[torch.from_numpy(ids.astype(np.int64)).cuda()].contiguous()
        torch.cuda.synchronize()
        _abi.check(L.gs_upload_splats_device(r2._ctx, rec.data_ptr(), n))
        mse = float(((frame(r2) - ref) ** 2).mean())
        say("  %-34s %s   (%d intersections)" % ("original records in Morton order", "identical" if mse == 0.0 else "%.2f dB" % (10 * np.log10(255.0 ** 2 / mse)),
                                                  r2.stats()["num_intersections"]))
        del rec
        for order in ("index", "morton"):
            for degree in (0, 1, 2, 3):
                packed.upload(r2, files[(order, degree)])
                mse = float(((frame(r2) - ref) ** 2).mean())
                say("  %-34s %s   (%d intersections)" % ("packed %s degree %d" % (order, degree),
                                                          "identical" if mse == 0.0 else "%.2f dB" % (10 * np.log10(255.0 ** 2 / mse)), r2.stats()["num_intersections"]))
        # the yardstick once more, behind every other upload into the same context: still exact
        _abi.check(L.gs_upload_ply(r2._ctx, ply.encode(), ctypes.byref(cnt)))
        mse = float(((frame(r2) - ref) ** 2).mean())
        st = r2.stats()
        say("  %-34s %s   (truncated frames %d, intersections %d of capacity %d)"
            % (".ply degree 3, again", "identical" if mse == 0.0 else "%.2f dB" % (10 * np.log10(255.0 ** 2 / mse)), st["truncated_frames"],
               st["num_intersections"], st["capacity"]))
    r.destroy()
    r2.destroy()
    for p in [ply] + list(files.values()):
        os.remove(p)
    if not a.dir:
        os.rmdir(tmp)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
