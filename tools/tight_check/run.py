#!/usr/bin/env python3
"""CPU-only logic check of the tight binning (gs_tight.h) against the oracle's exact contribution masks.
Usage: python tools/tight_check/run.py [dump] [n] [W] [H] [ts] [camera step] [scale_modifier]
As a module: check(splats, uniforms, W, H, ts, header=None) -> the counts host_check prints (see check);
dump(splats, uniforms, W, H, ts, cols=None) -> every row-item slot the tight projection hands the row pipeline (see dump)."""
import hashlib, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-wgpu_amd")); sys.path.insert(0, ROOT)
import numpy as np
HEADER = os.path.join(ROOT, "gaussian-splatting-wgpu_amd", "csrc", "gs_tight.h")
_TMP, _EXE = [], {}
_LINE = re.compile(r"reference instances (\d+) .*\(tight total (\d+)\).*dropped-but-contributing (\d+) \| mask misses (\d+) \| contributing (\d+) \| kept (\d+)")


def header_text():
    """The committed gs_tight.h."""
    return open(HEADER).read()


def _tmp():
    if not _TMP:
        _TMP.append(tempfile.mkdtemp())
    return _TMP[0]


def build(header=None):
    """host_check.cpp compiled against `header` (the text of a gs_tight.h; None: the committed one), once per text and process."""
    src = (header_text() if header is None else header).replace('#include "gs_device.h"', "")
    h = hashlib.sha256(src.encode()).hexdigest()[:16]
    if h not in _EXE:
        d = os.path.join(_tmp(), h)
        os.makedirs(d, exist_ok=True)
        open(os.path.join(d, "gs_tight_host.h"), "w").write(src)
        exe = os.path.join(d, "check")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", d, os.path.join(ROOT, "tools", "tight_check", "host_check.cpp"), "-o", exe])
        _EXE[h] = exe
    return _EXE[h]


def check(splats, uniforms, W, H, ts, header=None):
    """Runs the host emulation of `header` on one frame's reference lists.  Returns a dict: ref (the reference's instances),
    contributing (those with a non-zero exact mask), kept (those the tight binning keeps), tight_total (what tight_slot_item
    emits), dropped (contributing but not kept), misses (kept with a contributing sub-block outside their mask), ratio (kept /
    contributing), returncode and stdout of host_check."""
    from oracle import gs_oracle as o
    exe = build(header)
    gd, cnt = o.preprocess(splats, uniforms, W, H, ts)
    off, I = o.scan(cnt)
    k, v = o.emit(gd, off, cnt, I, W, ts)
    sk, sv = o.sort(k, v)
    m = o.instance_masks(gd, sk, sv, W, H, ts)
    d = tempfile.mkdtemp(dir=_tmp())
    for name, a in (("gd", gd), ("sk", sk), ("sv", sv), ("m", m)):
        a.astype(np.uint32).tofile(os.path.join(d, name + ".bin"))
    out = subprocess.run([exe] + [os.path.join(d, x + ".bin") for x in ("gd", "sk", "sv", "m")] + [str(W), str(H), str(ts)],
                         capture_output=True, text=True)
    for x in ("gd", "sk", "sv", "m"):
        os.remove(os.path.join(d, x + ".bin"))
    os.rmdir(d)
    f = _LINE.search(out.stdout)
    if not f:
        raise RuntimeError("host_check said nothing to parse: %s %s" % (out.stdout[-500:], out.stderr[-500:]))
    ref, total, dropped, misses, contributing, kept = (int(x) for x in f.groups())
    return {"ref": ref, "contributing": contributing, "kept": kept, "tight_total": total, "dropped": dropped, "misses": misses,
            "ratio": kept / max(contributing, 1), "returncode": out.returncode, "stdout": out.stdout}


def dump(splats, uniforms, W, H, ts, cols=None, header=None):
    """host_check's second mode on one frame (cols: a tile-column slab, None: the whole canvas): every row-item slot the tight
    projection hands the row pipeline, as a uint32 [slots, 5] array of (gaussian index, slot number, tile row, first tile column,
    tiles; tiles == 0: a hole), gaussians in index order, and the depth bucket of every gaussian (uint32 [n]; the oracle's key
    % 1000 where the gaussian has an instance, else 0)."""
    from oracle import gs_oracle as o
    exe = build(header)
    gd, cnt = o.preprocess(splats, uniforms, W, H, ts, cols)
    off, I = o.scan(cnt)
    k, v = o.emit(gd, off, cnt, I, W, ts, cols)
    bucket = np.zeros(gd.shape[0], np.uint32)
    bucket[v] = k % 1000
    c0, c1 = cols if cols is not None else (0, o.num_tiles(W, H, ts)[0])
    with tempfile.TemporaryDirectory(dir=_tmp()) as d:
        names = [os.path.join(d, x + ".bin") for x in ("gd", "cnt", "out")]
        gd.astype(np.uint32).tofile(names[0])
        cnt.astype(np.uint32).tofile(names[1])
        out = subprocess.run([exe, "dump", names[0], names[1], str(W), str(H), str(ts), str(c0), str(c1), names[2]], capture_output=True, text=True)
        if out.returncode:
            raise RuntimeError("host_check dump failed (%d): %s" % (out.returncode, out.stderr[-500:]))
        slots = np.fromfile(names[2], np.uint32).reshape(-1, 5)
    return slots, bucket


def bicycle_case(n, W, H, ts, step, mod=1.0):
    """(splats, uniforms) of the command line's scene: synth.bicycle_like from the orbit camera's step."""
    from gsplat import synth
    s = synth.bicycle_like(n, synth.BASE_SEED + 1)
    u = synth.orbit_camera(step, W, H).uniforms(W, H).copy()
    u[39] = np.float32(mod)
    return s, u


def main(argv):
    if len(argv) > 1 and argv[1] == "dump":  # the slots of the same scene: their number, the items and the instances among them
        argv = argv[:1] + argv[2:]
        n, W, H, ts, step = (int(x) for x in (argv[1:6] + ["200000", "1920", "1080", "16", "0"][len(argv) - 1:]))
        s, u = bicycle_case(n, W, H, ts, step, float(argv[6]) if len(argv) > 6 else 1.0)
        slots, _ = dump(s, u, W, H, ts)
        print("slots %d | items %d | instances %d | gaussians with slots %d" % (slots.shape[0], int((slots[:, 4] > 0).sum()), int(slots[:, 4].sum()),
                                                                             np.unique(slots[:, 0]).size))
        return 0
    n, W, H, ts, step = (int(x) for x in (argv[1:6] + ["200000", "1920", "1080", "16", "0"][len(argv) - 1:]))
    mod = float(argv[6]) if len(argv) > 6 else 1.0
    s, u = bicycle_case(n, W, H, ts, step, mod)
    res = check(s, u, W, H, ts)
    sys.stdout.write(res["stdout"])
    return res["returncode"]


if __name__ == "__main__":
    sys.exit(main(sys.argv))
