#!/usr/bin/env python3
"""GPU box: what the splat-attribute calls cost at config B size (6.1 M synthetic splats, a state plane, 1080p, tile 16).

  python tools/attr_bench.py [--out profiles/attributes.txt] [--n N] [--reps 21]

Every call is timed on the host around the call (each returns when the device is done): 3 warm-ups, then the median / min / max of
`reps` calls in microseconds.  Timed: the four calls for POS_X, OPACITY_LOGIT, DC_R and COVER_SUM, dense and with a one-in-three
filter; the histogram at 256 and 1024 bins over a spread range and over a range whose first bin holds every splat; and, in the same
run, gs_state_region(BOX), gs_state_count and the route there was before -- export_splats, numpy, state_ids -- for one question.
gs_state_attr(POS_X) and the BOX pass are also timed alternately, pair by pair, because their difference is what the file records.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-wgpu_amd"))
sys.path.insert(0, ROOT)

N, W, H, TS = 6_100_000, 1920, 1080, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    import numpy as np
    import torch
    import gsplat
    from gsplat import _abi, attributes, synth
    n, reps = a.n, max(20, a.reps)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sp = synth.bicycle_like_torch(n, synth.BASE_SEED + 1, "cuda")
    torch.cuda.synchronize()
    pg = gsplat.PackedGaussians.__new__(gsplat.PackedGaussians)
    pg.numGaussians, pg.gaussiansBuffer, pg.sphericalHarmonicsDegree = n, sp, 3
    r = gsplat.Renderer(gsplat.Canvas(W, H), None, 0, pg, TS, flags=_abi.GS_FLAG_SPLAT_STATE)
    u = synth.orbit_camera(0, W, H).uniforms(W, H)
    for _ in range(2):  # (the first frame grows the capacity)
        r.render_uniforms(u)
        r.wait()
    r.accumulate_coverage()
    plane = np.zeros(n, np.uint8)
    plane[::3] = 0x04
    r.write_state(plane)
    THIRD, SEL = (0x04, 0x04), _abi.GS_SPLAT_SELECTED

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

    fmt = "%9.1f / %9.1f / %9.1f"
    say("splat attributes (gs_attr_* / gs_state_attr), tools/attr_bench.py")
    say("%s: N = %d, a state plane with one splat in three marked, coverage planes of one %d x %d frame" % (torch.cuda.get_device_name(0), n, W, H))
    say("host end to end around each call (it returns when the device is done): median / min / max of %d calls after 3 warm-ups, us" % reps)
    kinds = [("POS_X", _abi.GS_ATTR_POS_X, 4), ("OPACITY_LOGIT", _abi.GS_ATTR_OPACITY_LOGIT, 16), ("DC_R", _abi.GS_ATTR_DC_R, 12),
             ("COVER_SUM", _abi.GS_ATTR_COVER_SUM, 16)]
    ranges = {}
    for name, kind, nbytes in kinds:
        at = attributes.attr(kind)
        sm = attributes.summary(r, at)
        lo, hi = float(sm["min"]), float(np.nextafter(sm["max"], np.float32(np.inf)))
        ranges[name] = (lo, hi)
        mid = 0.5 * (lo + hi)
        say("%s (%d B per splat), values in [%g, %g]" % (name, nbytes, sm["min"], sm["max"]))
        for label, where in (("dense", (0, 0)), ("1 in 3", THIRD)):
            say("  summary        %-7s " % label + fmt % timed(lambda: attributes.summary(r, at, where)))
            say("  histogram 256  %-7s " % label + fmt % timed(lambda: attributes.histogram(r, at, lo, hi, 256, where)))
            say("  values         %-7s " % label + fmt % timed(lambda: attributes.values(r, at, where), 20)
                + "   (%d floats to the host)" % attributes.values(r, at, where).size)
            say("  select TOGGLE  %-7s " % label + fmt % timed(lambda: attributes.select(r, at, lo, mid, True, _abi.GS_STATE_TOGGLE, SEL, where)))
    say("histogram(POS_X), dense: a spread range against a range whose first bin holds every splat")
    at = attributes.attr(_abi.GS_ATTR_POS_X)
    lo, hi = ranges["POS_X"]
    wide = lo + 2048.0 * (hi - lo + 1.0)
    one = {}
    for bins in (256, 1024):
        c = attributes.histogram(r, at, lo, wide, bins)[0]
        assert int(c[0]) == n
        s_t = timed(lambda: attributes.histogram(r, at, lo, hi, bins))
        o_t = timed(lambda: attributes.histogram(r, at, lo, wide, bins))
        one[bins] = o_t[0] / s_t[0]
        say("  %4d bins  spread  " % bins + fmt % s_t)
        say("  %4d bins  one bin " % bins + fmt % o_t + "   one bin / spread = %.2f" % one[bins])
    say("for comparison, in the same run")
    box = lambda: r.state_region(_abi.GS_REGION_BOX, _abi.GS_STATE_TOGGLE, SEL, a=(-1.0, -0.5, -1.0), b=(0.5, 1.0, 1.5))
    attr_x = lambda: attributes.select(r, at, -1.0, 0.5, True, _abi.GS_STATE_TOGGLE, SEL)
    say("  gs_state_region(BOX), 13 B per splat    " + fmt % timed(box))
    say("  gs_state_attr(POS_X), 5 B per splat     " + fmt % timed(attr_x))
    say("  gs_state_count, 1 B per splat           " + fmt % timed(lambda: r.state_count(SEL, SEL)))
    tb, ta = [], []
    for fn in (box, attr_x) * 3:
        fn()
    for k in range(4 * reps):  # alternated, pair by pair, the order swapped every pair
        for fn, t in ((box, tb), (attr_x, ta))[:: 1 if k % 2 == 0 else -1]:
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
    tb.sort()
    ta.sort()
    ratio = ta[len(ta) // 2] / tb[len(tb) // 2]
    say("  alternated, %d pairs: BOX median %.1f, attr(POS_X) median %.1f us: attr / BOX = %.3f" % (len(tb), tb[len(tb) // 2], ta[len(ta) // 2], ratio))
    r.clear_selection()

    def old_route():  # "select opacity logit below 0": export, numpy, state_ids
        rec = r.export_splats()
        ids = np.flatnonzero(rec[:, 12] <= 0.0).astype(np.uint32)
        r.state_ids(ids, _abi.GS_STATE_SET, SEL)
        return ids.size
    new_route = lambda: attributes.select(r, attributes.attr(_abi.GS_ATTR_OPACITY_LOGIT), -np.inf, 0.0)
    m_old = old_route()
    m_new = new_route()
    assert m_old == m_new == r.state_count(SEL, SEL)
    old_t = timed(old_route, 5)
    new_t = timed(new_route)
    say("  one question, \"select the splats with opacity logit <= 0\" (%d of them):" % m_new)
    say("    export_splats + numpy + state_ids     " + fmt % old_t + "   (5 calls; %.2f GB to the host)" % (n * 320 / 1e9))
    say("    gs_state_attr(OPACITY_LOGIT)          " + fmt % new_t + "   = 1 / %.0f of it" % (old_t[0] / new_t[0]))
    say("what was to be checked")
    say("  gs_state_attr(POS_X) is the BOX pass reading 5 of its 13 bytes per splat: it should take no longer than BOX, 10 % allowed for")
    say("  launch and timer noise.  Measured attr / BOX = %.3f: %s." % (ratio, "it does not" if ratio <= 1.10 else "IT DOES -- see the note below"))
    say("  the one-bin histogram should be no more than a few times the spread one.  Measured %.2f (256 bins), %.2f (1024 bins)." % (one[256], one[1024]))
    r.destroy()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
