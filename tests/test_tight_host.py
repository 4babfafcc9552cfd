"""CPU: the tight binning's geometry (gaussian-splatting-wgpu_amd/csrc/gs_tight.h -- the row items of the product path, compiled for the host)
against the oracle's exact contribution masks (oracle.instance_masks): no instance that contributes to a pixel under the
canonical arithmetic may be dropped, and every kept instance's sub-block mask must cover its contributing blocks.  The GPU
tests prove the same for the kernels (tests/gpu_checks.py::check_product_lists); this one runs without a GPU.

The bicycle_like cases almost never put a contributing pixel on the contour; the margin scene (support.tight_margin_scene) does, and
the teeth test proves it: the same scene run through copies of the header with margins removed (CPU only, a temporary copy) must
find dropped instances or mask misses.  profiles/tight_margins.txt records the figures the bounds below come from."""
import importlib.util
import os

import pytest

from support import ROOT, cached, tight_scene

_spec = importlib.util.spec_from_file_location("tight_check_run", os.path.join(ROOT, "tools", "tight_check", "run.py"))
tight_check = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tight_check)

TILES = (8, 16, 32)

# kept / exactly contributing, measured with the committed header (profiles/tight_margins.txt) plus 10 %: a margin tweak moves the
# ratio by a few per cent, a fall-back to the reference's rect everywhere at least doubles it on the bicycle_like cases
BICYCLE_RATIO = {(20000, 640, 360, 16, 3, 1.0): 1.1 * 1.0567, (15000, 320, 200, 8, 5, 1.0): 1.1 * 1.0854, (15000, 640, 480, 32, 9, 1.0): 1.1 * 1.0240,
                 (6000, 256, 256, 16, 40, 2.5): 1.1 * 1.0440}
MARGIN_RATIO = {8: 1.1 * 3.8442, 16: 1.1 * 2.8537, 32: 1.1 * 2.0300}  # (thin far-reaching splats: their 8 px strips hold few pixels)

# the mutated headers: (old, new) pairs, each of which must match the committed text exactly once
SLACK = ("const float slack = 0.02f + 1.0e-5f * (__builtin_fabsf(xlo) + __builtin_fabsf(xhi) + __builtin_fabsf(g.gx));", "const float slack = 0.0f;")
LIM = ("* 0.693147182464599609375f + 0.01f;", "* 0.693147182464599609375f;")
QA = ("g.qa = (cyy - g.cxz) + 1.0e-5f * (cyy + g.cxz);", "g.qa = (cyy - g.cxz);")
QB = ("g.qb = (g.lim2 * cx) * 1.00001f;", "g.qb = (g.lim2 * cx);")
ER = ("g.eR = __builtin_fabsf(g.dyR) * ((D - Dlo) / Dlo + 4.0e-4f) + 0.02f;", "g.eR = 0.0f;")
XMAX = ("g.xmax = __builtin_sqrtf(g.lim2 * 1.0001f * cz / Dlo) * 1.0002f + 0.02f;", "g.xmax = __builtin_sqrtf(g.lim2 * 1.0001f * cz / Dlo);")
YMAX = ("g.ymax = __builtin_sqrtf(g.lim2 * 1.0001f * cx / Dlo) * 1.0002f + 0.02f;", "g.ymax = __builtin_sqrtf(g.lim2 * 1.0001f * cx / Dlo);")
MUTATIONS = {"no_slack": [SLACK], "no_eR": [ER], "no_lim_margin": [LIM], "no_discriminant_inflation": [QA, QB], "no_extent_inflation": [XMAX, YMAX],
             "no_slack_lim_discriminant": [SLACK, LIM, QA, QB]}


def mutated_header(name):
    text = tight_check.header_text()
    for old, new in MUTATIONS[name]:
        assert text.count(old) == 1, "gs_tight.h no longer holds exactly one %r: restate the mutation" % old
        text = text.replace(old, new)
    return text


def margin_run(oracle, name, ts, mutation=None):
    def make():
        t = tight_scene(oracle, name)
        return tight_check.check(t["splats"], t["uniforms"], t["W"], t["H"], ts, None if mutation is None else mutated_header(mutation))
    return cached(("tight_host", name, ts, mutation), make)


@pytest.mark.parametrize("case", list(BICYCLE_RATIO))
def test_row_items_drop_nothing_that_contributes(case):
    n, W, H, ts, step, mod = case
    s, u = tight_check.bicycle_case(n, W, H, ts, step, mod)
    res = tight_check.check(s, u, W, H, ts)
    print("kept / exactly contributing %.4f (%d / %d of %d)" % (res["ratio"], res["kept"], res["contributing"], res["ref"]))
    assert res["returncode"] == 0, res["stdout"][-2000:]
    assert res["dropped"] == 0 and res["misses"] == 0
    assert 0 < res["kept"] <= res["ref"]  # an ordered subset of the reference's instances ...
    assert res["ratio"] <= BICYCLE_RATIO[case]  # ... and not much more than what contributes


def test_command_line_still_reports(tmp_path):
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tight_check", "run.py"), "2000", "128", "96", "16", "3"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "dropped-but-contributing 0 | mask misses 0" in out.stdout


@pytest.mark.parametrize("ts", TILES)
def test_margin_scene_drops_nothing_that_contributes(oracle, ts):
    res = margin_run(oracle, "tight_margins", ts)
    print("kept / exactly contributing %.4f (%d / %d of %d)" % (res["ratio"], res["kept"], res["contributing"], res["ref"]))
    assert res["dropped"] == 0 and res["misses"] == 0, res["stdout"][-2000:]
    assert 0 < res["kept"] <= res["ref"]
    assert res["ratio"] <= MARGIN_RATIO[ts]


def test_margin_scene_has_teeth(oracle):
    """The header without its slack, its +0.01 and its discriminant inflation is caught at every tile size, the header with eR = 0
    at one at least; which single removals are caught is recorded in profiles/tight_margins.txt, not required (the margins overlap)."""
    found = {}
    for m in ("no_slack_lim_discriminant", "no_eR"):
        for ts in TILES:
            res = margin_run(oracle, "tight_margins", ts, m)
            found[m, ts] = res["dropped"] + res["misses"]
    print(found)
    assert all(found["no_slack_lim_discriminant", ts] > 0 for ts in TILES), found
    assert any(found["no_eR", ts] > 0 for ts in TILES), found


def test_every_mutation_still_matches_the_header():
    for name in MUTATIONS:
        assert mutated_header(name) != tight_check.header_text()
