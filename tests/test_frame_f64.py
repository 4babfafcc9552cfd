"""Projection and both blends against an f64 model written from the mathematics (tests/frame_f64.py), under general cameras.

Every GPU test of the project is anchored to oracle/gs_oracle.c, which oracle/np_oracle.py restates line by line: a misreading the
two share (a transposed rotation, swapped focal lengths, a sign of one SH basis function, the Jacobian clamp on the wrong axis) would
pass everywhere.  Here the oracle itself is held against the mathematics, and the kernels are run where no other test runs them:
fx != fy, rolled views, a camera inside the cloud, a non-rigid view matrix, uniforms under which the 1.3 tan_fov clamp of the
Jacobian fires on visible splats, and a camera that looks away from the scene.

CAMERAS (bicycle_like(6000) with the f_rest coefficients x 4; `own tile size` is the one the CPU tests use):
  rolled     roll 0.6 rad, fx, fy = 230, 170                                                           200 x 120, tile 16
  inside     orbit radius 1.2 (inside the cloud), roll -0.4, fx, fy = 90, 75, scale_modifier 3         200 x 120, tile 8
  clamp      tan_fov uniforms x 0.7 after packing: visible splats beyond 1.3 tan_fov                   200 x 120, tile 32
  nonrigid   the view's first three rows x 1.5, proj recomputed, scale_modifier 0.25                   200 x 120, tile 16
  odd        roll pi / 2, fx, fy = 150, 120                                                            131 x 77,  tile 16
  away       looks away from the origin: most splats fall to the near and ndc culls; 25 tiny splats
             are placed ON the five cull planes (margins 0, +-0.3, +-0.6 of the derived tolerance)     200 x 120, tile 16
and sixteen ONE-HOT scenes: 200 splats on a shell around the camera, one SH coefficient index nonzero, seen through six cube-face
cameras (tan_fov 1), so that every direction of the sphere is visible in one of them and no sign can hide in a sum.

TOLERANCES.  Every one is (a) a rounding-count bound k 2^-24 magnitude derived in frame_f64.py, (b) 2 E_ref with E_ref = max |oracle
f32 image - f64 image| computed from the reference when the test runs, or (c) one of two caps of 0.5 %: the pixels the f64 model
flags as decided within rounding of a threshold (gpu_checks' own max_ill), and the splats left out of a cull comparison because
their f64 margin to a cull plane is inside its tolerance.  TEETH below is no tolerance: it is what "fails by orders of magnitude"
means for the three perturbed models.

The CPU tests compare the oracle with the model.  The GPU tests run the EXACT blend (debug and
product frames, both binnings, both emission orders, tile sizes 8 / 16 / 32), three column slabs per camera for rolled / clamp /
nonrigid (one a single tile column wide), the fused blend on the same cameras and tile sizes, and eight seeded random fused
configurations; a fused frame must satisfy check_image as it stands and |fused - f64| <= 2 E_ref on the pixels neither the oracle
nor the model flags.  In the random configurations the f64 blend evaluates a seeded sample of tiles (F64_BUDGET pixel-entries), the
only place where a frame is not modelled whole: a 420 x 300 canvas inside a 40 000-splat cloud would take a minute otherwise.

MEASURED (for orientation; no test reads these).  Oracle against the model on the CPU, at the camera's own tile size: the largest
|oracle - f64| / tolerance per quantity, the splats left out of the cull comparison, the pixels the model flags, the largest
|oracle f32 image - f64 image| / bound on the others.  Then on an MI355X: E_ref and the fused blend's largest |fused - f64| at tile
sizes 8 / 16 / 32 (E_ref is the same at the three).
             uv    conic  depth  colour opacity  left out  flagged   image    E_ref      fused 8 / 16 / 32 (x E_ref)
  rolled     0.57  0.18   0.39   0.02   0.27     0      %  0.021 %   0.26     2.53e-5    1.00 / 1.06 / 1.06
  inside     0.72  0.07   0.45   0.03   0.27     0.017  %  0.221 %   0.20     1.21e-5    1.00 / 1.13 / 1.13
  clamp      0.73  0.18   0.40   0.03   0.26     0      %  0.042 %   0.33     1.57e-5    1.00 / 1.00 / 1.00
  nonrigid   0.72  0.28   0.44   0.04   0.27     0      %  0.017 %   0.29     2.10e-5    1.00 / 1.00 / 1.00
  odd        0.72  0.20   0.46   0.03   0.30     0      %  0.050 %   0.25     1.67e-5    1.00 / 1.06 / 1.06
  away       0.31  0.13   0.46   0.04   0.25     0.415  %  0.013 %   0.19     2.85e-5    1.00 / 1.00 / 1.00
The one-hot scenes: colour within 0.08 of its tolerance in all sixteen.  The perturbed models miss the conic by 1e6 (transposed
rotation) and 1e5 (swapped focal lengths) tolerances and the colour by 4e4 (one SH sign).  Random fused configurations (seeds 200 ..
207): E_ref 0.9e-5 .. 2.7e-5, fused error 0.99 .. 1.02 E_ref on debug and product frames alike, flagged 0.03 .. 0.23 % of the modelled
pixels (all of them in six frames, 40 % and 50 % in two).  The fused blend never exceeded 1.13 E_ref; no defect was found in a kernel,
in the oracle or in np_oracle.
"""
import math

import numpy as np
import pytest

import frame_f64 as f64
from support import cached, mk, oracle_frame

F = np.float32
MAX_FLAGGED = 0.005   # of a frame's pixels: gpu_checks.check_image's max_ill
MAX_LEFT_OUT = 0.005  # of a scene's splats, left out of the cull comparison
TEETH = 100.0         # a perturbed model must miss some tolerance by this factor: two orders of magnitude
F64_BUDGET = 1.0e7    # pixel-entries the f64 blend evaluates per random configuration
TILE_SIZES = (8, 16, 32)


# ---- cameras ---------------------------------------------------------------------------------------------------------------------------
def view_matrix(eye, forward, up=(0.0, 1.0, 0.0), roll=0.0):
    """Rigid world -> camera matrix (column-major f32[16]): +z along `forward`, +y down, rolled about the view axis."""
    eye, f = np.asarray(eye, np.float64), np.asarray(forward, np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(-np.asarray(up, np.float64), f)
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    r, d = math.cos(roll) * r + math.sin(roll) * d, -math.sin(roll) * r + math.cos(roll) * d
    m = np.eye(4)
    m[0:3, 0:3] = np.stack([r, d, f])
    m[0:3, 3] = -m[0:3, 0:3] @ eye
    return m.T.reshape(16).astype(F)


def pack(view, fx, fy, W, H, mod=1.0):
    from gsplat.camera import Camera, focal2fov, get_projection_matrix
    return Camera(H, W, view, get_projection_matrix(0.2, 100.0, focal2fov(fx, W), focal2fov(fy, H)), fx, fy, mod).uniforms(W, H).copy()


def cam_rolled():
    eye = (3.6, -0.8, -2.7)
    return pack(view_matrix(eye, np.negative(eye), roll=0.6), 230.0, 170.0, 200, 120), 200, 120


def cam_inside():
    eye = (1.2 * math.cos(5.0), 0.3, 1.2 * math.sin(5.0))  # (the angle: one at which splats lie between z = 0.2 and 0.3)
    return pack(view_matrix(eye, np.negative(eye), roll=-0.4), 90.0, 75.0, 200, 120, mod=3.0), 200, 120


def cam_clamp():
    eye = (-2.9, 0.8, 3.4)
    u = pack(view_matrix(eye, np.negative(eye)), 200.0, 200.0, 200, 120)
    u[35] *= F(0.7)
    u[36] *= F(0.7)
    return u, 200, 120


def cam_nonrigid():
    from gsplat.camera import focal2fov, get_projection_matrix, mat4_multiply
    eye = (0.5, 1.5, -4.2)
    u = pack(view_matrix(eye, np.negative(eye), roll=0.2), 200.0, 200.0, 200, 120, mod=0.25)
    v = u[0:16].reshape(4, 4).copy()  # v[c, r]
    v[:, 0:3] *= F(1.5)
    u[0:16] = v.reshape(16)
    u[16:32] = mat4_multiply(get_projection_matrix(0.2, 100.0, focal2fov(200.0, 200), focal2fov(200.0, 120)), u[0:16])
    return u, 200, 120


def cam_odd():
    eye = (-3.1, -0.6, -3.0)
    return pack(view_matrix(eye, np.negative(eye), roll=math.pi / 2), 150.0, 120.0, 131, 77), 131, 77


def cam_away():
    eye = (1.6, 0.4, 0.9)
    return pack(view_matrix(eye, (-0.4, -0.1, 0.9), roll=0.3), 180.0, 200.0, 200, 120), 200, 120


CAMERAS = {"rolled": (cam_rolled, 16), "inside": (cam_inside, 8), "clamp": (cam_clamp, 32), "nonrigid": (cam_nonrigid, 16),
           "odd": (cam_odd, 16), "away": (cam_away, 16)}  # name: (uniforms and canvas, own tile size)
SLAB_CAMERAS = ("rolled", "clamp", "nonrigid")


def base_scene():
    def make():
        from gsplat import synth
        s = synth.bicycle_like(6000)
        s[:, 20:80] *= F(4.0)
        return s
    return cached(("f64_base_scene",), make)


def on_plane_splats(u):
    """25 tiny splats on the five cull planes of uniforms u: per plane, f64 margins of 0, +-0.3 and +-0.6 of that plane's derived
    tolerance, robustly inside the four other planes.  The position's own rounding to f32 moves a margin by at most a quarter of
    the tolerance (one rounding per coordinate against the four the tolerance counts), so two of each five stay on the culled side."""
    V = u[0:16].astype(np.float64).reshape(4, 4).T
    Vinv = np.linalg.inv(V)
    out = []
    for plane in range(5):
        for k, frac in enumerate((-0.6, -0.3, 0.0, 0.3, 0.6)):
            lat = 0.013 * (k - 2) + 0.005 * plane
            z = 0.2 if plane == 0 else 2.5 + 0.4 * k
            tx, ty = lat * z, -0.7 * lat * z
            if plane in (1, 2):
                tx = (1.0 if plane == 1 else -1.0) * z * 1.1 * float(u[35]) * 0.999
            if plane in (3, 4):
                ty = (1.0 if plane == 3 else -1.0) * z * 1.1 * float(u[36]) * 0.999
            p = (Vinv @ np.array([tx, ty, z, 1.0]))[0:3]
            for _ in range(3):  # the margin is an affine (near) or a smooth (ndc) function of the position: Newton along its gradient
                def margin(q):
                    rec = np.zeros((1, 80))
                    rec[0, 0:3] = q
                    rec[0, 8] = 1.0
                    pr = f64.project(rec, u)
                    return pr["margins"][0, plane] - frac * pr["margin_tol"][0, plane]
                m0 = margin(p)
                grad = np.array([(margin(p + h) - m0) / 1e-6 for h in 1e-6 * np.eye(3)])
                p = p - m0 * grad / (grad @ grad)
            out.append(p)
    s = np.zeros((25, 80), F)
    s[:, 0:3] = np.array(out)
    s[:, 4:7] = math.log(0.002)
    s[:, 8] = 1.0
    s[:, 12] = 1.0
    s[:, 16:19] = [0.4, -0.3, 0.8]
    return s


def case(name):
    """(splats, uniforms, W, H) of one of CAMERAS."""
    def make():
        u, W, H = CAMERAS[name][0]()
        s = base_scene()
        if name == "away":
            s = np.concatenate([s, on_plane_splats(u)])
        return s, u, W, H
    return cached(("f64_case", name), make)


def one_hot_scene(index):
    """200 splats on a shell of radius 2 .. 4 around the origin, directions spread over the sphere (a Fibonacci lattice), coefficient
    `index` = (0.9, -0.6, 0.3), every other one zero."""
    n = 200
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * math.pi * (3.0 - math.sqrt(5.0))
    rad = 2.0 + 2.0 * ((k * 0.618033988749895) % 1.0)
    s = np.zeros((n, 80), F)
    s[:, 0] = rad * np.sqrt(1.0 - z * z) * np.cos(phi)
    s[:, 1] = rad * np.sqrt(1.0 - z * z) * np.sin(phi)
    s[:, 2] = rad * z
    s[:, 4:7] = math.log(0.05)
    s[:, 8:12] = [0.8, 0.2, -0.4, 0.3]
    s[:, 12] = 1.0
    s[:, 16 + 4 * index:19 + 4 * index] = [0.9, -0.6, 0.3]
    return s


CUBE = 128  # the cube-face canvases


def cube_faces():
    """Six cameras at (0.3, -0.2, 0.1) looking along +-x, +-y, +-z with tan_fov = 1: the ndc cull at 1.1 makes the faces overlap."""
    eye = (0.3, -0.2, 0.1)
    out = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            f = np.zeros(3)
            f[axis] = sign
            up = (0.0, 1.0, 0.0) if axis != 1 else (0.0, 0.0, 1.0)
            out.append(pack(view_matrix(eye, f, up=up), CUBE / 2.0, CUBE / 2.0, CUBE, CUBE))
    return out


# ---- the comparison of a projected frame with the model ----------------------------------------------------------------------------------
QUANTITIES = (("uv", slice(0, 2)), ("conic", slice(4, 7)), ("depth", slice(7, 8)), ("colour", slice(8, 11)), ("opacity", slice(11, 12)))


def projection_ratios(gdata, counts, p):
    """Per quantity, max over the splats both sides keep of |oracle - model| / tolerance; and the cull comparison: (number of
    decided splats on which the oracle and the model disagree, share of the splats left out as undecided)."""
    g = gdata.view(F).reshape(-1, 16).astype(np.float64)
    both = (counts > 0) & p["visible"]
    ratios = {}
    for name, sl in QUANTITIES:
        model, tol = p[name].reshape(both.size, -1), p[name + "_tol"].reshape(both.size, -1)
        ratios[name] = float((np.abs(g[:, sl] - model) / tol)[both].max(initial=0.0))
    disagree = int((((counts > 0) != p["visible"]) & p["decided"]).sum())
    return ratios, disagree, float((~p["decided"]).mean())


def model_frame(oracle, name, ts):
    """The f64 frame of a camera at a tile size over the oracle's lists, with the reference's own distance from it: a dict of the
    oracle frame `ref`, the projection `proj`, image, bound, flagged, and E_ref (max |oracle f32 - f64| over the pixels neither
    side flags)."""
    def make():
        s, u, W, H = case(name)
        ref = oracle_frame(oracle, "f64_" + name, s, u, W, H, ts, want_illcond=True)
        proj = cached(("f64_proj", name), lambda: f64.project(s, u))
        image, bound, flagged, _ = f64.blend(proj, ref["sorted_values"], ref["ranges"], W, H, ts)
        clean = ~flagged & ~ref["illcond"].astype(bool)
        e = np.abs(ref["rgbf"].astype(np.float64) - image)
        return {"ref": ref, "proj": proj, "image": image, "bound": bound, "flagged": flagged, "clean": clean,
                "E_ref": float(e[clean].max(initial=0.0))}
    return cached(("f64_frame", name, ts), make)


# ---- CPU: the scenes reach what they are for ---------------------------------------------------------------------------------------------
def test_counts_are_the_stated_ones():
    """The compound counts of frame_f64's table follow from its own calculus."""
    K, BK = f64.STAGE_K, f64.BASIS_K
    assert K["affine"] == 1 + 3 and K["norm2"] == 1 + 3 and K["scale"] == 3 + 1 and K["matmul3"] == 1 + 2 and K["opacity"] == 3 + (3 + 1) + 1
    unit = K["norm2"] / 2 + 1 + 1  # q / |q|: half the error of |q|^2, the sqrt, the quotient
    assert unit == 4 and 2 * K["norm2"] + K["rotation_inner"] == (2 * unit + 1) + 1
    assert K["direction"] == 1 + ((2 * 1 + 1 + 2) / 2 + 1) + 1
    assert BK == (1 + 1, math.ceil(K["direction"]) + 2 + 2, math.ceil(2 * K["direction"]) + 3 + 2, math.ceil(3 * K["direction"]) + 5 + 1)


def test_the_scenes_reach_what_they_are_for(oracle):
    vis, proj, ref = {}, {}, {}
    for name, (_, ts) in CAMERAS.items():
        s, u, W, H = case(name)
        m = model_frame(oracle, name, ts)
        proj[name], ref[name] = m["proj"], m["ref"]
        vis[name] = (ref[name]["tile_counts"] > 0) & proj[name]["visible"]
        assert vis[name].sum() >= (100 if name == "away" else 300), name
    # rolled, odd: fx != fy and a view whose x axis is far from horizontal
    for name in ("rolled", "odd"):
        u = case(name)[1]
        assert abs(u[37] - u[38]) >= 30 and abs(u[4]) > 0.3  # view[1][0]: the world-y part of the camera's x axis
    # inside: visible splats between the near plane and z = 0.3, and large footprints (scale_modifier 3)
    z = proj["inside"]["depth"]
    assert (vis["inside"] & (z > 0.2) & (z < 0.3)).sum() >= 3
    # clamp: visible splats beyond 1.3 tan_fov on either axis
    u, t = case("clamp")[1], proj["clamp"]["t"]
    for a in (0, 1):
        assert (vis["clamp"] & (np.abs(t[:, a] / t[:, 2]) > 1.3 * float(u[35 + a]))).sum() >= 20, a
    # nonrigid: W W^T = 2.25 I
    Wv = case("nonrigid")[1][0:16].astype(np.float64).reshape(4, 4).T[0:3, 0:3]
    np.testing.assert_allclose(Wv @ Wv.T, 2.25 * np.eye(3), atol=1e-5)
    # away: most splats culled, each of the two kinds of cull takes many, and every cull plane has culled splats within its tolerance
    p = proj["away"]
    counts = ref["away"]["tile_counts"]
    assert (counts == 0).mean() > 0.6
    assert (p["margins"][:, 0] < 0).sum() >= 1000 and ((p["margins"][:, 0] > 0) & (p["margins"][:, 1:] < 0).any(axis=1)).sum() >= 1000
    others_fine = lambda k: np.delete(p["margins"] > p["margin_tol"], k, axis=1).all(axis=1)
    for k, plane in enumerate(f64.PLANES):
        at = (np.abs(p["margins"][:, k]) <= p["margin_tol"][:, k]) & others_fine(k)
        assert (at & (counts == 0)).sum() >= 1 and (at & (p["margins"][:, k] < 0)).sum() >= 1, plane
        assert (at & (counts > 0)).sum() >= 1, plane  # ... and kept ones: the band is two-sided
    # one-hot: every direction is visible in some cube face
    s = one_hot_scene(0)
    seen = np.zeros(s.shape[0], bool)
    for u in cube_faces():
        seen |= oracle.preprocess(s, u, CUBE, CUBE, 16)[1] > 0
    assert seen.all()


# ---- CPU: the oracle against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CAMERAS))
def test_oracle_projection_matches_the_model(oracle, name):
    m = model_frame(oracle, name, CAMERAS[name][1])
    ratios, disagree, left_out = projection_ratios(m["ref"]["gdata"], m["ref"]["tile_counts"], m["proj"])
    print("%s: |oracle - f64| / tolerance %s, culls: %d disagree, %.4f %% left out" % (name, ratios, disagree, 100 * left_out))
    assert max(ratios.values()) <= 1.0, ratios
    assert disagree == 0
    assert left_out <= MAX_LEFT_OUT


@pytest.mark.parametrize("name", list(CAMERAS))
def test_oracle_image_matches_the_model(oracle, name):
    m = model_frame(oracle, name, CAMERAS[name][1])
    e = np.abs(m["ref"]["rgbf"].astype(np.float64) - m["image"])
    keep = ~m["flagged"]
    over = (e > m["bound"])[keep]
    print("%s: flagged %.4f %% (oracle's own flag: %.4f %%), max |oracle - f64| %.3g unflagged, E_ref %.3g, max bound %.3g, largest error / bound %.3g" % (
        name, 100 * m["flagged"].mean(), 100 * m["ref"]["illcond"].mean(), e[keep].max(initial=0.0), m["E_ref"],
        m["bound"][keep].max(initial=0.0), (e / np.maximum(m["bound"], 1e-300))[keep].max(initial=0.0)))
    assert not over.any(), "%d pixels beyond the model's bound" % int(over.any(axis=-1).sum())
    assert m["flagged"].mean() <= MAX_FLAGGED
    assert m["image"].max() > 0.2  # a frame, not a black canvas


@pytest.mark.parametrize("index", list(range(16)))
def test_one_hot_sh_coefficients(oracle, index):
    s = one_hot_scene(index)
    worst, seen = {}, 0
    for u in cube_faces():
        gd, counts = oracle.preprocess(s, u, CUBE, CUBE, 16)
        p = f64.project(s, u)
        ratios, disagree, left_out = projection_ratios(gd, counts, p)
        assert disagree == 0 and left_out <= MAX_LEFT_OUT
        seen += int((counts > 0).sum())
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in ratios.items()}
        # the basis function is there at all: its coefficient moves the colour of the visible splats
        assert np.abs(p["colour"][counts > 0] - 0.5).max() > 0.1
    assert seen >= s.shape[0]
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("perturb", f64.PERTURBATIONS)
def test_the_pin_has_teeth(oracle, perturb):
    """A model with a transposed rotation, swapped focal lengths or one flipped SH sign misses the oracle by orders of magnitude --
    so would an oracle with that misreading miss the true model."""
    name = "rolled"
    s, u, W, H = case(name)
    ref = model_frame(oracle, name, CAMERAS[name][1])["ref"]
    ratios, _, _ = projection_ratios(ref["gdata"], ref["tile_counts"], f64.project(s, u, perturb=perturb))
    print(perturb, ratios)
    hit = {"transposed_rotation": "conic", "swapped_focal": "conic", "sh_sign": "colour"}[perturb]
    assert ratios[hit] >= TEETH, ratios
    assert all(v <= 1.0 for k, v in ratios.items() if k != hit), ratios  # ... and touches nothing else
    if perturb == "sh_sign":  # one sign: exactly one one-hot scene notices, through a single cube face already
        for index in (10, 11, 12):
            s1, u1 = one_hot_scene(index), cube_faces()[0]
            gd, counts = oracle.preprocess(s1, u1, CUBE, CUBE, 16)
            r = projection_ratios(gd, counts, f64.project(s1, u1, perturb=perturb))[0]
            assert (r["colour"] >= TEETH) == (index == 11), (index, r)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------
def check_against_f64(r, ref, image, flagged, label, done=None):
    """|fused - f64| <= 2 E_ref on the pixels neither the oracle nor the model flags, E_ref = max |oracle f32 - f64| there.  done: the
    pixels the model evaluated (all of them if None)."""
    from gsplat import _abi
    H, W = ref["rgbf"].shape[0:2]
    done = np.ones((H, W), bool) if done is None else done
    clean = done & ~flagged & ~ref["illcond"].astype(bool)
    got = r.read_buffer(_abi.GS_BUF_RGB_F32, F).reshape(H, W, 3).astype(np.float64)
    e_ref = float(np.abs(ref["rgbf"].astype(np.float64) - image)[clean].max(initial=0.0))
    e_gpu = float(np.abs(got - image)[clean].max(initial=0.0))
    print("F64 %s: E_ref %.4g, fused error %.4g (%.2f E_ref), clean pixels %.4f %%" % (label, e_ref, e_gpu, e_gpu / max(e_ref, 1e-300),
                                                                                  100 * clean.sum() / max(int(done.sum()), 1)))
    assert (flagged & done).sum() <= MAX_FLAGGED * done.sum()
    assert e_gpu <= 2 * e_ref, "%s: the fused blend is %.4g from the f64 image, the reference %.4g" % (label, e_gpu, e_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("ts", TILE_SIZES)
@pytest.mark.parametrize("name", list(CAMERAS))
def test_exact_frames(oracle, name, ts):
    """EXACT blend: a debug frame tap by tap, product frames in both binnings and both emission orders (the tight lists as a provably
    harmless subset), every image bit-equal."""
    from gpu_checks import check_stages
    from gsplat import _abi
    s, u, W, H = case(name)
    ref = oracle_frame(oracle, "f64_" + name, s, u, W, H, ts, want_illcond=True)
    r = mk(s, W, H, ts, exact=True)
    r.render_uniforms(u, debug=True)
    r.wait()
    check_stages(r, ref, exact_image=True)
    for cull in (1, 0):
        for order in (1, 0):
            r.set_option(_abi.GS_OPT_TILE_CULL, cull)
            r.set_option(_abi.GS_OPT_EMIT_ORDER, order)
            r.render_uniforms(u)
            r.wait()
            st = r.stats()
            assert st["tight_binning"] == cull and st["depth_ordered"] == (1 if cull else 1 - order)  # a tight frame is depth-ordered
            check_stages(r, ref, exact_image=True, debug=False, oracle=oracle, W=W, H=H, ts=ts)
    r.destroy()


def slabs_of(W, ts):
    """Three tile-column slabs whose union is the canvas, the middle one a single column wide."""
    ntx = -(-W // ts)
    mid = ntx // 2
    return [(0, mid), (mid, mid + 1), (mid + 1, ntx)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SLAB_CAMERAS)
def test_slabs(oracle, name):
    from gpu_checks import check_stages
    s, u, W, H = case(name)
    ts = CAMERAS[name][1]
    whole = mk(s, W, H, ts, exact=True)
    whole.render_uniforms(u)
    whole.wait()
    img = whole.read_rgba8()
    whole.destroy()
    parts = []
    for cols in slabs_of(W, ts):
        ref = oracle.render(s, u, W, H, ts, cols=cols)
        r = mk(s, W, H, ts, exact=True, cols=cols)
        r.render_uniforms(u, debug=True)
        r.wait()
        check_stages(r, ref, exact_image=True)
        r.render_uniforms(u)
        r.wait()
        assert r.stats()["tight_binning"] == 1
        check_stages(r, ref, exact_image=True, debug=False, oracle=oracle, W=W, H=H)
        parts.append(r.read_rgba8())
        r.destroy()
    assert [p.shape[1] for p in parts][1] == ts
    np.testing.assert_array_equal(np.concatenate(parts, axis=1), img)


@pytest.mark.gpu
@pytest.mark.parametrize("ts", TILE_SIZES)
@pytest.mark.parametrize("name", list(CAMERAS))
def test_fused_frames(oracle, name, ts):
    """Default flags, the mode the product ships: check_image as it stands, and the distance from the f64 image."""
    from gpu_checks import check_stages
    m = model_frame(oracle, name, ts)
    s, u, W, H = case(name)
    r = mk(s, W, H, ts)
    r.render_uniforms(u)
    r.wait()
    check_stages(r, m["ref"], exact_image=False, debug=False, oracle=oracle, W=W, H=H, ts=ts)
    check_against_f64(r, m["ref"], m["image"], m["flagged"], "%s/%d" % (name, ts))
    r.destroy()


# Eight consecutive seeds.  Where a camera sits among 40 000 splats at scale_modifier 3, most pixels end with T within rounding of the
# 1e-4 threshold after hundreds of entries, and the model flags several percent of the frame: such a frame says little here (the blend's
# culls at that threshold have tests/test_blend_culls.py).  200 is the first multiple of 100 from which eight consecutive seeds stay
# under MAX_FLAGGED -- a property of the seeded scenes and the model, found without any kernel.
RANDOM_SEEDS = list(range(200, 208))


def random_config(seed):
    """(splats, uniforms, W, H, tile size): tile size, odd canvas, scene size and scale modifier drawn as test_random_configs_exact
    draws them, and a general camera: orbit radius 1 .. 9, roll, fx != fy."""
    from gsplat import synth
    rng = np.random.default_rng(2000 + seed)
    ts = int(rng.choice([8, 16, 16, 32]))
    W, H = int(rng.integers(33, 420)), int(rng.integers(17, 300))
    n = int(rng.integers(1, 40000))
    s = synth.bicycle_like(n, seed=synth.BASE_SEED + 70 + seed)
    th, radius, height = float(rng.uniform(0, 2 * math.pi)), float(rng.uniform(1.0, 9.0)), float(rng.uniform(-2.0, 3.0))
    eye = (radius * math.cos(th), height, radius * math.sin(th))
    fx, fy = float(W * rng.uniform(0.6, 1.5)), float(W * rng.uniform(0.6, 1.5))
    u = pack(view_matrix(eye, np.negative(eye), roll=float(rng.uniform(-math.pi, math.pi))), fx, fy, W, H)
    u[39] = F(rng.choice([0.25, 1.0, 1.0, 3.0]))
    return s, u, W, H, ts


def sample_tiles(ref, W, H, ts, seed):
    """Tiles in a seeded random order while their pixel-entries fit F64_BUDGET (at least one tile)."""
    lens = np.diff(np.concatenate([[0], ref["ranges"].astype(np.int64)]))
    order = np.random.default_rng(3000 + seed).permutation(lens.size)
    cost = np.cumsum(lens[order] * ts * ts)
    return order[:max(1, int(np.searchsorted(cost, F64_BUDGET, side="right")))]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_configs_fused(oracle, seed):
    """A debug frame and a product frame of the fused blend per seeded configuration: every list, check_image as it stands, and the
    distance from the f64 image on the modelled tiles."""
    from gpu_checks import check_stages
    s, u, W, H, ts = random_config(seed)
    ref = oracle.render(s, u, W, H, ts, want_illcond=True)
    image, _, flagged, done = f64.blend(f64.project(s, u), ref["sorted_values"], ref["ranges"], W, H, ts, tiles=sample_tiles(ref, W, H, ts, seed))
    r = mk(s, W, H, ts)
    r.render_uniforms(u, debug=True)
    r.wait()
    check_stages(r, ref, exact_image=False)
    check_against_f64(r, ref, image, flagged, "seed %d debug" % seed, done)
    r.render_uniforms(u)
    r.wait()
    check_stages(r, ref, exact_image=False, debug=False, oracle=oracle, W=W, H=H, ts=ts)
    check_against_f64(r, ref, image, flagged, "seed %d (%d splats, %d x %d, tile %d, %.0f %% of the pixels modelled)" % (
        seed, s.shape[0], W, H, ts, 100 * done.mean()), done)
    r.destroy()
