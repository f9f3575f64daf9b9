"""Polygon lights of next-event estimation (rt_set_light_shapes, csrc/rt_light.h;
DESIGN.md section 25) on the CPU backend — no GPU needed.  The HIP kernels
compute the same bits (tests/test_gpu_light_shapes.py).

What is checked here: the interface; the light table with its polygon records
and what is kept out of it; that the mode changes nothing where it cannot act;
that sampling emissive triangles and quads has the default estimator's
expectation (the z protocol of tests/test_light_sampling.py) and a smaller
variance; the geometry cases; shards, adaptive calls, toggling and the
downstream passes.
"""
import subprocess

import numpy as np
import pytest

from bwrt import Renderer, abi, scenefile, scenes
from bwrt.abi import Quad, Sphere, Triangle, Vec3
from bwrt.scenes import material, vec
from test_adaptive import adaptive_sequence, check_replay
from test_light_sampling import CLI, LUM, assert_same_expectation, dark_07, read_ppm, same_state, state, z_scores


def cpu(lib, scene, shapes="all", pick="uniform", on=True, threads=0):
    r = Renderer.cpu(threads, lib=lib)
    r.set_scene(scene)
    r.set_light_sampling(on)
    r.set_light_picking(pick)
    r.set_light_shapes(shapes)
    return r


def quad(verts, mat):
    return Quad((Vec3 * 4)(*[vec(*p) for p in verts]), mat)


def tri(verts, mat):
    return Triangle((Vec3 * 3)(*[vec(*p) for p in verts]), mat)


PANEL = material((1, 0.9, 0.7), 12)


def panel_quads(mat=PANEL, y=4.0):
    """Four unit quads (unit normals) side by side, above and behind the camera's view."""
    return [quad([(x, y, z), (x + 1, y, z), (x + 1, y, z + 1), (x, y, z + 1)], mat) for x in (-1, 0) for z in (-5, -4)]


def panel_triangles(mat=PANEL, y=4.0):
    out = []
    for x in (-1, 0):
        for z in (-5, -4):
            out.append(tri([(x, y, z), (x + 1, y, z), (x, y, z + 1)], mat))
            out.append(tri([(x + 1, y, z + 1), (x, y, z + 1), (x + 1, y, z)], mat))
    return out


def with_polygons(s, triangles=(), quads=(), name=""):
    n = s.counts
    return scenes.Scene(s.camera, list(s.spheres)[:n[0]], list(s.planes)[:n[1]], list(s.triangles)[:n[2]] + list(triangles),
                        list(s.quads)[:n[3]] + list(quads), name=name)


def quad_panel():
    return with_polygons(dark_07(), quads=panel_quads(), name="quad_panel")


def triangle_panel():
    return with_polygons(dark_07(), triangles=panel_triangles(), name="triangle_panel")


def mixed():
    return with_polygons(scenes.scene_07(), quads=panel_quads(), name="mixed")


def box_with_emissive_quad():
    """04_box (the QUADS hit loop) with its top mirror quad made emissive; its
    normal has length 200, so the quad itself is no NEE level."""
    s = scenes.scene_04_box()
    s.quads[4].mat.emittance = 0.5
    return s


STRESS_LIT = (3, 17, 4242, 9999)


def stress_with_emissive_triangles():
    s = scenes.stress_scene()
    for i in STRESS_LIT:
        s.triangles[i].mat.emittance = 15.0
    return s


# ---- interface ----------------------------------------------------------------------

def test_abi_and_defaults(bwrt_lib):
    names = {"rt_set_light_shapes", "rt_get_light_shapes"}
    assert names <= set(abi.declared_functions())
    for n in names:
        assert hasattr(bwrt_lib, n)
    assert (abi.RT_LIGHT_SHAPES_SPHERES, abi.RT_LIGHT_SHAPES_ALL) == (0, 1)
    with Renderer.cpu(1, lib=bwrt_lib) as r:
        assert r.light_shapes == "spheres" and bwrt_lib.rt_get_light_shapes(r.ctx) == 0
        r.set_light_shapes("all")
        assert r.light_shapes == "all" and bwrt_lib.rt_get_light_shapes(r.ctx) == 1
        assert r.light_sampling is False and r.light_picking == "uniform"  # the switches are independent
        for bad in (2, -1, 7):
            assert bwrt_lib.rt_set_light_shapes(r.ctx, bad) == abi.RT_ERR_INVALID_ARGUMENT
            assert "rt_set_light_shapes" in bwrt_lib.rt_last_error(r.ctx).decode()
        assert r.light_shapes == "all"
        with pytest.raises(ValueError):
            r.set_light_shapes("polygons")
        r.set_light_shapes("spheres")
        assert r.light_shapes == "spheres"
    assert bwrt_lib.rt_set_light_shapes(None, 1) == bwrt_lib.rt_set_light_picking(None, 1) == abi.RT_ERR_INVALID_ARGUMENT
    assert bwrt_lib.rt_get_light_shapes(None) == 0


def test_reference_fast_stays_refused(bwrt_lib):
    """The shapes mode does not open the reference-fast mode to light sampling
    (a CPU context has no such mode at all; the GPU file checks the render)."""
    with Renderer.cpu(1, lib=bwrt_lib) as r:
        r.set_light_shapes("all")
        assert bwrt_lib.rt_set_precision(r.ctx, abi.RT_PRECISION_REFERENCE_FAST) == abi.RT_ERR_UNSUPPORTED


def test_cli_flag_matches_python(bwrt_lib, tmp_path):
    def run(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)

    assert "--light-shapes" in run("--help").stdout
    r = run("--light-shapes", "all")
    assert r.returncode == 2 and "--light-sampling" in r.stderr
    r = run("--light-sampling", "--light-shapes", "polygons")
    assert r.returncode == 2 and "--light-shapes" in r.stderr
    w, h = 64, 36
    path = tmp_path / "panel.scene"
    scenefile.save(str(path), quad_panel())
    common = ("--cpu", "2", "--scene-file", str(path), "--width", str(w), "--height", str(h), "--frames", "3",
              "--max-bounces", "4", "--light-sampling")
    imgs = {}
    for shapes in ("spheres", "all"):
        out = tmp_path / f"{shapes}.ppm"
        r = run(*common, "--light-shapes", shapes, "--out", str(out))
        assert r.returncode == 0, r.stderr
        imgs[shapes] = read_ppm(out)
        with cpu(bwrt_lib, scenefile.load(str(path)), shapes, threads=2) as p:
            img = None
            for f in range(3):  # the CLI renders --frames-per-call 1
                img = p.render(w, h, 1, 4, first_frame=1 if f == 0 else 0)
        assert np.array_equal(imgs[shapes], img[..., :3]), shapes
    assert not np.array_equal(imgs["spheres"], imgs["all"])


# ---- the light table ------------------------------------------------------------------

def polygons_of(scene):
    """(primitive id, vertices, material) of every triangle and quad"""
    ns, npl, nt, nq = scene.counts
    out = [(ns + npl + i, scene.triangles[i].vertices, scene.triangles[i].mat) for i in range(nt)]
    return out + [(ns + npl + nt + i, scene.quads[i].vertices, scene.quads[i].mat) for i in range(nq)]


@pytest.mark.parametrize("make,polys", [(quad_panel, 4), (triangle_panel, 8), (mixed, 4), (box_with_emissive_quad, 1),
                                        (stress_with_emissive_triangles, len(STRESS_LIT))])
def test_light_table(bwrt_lib, make, polys):
    scene = make()
    with cpu(bwrt_lib, scene, "spheres") as r:
        sph = r.lights()
        r.set_light_shapes("all")
        tab = r.lights()
        assert tab.dtype.names == ("centre", "r2", "emitted", "prim")
        r.set_light_shapes("spheres")
        assert r.lights().tobytes() == sph.tobytes()  # rt_get_lights follows the mode
    assert len(tab) == len(sph) + polys
    assert tab[:len(sph)].tobytes() == sph.tobytes()
    assert (np.diff(tab["prim"]) > 0).all()
    assert (tab["prim"][:len(sph)] < scene.counts[0]).all()
    by_id = {pid: (v, m) for pid, v, m in polygons_of(scene)}
    want = [pid for pid, _, m in polygons_of(scene) if m.emittance > 0]
    assert [int(p) for p in tab["prim"][len(sph):]] == want
    for rec in tab[len(sph):]:
        v, m = by_id[int(rec["prim"])]
        c = rec["centre"].astype(np.float64)
        for p in v:
            assert ((np.array([p.x, p.y, p.z], np.float64) - c) ** 2).sum() <= float(rec["r2"])
        # the hit table's floats: emittance * albedo in float
        e = np.float32(m.emittance) * np.array([m.albedo.x, m.albedo.y, m.albedo.z], np.float32)
        assert np.array_equal(rec["emitted"], e)


def exclusion_scene():
    """dark_07 with seven emissive triangles and seven emissive quads of which the
    light table admits the first triangle and the first and fourth quad; returns
    (scene, the admitted primitive ids)."""
    lit = material((1, 1, 1), 5)
    ok_t = [(0, 3, -4), (1, 3, -4), (0, 3, -3)]
    ok_q = [(0, 5, -4), (1, 5, -4), (1, 5, -3), (0, 5, -3)]
    tris = [
        tri(ok_t, lit),                                             # in
        tri([(0, 3, -4), (float("nan"), 3, -4), (0, 3, -3)], lit),  # NaN vertex
        tri([(0, 3, -4), (1, 3, -4), (2, 3, -4)], lit),             # zero area
        tri(ok_t, material((1, 1, 1), float("inf"))),
        tri(ok_t, material((1, 1, 1), float("nan"))),
        tri(ok_t, material((1, 1, 1), -1.0)),
        tri(ok_t, material((1, 1, 1), 0.0)),
    ]
    quads = [
        quad(ok_q, lit),                                                   # in
        quad([(0, 5, -4), (1, 5, -4), (0, 5, -3), (1, 5, -3)], lit),       # bow-tie
        quad([(0, 5, -4), (1, 5, -4), (0.25, 5, -3.75), (0, 5, -3)], lit),   # reflex vertex v2
        quad([(0, 5, -4), (1, 5, -4), (1, 5, -3), (0, 5.3, -3)], lit),     # non-planar, its projection convex: in
        quad([(0, 5, -4), (float("inf"), 5, -4), (1, 5, -3), (0, 5, -3)], lit),
        quad(ok_q, material((1, 1, 1), float("inf"))),
        quad([(0, 5, -4), (1, 5, -4), (2, 5, -4), (0, 5, -3)], lit),       # first half of zero area
    ]
    scene = with_polygons(dark_07(), tris, quads, name="exclusions")
    ns, npl, nt, _ = scene.counts
    t0, q0 = ns + npl + nt - len(tris), ns + npl + nt
    return scene, [t0, q0, q0 + 3]


def test_light_table_exclusions(bwrt_lib):
    scene, admitted = exclusion_scene()
    with cpu(bwrt_lib, scene) as r:
        assert [int(p) for p in r.lights()["prim"]] == admitted
        r.set_light_shapes("spheres")
        assert len(r.lights()) == 0


# ---- identities -------------------------------------------------------------------------

W0, H0 = 67, 45


def test_no_op_with_light_sampling_off(bwrt_lib):
    with cpu(bwrt_lib, quad_panel(), "spheres", on=False) as a, cpu(bwrt_lib, quad_panel(), "all", on=False) as b:
        same_state(state(a, W0, H0, 3, 4), state(b, W0, H0, 3, 4))


@pytest.mark.parametrize("name", ["07", "stress"])
@pytest.mark.parametrize("pick", ["uniform", "weighted"])
def test_all_is_spheres_without_a_polygon_emitter(bwrt_lib, name, pick):
    with cpu(bwrt_lib, scenes.SCENES[name](), "spheres", pick) as a, cpu(bwrt_lib, scenes.SCENES[name](), "all", pick) as b:
        assert a.lights().tobytes() == b.lights().tobytes()
        same_state(state(a, W0, H0, 3, 4), state(b, W0, H0, 3, 4))


def test_spheres_on_a_polygon_lit_scene_is_the_default(bwrt_lib):
    with cpu(bwrt_lib, triangle_panel(), "spheres", on=False) as a, cpu(bwrt_lib, triangle_panel(), "spheres") as b:
        same_state(state(a, W0, H0, 3, 4), state(b, W0, H0, 3, 4))


def test_all_at_zero_bounces_is_the_default(bwrt_lib):
    with cpu(bwrt_lib, quad_panel(), "spheres", on=False) as a, cpu(bwrt_lib, quad_panel(), "all") as b:
        same_state(state(a, W0, H0, 3, 0), state(b, W0, H0, 3, 0))


@pytest.mark.parametrize("make", [quad_panel, triangle_panel, mixed])
def test_all_acts_and_draws_three_numbers_per_level(bwrt_lib, make):
    """frameSum and RNG state differ from the default's; the path does not
    depend on the pick or on the kind of the picked light, so the RNG state is
    the same under both picks, and on Mixed the same as under SPHERES (the
    levels are the same hits: every diffuse hit with a scattered ray)."""
    with cpu(bwrt_lib, make(), "all", on=False) as d, cpu(bwrt_lib, make(), "all", "uniform") as u, \
            cpu(bwrt_lib, make(), "all", "weighted") as w:
        sd, su, sw = state(d, W0, H0, 3, 4), state(u, W0, H0, 3, 4), state(w, W0, H0, 3, 4)
    assert not np.array_equal(sd[1], su[1], equal_nan=True)
    assert not np.array_equal(sd[2], su[2])
    assert np.array_equal(su[2], sw[2])
    assert not np.array_equal(su[1], sw[1], equal_nan=True)
    if make is mixed:
        with cpu(bwrt_lib, make(), "spheres") as s:
            ss = state(s, W0, H0, 3, 4)
        assert np.array_equal(ss[2], su[2])
        assert not np.array_equal(ss[1], su[1], equal_nan=True)


# ---- same expectation as the default estimator, smaller variance ---------------------------

W, H, BATCHES, FRAMES = 80, 48, 32, 128


def block_means(lib, scene, shapes, pick, on, mb, w=W, h=H, batches=BATCHES, frames=FRAMES, rows=None, spp=1):
    """tests/test_light_sampling.py's block_means with the two modes: (batches,
    blocks) luminance means over 8x8 blocks and (batches,) frame means."""
    rows = h if rows is None else rows
    out, whole = [], []
    with cpu(lib, scene, shapes, pick, on) as r:
        r.set_samples_per_pixel(spp)
        r.init_rand(w, h)
        for _ in range(batches):
            _, acc = r.render(w, h, frames, mb, first_frame=1, want_accum=True)
            lum = (acc.astype(np.float64) / frames) @ LUM
            whole.append(lum.mean())
            out.append(lum[:rows].reshape(rows // 8, 8, w // 8, 8).mean((1, 3)).ravel())
    return np.array(out), np.array(whole)


SCENES3 = {"quad": quad_panel, "triangle": triangle_panel, "mixed": mixed}
CASES = [(s, mb) for s in SCENES3 for mb in (4, 1)]
# the default estimator on these scenes (the issue's figures): lit blocks and
# the largest relative standard error of a lit block
BLIND = {("quad", 4): (34, 0.051), ("quad", 1): (32, 0.034), ("triangle", 4): (34, 0.051), ("triangle", 1): (32, 0.034),
         ("mixed", 4): (37, 0.026), ("mixed", 1): (37, 0.027)}
_RUNS = {}


def runs(lib, scene, mb, what):
    """what: "default", "spheres" (uniform pick), "uniform" or "weighted" (ALL) — computed once"""
    key = (scene, mb, what)
    if key not in _RUNS:
        shapes, pick, on = {"default": ("spheres", "uniform", False), "spheres": ("spheres", "uniform", True),
                            "uniform": ("all", "uniform", True), "weighted": ("all", "weighted", True)}[what]
        _RUNS[key] = block_means(lib, SCENES3[scene](), shapes, pick, on, mb)
    return _RUNS[key]


@pytest.mark.parametrize("scene,mb", CASES)
@pytest.mark.parametrize("pick", ["uniform", "weighted"])
def test_same_expectation(bwrt_lib, scene, mb, pick):
    """ALL against the default estimator.  Measured on the CPU backend
    (deterministic), lit blocks, max |z|, rms z, frame z:
      quad 4 uniform      34  2.26  1.21  0.59     quad 4 weighted      34  2.28  1.21  0.61
      quad 1 uniform      32  2.16  1.07  1.01     quad 1 weighted      32  2.16  1.06  1.04
      triangle 4 uniform  34  2.27  1.21  0.62     triangle 4 weighted  34  2.26  1.21  0.62
      triangle 1 uniform  32  2.17  1.08  1.03     triangle 1 weighted  32  2.15  1.08  1.06
      mixed 4 uniform     37  2.43  1.01  0.20     mixed 4 weighted     37  2.55  1.02  0.20
      mixed 1 uniform     37  2.60  0.88  0.19     mixed 1 weighted     37  2.48  0.92  0.21
    (default relative standard error of a lit block at most 5.1 %, 3.4 %, 5.1 %,
    3.4 %, 2.6 %, 2.7 %).
    """
    d, a = runs(bwrt_lib, scene, mb, "default"), runs(bwrt_lib, scene, mb, pick)
    z, zf, lit, ma, sa, sb = z_scores(d, a)
    # the test cannot go blind: the default estimator resolves every lit block
    print(f"{scene}/{mb}: lit {int(lit.sum())}, default relative standard error at most {(sa[lit] / ma[lit]).max():.3f}")
    assert lit.sum() >= 30 and lit.sum() == BLIND[scene, mb][0]
    assert (sa[lit] / ma[lit]).max() <= 0.08
    assert abs((sa[lit] / ma[lit]).max() - BLIND[scene, mb][1]) < 0.001
    assert_same_expectation(d, a, f"{scene} at {mb} bounces, {pick}")


# measured ratios of the summed squared block standard errors over the default
# estimator's lit blocks (32 batches of 128 frames, 80x48): ALL over the default
# estimator, and on Mixed ALL over sphere-only NEE (uniform pick).  Pinned at
# x 1.25 as section 23's: a variance estimate from 32 batches wobbles by about
# sqrt(2 / 31) = 25 %.
VAR_RATIO = {
    ("quad", 4, "uniform"): 0.0402, ("quad", 4, "weighted"): 0.0387,
    ("quad", 1, "uniform"): 0.0273, ("quad", 1, "weighted"): 0.0253,
    ("triangle", 4, "uniform"): 0.0391, ("triangle", 4, "weighted"): 0.0371,
    ("triangle", 1, "uniform"): 0.0273, ("triangle", 1, "weighted"): 0.0245,
    ("mixed", 4, "uniform"): 0.1847, ("mixed", 4, "weighted"): 0.1094,
    ("mixed", 1, "uniform"): 0.1073, ("mixed", 1, "weighted"): 0.0486,
}
# (sphere-only NEE over the default on Mixed: 0.787 at 4 bounces, 0.747 at 1 — the panel is most of its light)
VAR_RATIO_SPHERES = {(4, "uniform"): 0.2347, (4, "weighted"): 0.1390, (1, "uniform"): 0.1437, (1, "weighted"): 0.0651}


@pytest.mark.parametrize("scene,mb", CASES)
@pytest.mark.parametrize("pick", ["uniform", "weighted"])
def test_variance_is_below_the_default(bwrt_lib, scene, mb, pick):
    d, a = runs(bwrt_lib, scene, mb, "default"), runs(bwrt_lib, scene, mb, pick)
    _, _, lit, _, sd, sa = z_scores(d, a)
    ratio = (sa[lit] ** 2).sum() / (sd[lit] ** 2).sum()
    print(f"variance ratio ALL / default, {scene}/{mb}/{pick}: {ratio:.4f}")
    assert ratio < 1.0
    assert ratio <= 1.25 * VAR_RATIO[scene, mb, pick]


@pytest.mark.parametrize("mb", [4, 1])
@pytest.mark.parametrize("pick", ["uniform", "weighted"])
def test_variance_on_mixed_is_below_sphere_only_nee(bwrt_lib, mb, pick):
    d, s, a = runs(bwrt_lib, "mixed", mb, "default"), runs(bwrt_lib, "mixed", mb, "spheres"), runs(bwrt_lib, "mixed", mb, pick)
    _, _, lit, _, _, ss = z_scores(d, s)
    _, _, _, _, _, sa = z_scores(d, a)
    ratio = (sa[lit] ** 2).sum() / (ss[lit] ** 2).sum()
    print(f"variance ratio ALL / sphere-only NEE, mixed/{mb}/{pick}: {ratio:.4f}")
    assert ratio < 1.0
    assert ratio <= 1.25 * VAR_RATIO_SPHERES[mb, pick]


# ---- geometry cases ----------------------------------------------------------------------

GW, GH = 32, 18


def finite_and_repeatable(lib, scene, mb=4, frames=4, pick="uniform", spp=1):
    res = []
    for _ in range(2):
        with cpu(lib, scene, "all", pick) as r:
            r.set_samples_per_pixel(spp)
            assert len(r.lights()) > 0
            res.append(state(r, GW, GH, frames, mb, calls=2))
    same_state(res[0], res[1])
    assert np.isfinite(res[0][-1]).all()
    return res[0]


def means_agree(lib, scene, what, mb=4, frames=256, batches=16, pick="uniform", spp=1, other=None):
    """The z rule against the default estimator (or against `other`'s ALL
    render) at 32x18, 16 batches of `frames` frames; the default's relative
    standard error on the whole-frame mean must be at most 8 %."""
    kw = dict(w=GW, h=GH, rows=16, batches=batches, frames=frames, spp=spp)
    if other is None:
        a = block_means(lib, scene, "spheres", "uniform", False, mb, **kw)
    else:
        a = block_means(lib, other, "all", pick, True, mb, **kw)
    b = block_means(lib, scene, "all", pick, True, mb, **kw)
    rse = a[1].std(ddof=1) / np.sqrt(len(a[1])) / a[1].mean()
    print(f"{what}: relative standard error of the reference's frame mean {rse:.4f}")
    assert rse <= 0.08
    assert_same_expectation(a, b, what)


def floor_and_ball(triangles=(), quads=(), spheres=()):
    ball = Sphere(vec(0.8, 0.5, -3.0), 0.5, material((0.8, 0.8, 0.8)))
    return scenes.Scene(scenes.camera_07(), [ball] + list(spheres), [scenes._floor()], list(triangles), list(quads))


def test_vertical_two_sided_quad(bwrt_lib):
    """A unit quad standing on edge between two diffuse balls: it emits to both
    sides.  256 frames x 16 batches.  Measured: reference frame error 1.3 %,
    6 lit blocks, max |z| 0.98, rms z 0.70, frame z -0.61."""
    q = quad([(0, 0.5, -3.5), (0, 0.5, -2.5), (0, 1.5, -2.5), (0, 1.5, -3.5)], material((1, 1, 1), 8))
    scene = floor_and_ball(quads=[q], spheres=[Sphere(vec(-0.8, 0.5, -3.0), 0.5, material((0.8, 0.8, 0.8)))])
    finite_and_repeatable(bwrt_lib, scene)
    means_agree(bwrt_lib, scene, "vertical quad")


def test_quad_in_the_floor_plane(bwrt_lib):
    """cos_l = 0 from every floor point (no shadow ray there); the ball above
    is lit.  256 frames x 16 batches.  Measured: reference frame error 0.5 %, 2 lit
    blocks, max |z| 1.11, rms z 1.07, frame z -0.47."""
    q = quad([(-0.5, 0, -3.5), (-0.5, 0, -2.5), (0.5, 0, -2.5), (0.5, 0, -3.5)], material((1, 1, 1), 8))
    scene = floor_and_ball(quads=[q], spheres=[Sphere(vec(0, 1.2, -3.0), 0.5, material((0.8, 0.8, 0.8)))])
    finite_and_repeatable(bwrt_lib, scene)
    means_agree(bwrt_lib, scene, "floor quad")


def test_shading_point_on_the_light(bwrt_lib):
    """The camera looks at the panel from below: most first hits lie on a light
    (prim == its own: unreachable, the other three are sampled in its plane
    with cos_l = 0)."""
    scene = quad_panel()
    cam = scenes.camera_07()
    cam.position = vec(0, 3.0, -4)
    cam.angle[1] = 1.2
    scene.set_camera(cam)
    finite_and_repeatable(bwrt_lib, scene)
    finite_and_repeatable(bwrt_lib, scene, pick="weighted")


def hidden_panel(emittance):
    """A unit quad inside an opaque sphere, and scene 07's orange light."""
    s = scenes._spheres_07()
    q = quad([(1.8, 1, -3.2), (2.2, 1, -3.2), (2.2, 1, -2.8), (1.8, 1, -2.8)], material((1, 1, 1), emittance))
    sph = [s[0], Sphere(vec(2, 1, -3), 0.5, material((0.8, 0.2, 0.2)))] + s[3:]
    return scenes.Scene(scenes.camera_07(), sph, [scenes._floor()], scenes._pyramid(), [q], name="hidden_panel")


def test_polygon_light_hidden_in_an_opaque_sphere(bwrt_lib):
    """Its shadow rays all end on the sphere: the means stay where emittance 0
    (a table without it) has them.  128 frames x 16 batches.  Measured:
    reference frame error 0.6 %, 8 lit blocks, max |z| 3.16, rms z 1.21, frame z -0.05."""
    finite_and_repeatable(bwrt_lib, hidden_panel(50.0))
    with cpu(bwrt_lib, hidden_panel(0.0)) as r:
        assert len(r.lights()) == 1
    means_agree(bwrt_lib, hidden_panel(50.0), "hidden panel", frames=128, other=hidden_panel(0.0))


def test_kind_2_triangle_lit_by_a_polygon(bwrt_lib):
    """tests/test_light_sampling.py's triangle with |n|^2 = 0.64 (the stretched
    cosine) under a quad light.  512 frames x 16 batches.  Measured: reference
    frame error 0.5 %, 7 lit blocks, max |z| 0.82, rms z 0.53, frame z -0.60."""
    a = 0.8 ** 0.5
    t = tri([(-a / 2, 0.6, -0.5), (a / 2, 0.6, -0.5), (-a / 2, 0.6 + a, -0.5)], material((0.8, 0.8, 0.8)))
    q = quad([(0.2, 1.2, 0.5), (1.2, 1.2, 0.5), (1.2, 2.2, 0.5), (0.2, 2.2, 0.5)], material((1, 1, 1), 10))
    scene = scenes.Scene(scenes.camera_07(), [], [scenes._floor()], [t], [q], name="kind2")
    finite_and_repeatable(bwrt_lib, scene, mb=2)
    means_agree(bwrt_lib, scene, "kind-2 triangle", mb=2, frames=512)


def test_non_planar_convex_quad_light(bwrt_lib):
    """v3 lifted off the plane of (v0, v1, v2): what rays hit, and what is
    sampled, is its projection.  256 frames x 16 batches.  Measured:
    reference frame error 0.3 %, 5 lit blocks, max |z| 1.60, rms z 1.15, frame z 1.77."""
    q = quad([(-0.5, 2.5, -3.5), (0.5, 2.5, -3.5), (0.5, 2.5, -2.5), (-0.5, 2.9, -2.5)], material((1, 1, 1), 10))
    scene = floor_and_ball(quads=[q])
    with cpu(bwrt_lib, scene) as r:
        assert len(r.lights()) == 1
    finite_and_repeatable(bwrt_lib, scene)
    means_agree(bwrt_lib, scene, "non-planar quad")


def test_samples_per_pixel(bwrt_lib):
    finite_and_repeatable(bwrt_lib, quad_panel(), spp=3)


def test_table_of_one_polygon(bwrt_lib):
    """n_lights = 1 and W / w == 1: both picks give the same frames.
    256 frames x 16 batches.  Measured: reference frame error 0.2 %, 5
    lit blocks, max |z| 2.23, rms z 1.36, frame z 1.90."""
    t = tri([(-0.5, 2.5, -3.5), (0.5, 2.5, -3.5), (-0.5, 2.5, -2.5)], material((1, 1, 1), 20))
    scene = floor_and_ball(triangles=[t])
    u = finite_and_repeatable(bwrt_lib, scene)
    same_state(u, finite_and_repeatable(bwrt_lib, scene, pick="weighted"))
    means_agree(bwrt_lib, scene, "one triangle")


def forty_quads():
    m = material((1, 0.9, 0.8), 10)
    qs = [quad([(x, 3, z), (x + 1, 3, z), (x + 1, 3, z + 1), (x, 3, z + 1)], m) for x in range(-4, 4) for z in range(-7, -2)]
    return floor_and_ball(quads=qs)


def test_table_of_forty_quads(bwrt_lib):
    with cpu(bwrt_lib, forty_quads()) as r:
        assert len(r.lights()) == 40
    finite_and_repeatable(bwrt_lib, forty_quads())
    finite_and_repeatable(bwrt_lib, forty_quads(), pick="weighted")


# ---- integration ---------------------------------------------------------------------------

@pytest.mark.parametrize("pick", ["uniform", "weighted"])
def test_row_shards_equal_the_full_frame(bwrt_lib, pick):
    with cpu(bwrt_lib, mixed(), "all", pick) as r:
        full = state(r, W0, H0, 3, 4, calls=2)
    for off in (0, 1):
        with cpu(bwrt_lib, mixed(), "all", pick) as r:
            part = state(r, W0, H0, 3, 4, calls=2, row_offset=off, row_stride=2)
        for f, p in zip(full, part):
            assert np.array_equal(f[:, off::2] if f.shape[0] == 6 else f[off::2], p, equal_nan=True)


def snapshots(lib, scene, w, h, bounces, upto):
    have = {}
    with cpu(lib, scene) as u:
        for f in range(1, upto + 1):
            img = u.render(w, h, 1, bounces, first_frame=1 if f == 1 else 0)
            rng, acc = u.get_state(h, w)
            have[f] = (img, rng, acc)
    return have


@pytest.mark.parametrize("make,w,h,bounces", [(quad_panel, 67, 45, 4), (stress_with_emissive_triangles, 48, 27, 4)])
def test_adaptive_replays_uniform_calls(bwrt_lib, make, w, h, bounces):
    """Every pixel after the adaptive calls holds the frameSum, RNG state and
    RGBA of an ALL uniform-call render stopped at its own frame count."""
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_light_sampling(True)
        r.set_light_shapes("all")
        res = adaptive_sequence(r, make(), w, h, bounces)
    assert len(np.unique(res["n"])) > 1
    check_replay(res, snapshots(bwrt_lib, make(), w, h, bounces, int(res["n"].max())))
    with Renderer.cpu(0, lib=bwrt_lib) as r:  # and the sphere-only sequence is another one
        r.set_light_sampling(True)
        sph = adaptive_sequence(r, make(), w, h, bounces)
    assert not np.array_equal(sph["accum"], res["accum"], equal_nan=True)


def test_toggling_inside_one_accumulation(bwrt_lib):
    """The mode resets nothing: spheres, all, spheres over one accumulation
    equals the same calls on contexts that were set once each."""
    w, h = 33, 17
    with cpu(bwrt_lib, mixed(), "spheres") as r:
        r.render(w, h, 2, 4, first_frame=1)
        rng0, acc0 = r.get_state(h, w)
        r.set_light_shapes("all")
        assert r.frame_counter == 3
        same_state(list(r.get_state(h, w)), [rng0, acc0])
        r.render(w, h, 2, 4)
        rng1, acc1 = r.get_state(h, w)
        r.set_light_shapes("spheres")
        r.render(w, h, 2, 4)
        assert r.frame_counter == 7
        toggled = r.get_state(h, w)
    with cpu(bwrt_lib, mixed(), "all") as r:
        r.init_rand(w, h)
        r.set_state(rng0, acc0, 3)
        r.render(w, h, 2, 4)
        same_state(list(r.get_state(h, w)), [rng1, acc1])
    with cpu(bwrt_lib, mixed(), "spheres") as r:
        r.init_rand(w, h)
        r.set_state(rng1, acc1, 5)
        r.render(w, h, 2, 4)
        same_state(list(r.get_state(h, w)), list(toggled))


def test_downstream_passes_run_on_polygon_lit_frames(bwrt_lib):
    w, h = 64, 36
    with cpu(bwrt_lib, quad_panel()) as r:
        r.set_moments(True)
        for i in range(3):
            r.render(w, h, 4, 4, first_frame=1 if i == 0 else 0)
        assert r.moments_batches == 3
        var = r.variance(h, w)
        assert np.isfinite(var).all() and (var > 0).any()
        img, col = r.denoise_var(w, h, want_color=True)
        assert img.shape == (h, w, 4) and np.isfinite(col).all()
        out = r.temporal_var(w, h)
        assert out is not None
        block, frames, batches = r.export_shard(h, w, planes=5)
        assert block.shape == (5, h, w) and (frames, batches) == (12, 3)
        assert np.array_equal(block[:3].transpose(1, 2, 0), r.get_state(h, w)[1])
