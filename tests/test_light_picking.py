"""Weighted light picking of next-event estimation (rt_set_light_picking,
csrc/rt_light.h) on the CPU backend — no GPU needed.  The
HIP kernels compute the same bits (tests/test_gpu_light_picking.py).

What is checked here: the interface; that the mode changes nothing where it
cannot act (light sampling off, empty table, max_bounces 0, one light); that
the path does not depend on the pick (the RNG state); that the weighted pick
has the default estimator's expectation (the z protocol of
tests/test_light_sampling.py) and a smaller variance than the uniform pick; the
geometry cases; shards, adaptive calls, toggling and the downstream passes.
"""
import subprocess

import numpy as np
import pytest

from bwrt import Renderer, abi, scenes
from bwrt.abi import Sphere, Triangle, Vec3
from bwrt.scenes import material, vec
from test_adaptive import check_replay, adaptive_sequence
from test_light_sampling import (CLI, LUM, assert_same_expectation, dark_07, hidden_light_scene, read_ppm, same_state,
                                 state, triangle_light_scene, z_scores)


def cpu(lib, scene, pick="weighted", on=True, threads=0):
    r = Renderer.cpu(threads, lib=lib)
    r.set_scene(scene)
    r.set_light_sampling(on)
    r.set_light_picking(pick)
    return r


def eight_lights():
    """A floor, an occluding sphere and 8 lights of radius 0.2 in a row, whose
    centres are 0.25 .. 4.5 above the floor (18x; their surfaces 0.05 .. 4.3)."""
    ys = [0.25, 0.4, 0.7, 1.0, 1.5, 2.2, 3.2, 4.5]
    cols = [(1, 0.6, 0.2), (1, 0.2, 0.6), (0.2, 0.8, 0.2), (1, 1, 1), (0.3, 0.5, 1), (1, 1, 0.3), (0.6, 0.3, 1), (1, 0.4, 0.4)]
    sph = [Sphere(vec(-3.5 + i, y, -4.0), 0.2, material(c, 10)) for i, (y, c) in enumerate(zip(ys, cols))]
    sph.append(Sphere(vec(0.5, 0.6, -2.8), 0.6, material((0.8, 0.8, 0.8))))  # the occluder
    return scenes.Scene(scenes.camera_07(), sph, [scenes._floor()], [], [], name="eight_lights")


# ---- interface, and where the mode cannot act ---------------------------------------

def test_abi_and_defaults(bwrt_lib):
    names = {"rt_set_light_picking", "rt_get_light_picking"}
    assert names <= set(abi.declared_functions())
    for n in names:
        assert hasattr(bwrt_lib, n)
    assert (abi.RT_LIGHT_PICK_UNIFORM, abi.RT_LIGHT_PICK_WEIGHTED) == (0, 1)
    with Renderer.cpu(1, lib=bwrt_lib) as r:
        assert r.light_picking == "uniform" and bwrt_lib.rt_get_light_picking(r.ctx) == 0
        r.set_light_picking("weighted")
        assert r.light_picking == "weighted" and bwrt_lib.rt_get_light_picking(r.ctx) == 1
        assert r.light_sampling is False  # the two switches are independent
        for bad in (2, -1, 7):
            assert bwrt_lib.rt_set_light_picking(r.ctx, bad) == abi.RT_ERR_INVALID_ARGUMENT
            assert "rt_set_light_picking" in bwrt_lib.rt_last_error(r.ctx).decode()
        assert r.light_picking == "weighted"
        with pytest.raises(ValueError):
            r.set_light_picking("power")
        r.set_light_picking("uniform")
        assert r.light_picking == "uniform"
    # the error of rt_set_light_sampling's bad values
    assert bwrt_lib.rt_set_light_picking(None, 1) == bwrt_lib.rt_set_light_sampling(None, 1) == abi.RT_ERR_INVALID_ARGUMENT
    assert bwrt_lib.rt_get_light_picking(None) == 0


W0, H0 = 67, 45


def test_no_op_with_light_sampling_off(bwrt_lib):
    with cpu(bwrt_lib, scenes.scene_07(), "uniform", on=False) as a, cpu(bwrt_lib, scenes.scene_07(), "weighted", on=False) as b:
        same_state(state(a, W0, H0, 3, 4), state(b, W0, H0, 3, 4))


@pytest.mark.parametrize("make,mb", [(dark_07, 4), (triangle_light_scene, 4), (scenes.scene_07, 0)])
def test_identical_to_the_default_where_nee_cannot_act(bwrt_lib, make, mb):
    with cpu(bwrt_lib, make(), "uniform", on=False) as a, cpu(bwrt_lib, make(), "weighted") as b:
        same_state(state(a, W0, H0, 3, mb), state(b, W0, H0, 3, mb))


def test_one_light_is_uniform_nee(bwrt_lib):
    """W / w_0 == 1 == n_lights exactly; an unreachable light gives 0 either way."""
    with cpu(bwrt_lib, scenes.scene_01(), "uniform") as a, cpu(bwrt_lib, scenes.scene_01(), "weighted") as b:
        same_state(state(a, W0, H0, 3, 4), state(b, W0, H0, 3, 4))
    s = lambda: scenes.Scene(scenes.camera_07(), [scenes._spheres_07()[0]] + scenes._spheres_07()[3:], [scenes._floor()],
                             scenes._pyramid(), [], name="one_light")
    with cpu(bwrt_lib, s(), "uniform") as a, cpu(bwrt_lib, s(), "weighted") as b:
        sa, sb = state(a, W0, H0, 3, 4), state(b, W0, H0, 3, 4)
    same_state(sa, sb)
    with cpu(bwrt_lib, s(), "uniform", on=False) as d:
        assert not np.array_equal(state(d, W0, H0, 3, 4)[1], sa[1])  # and NEE did act


@pytest.mark.parametrize("name,mb", [("07", 4), ("07", 1), ("stress", 4), ("04_box", 3)])
def test_the_path_does_not_depend_on_the_pick(bwrt_lib, name, mb):
    """Same draws, same rays: the RNG state after a weighted render is uniform
    NEE's; frameSum is not (another light, another weight)."""
    with cpu(bwrt_lib, scenes.SCENES[name](), "uniform") as a, cpu(bwrt_lib, scenes.SCENES[name](), "weighted") as b:
        sa, sb = state(a, W0, H0, 3, mb), state(b, W0, H0, 3, mb)
    assert np.array_equal(sa[2], sb[2])
    if name == "07":
        assert not np.array_equal(sa[1], sb[1], equal_nan=True)


# ---- same expectation as the default estimator, smaller variance than uniform NEE ----

W, H, BATCHES, FRAMES = 80, 48, 32, 128


def block_means(lib, scene, pick, on, mb, w=W, h=H, batches=BATCHES, frames=FRAMES, rows=None):
    """tests/test_light_sampling.py's block_means with the pick mode: (batches,
    blocks) luminance means over 8x8 blocks and (batches,) frame means."""
    rows = h if rows is None else rows
    out, whole = [], []
    with cpu(lib, scene, pick, on) as r:
        r.init_rand(w, h)
        for _ in range(batches):
            _, acc = r.render(w, h, frames, mb, first_frame=1, want_accum=True)
            lum = (acc.astype(np.float64) / frames) @ LUM
            whole.append(lum.mean())
            out.append(lum[:rows].reshape(rows // 8, 8, w // 8, 8).mean((1, 3)).ravel())
    return np.array(out), np.array(whole)


CASES = {"07/4": (scenes.scene_07, 4), "07/1": (scenes.scene_07, 1), "eight/4": (eight_lights, 4)}
_RUNS = {}


def runs(lib, case):
    """default, uniform NEE, weighted NEE — computed once per case"""
    if case not in _RUNS:
        make, mb = CASES[case]
        _RUNS[case] = (block_means(lib, make(), "uniform", False, mb), block_means(lib, make(), "uniform", True, mb),
                       block_means(lib, make(), "weighted", True, mb))
    return _RUNS[case]


def test_eight_lights_scene(bwrt_lib):
    with cpu(bwrt_lib, eight_lights()) as r:
        t = r.lights()
    assert len(t) == 8
    y = t["centre"][:, 1]
    assert y.max() >= 10 * y.min()


@pytest.mark.parametrize("case", list(CASES))
def test_same_expectation(bwrt_lib, case):
    """Weighted NEE against the default estimator.  Measured on the CPU backend
    (deterministic): 07 at 4 bounces 34 lit blocks, max |z| 2.22, rms z 1.03,
    frame z -0.27; 07 at 1 bounce 33 lit, 1.68, 0.83, -1.29; the 8-light
    scene 17 lit, 3.10, 1.36, -1.09 (uniform NEE there: 3.46, 1.31, -0.60, and
    weighted against uniform NEE 1.71, 0.89, -0.62: the two picks agree, the
    default estimator's own tails beside the small lights make up the rest)."""
    d, _, wgt = runs(bwrt_lib, case)
    z, zf, lit, ma, sa, sb = z_scores(d, wgt)
    # the test cannot go blind: the default estimator resolves every lit block
    print(f"{case}: default relative standard error at most {(sa[lit] / ma[lit]).max():.3f}")
    assert lit.sum() >= (30 if case.startswith("07") else 15)
    assert (sa[lit] / ma[lit]).max() <= 0.08
    assert_same_expectation(d, wgt, case)


# measured ratio of the summed squared block standard errors over the default
# estimator's lit blocks, weighted over uniform NEE (32 batches of 128 frames,
# 80x48).  Pinned at x 1.25 as section 23's: a variance estimate from 32 batches
# wobbles by about sqrt(2 / 31) = 25 %.
VAR_RATIO = {"07/4": 0.679, "07/1": 0.404, "eight/4": 0.147}


@pytest.mark.parametrize("case", list(CASES))
def test_variance_is_below_uniform_nee(bwrt_lib, case):
    d, uni, wgt = runs(bwrt_lib, case)
    _, _, lit, _, _, su = z_scores(d, uni)
    _, _, _, _, _, sw = z_scores(d, wgt)
    ratio = (sw[lit] ** 2).sum() / (su[lit] ** 2).sum()
    print(f"variance ratio weighted / uniform NEE, {case}: {ratio:.4f}")
    assert ratio < 1.0
    assert ratio <= 1.25 * VAR_RATIO[case]


# ---- geometry cases ------------------------------------------------------------------

GW, GH = 32, 18


def finite_and_repeatable(lib, scene, mb=4, frames=4):
    res = []
    for _ in range(2):
        with cpu(lib, scene) as r:
            res.append(state(r, GW, GH, frames, mb, calls=2))
    same_state(res[0], res[1])
    assert np.isfinite(res[0][-1]).all()
    return res[0]


def test_camera_inside_a_light(bwrt_lib):
    scene = scenes.scene_07()
    cam = scenes.camera_07()
    cam.position = vec(-6, 3, -4)  # the centre of light 0
    scene.set_camera(cam)
    finite_and_repeatable(bwrt_lib, scene)


def test_light_touching_the_floor(bwrt_lib):
    scene = scenes.scene_07()  # the green light: centre y 0.2, radius 0.2 — s2 reaches 1 beside it
    cam = scenes.camera_07()
    cam.position = vec(-0.5, 0.3, -2.0)
    scene.set_camera(cam)
    finite_and_repeatable(bwrt_lib, scene)


def test_light_buried_in_an_opaque_sphere(bwrt_lib):
    """W > 0 includes the hidden light's weight, but its shadow rays all end on
    the red sphere: the means stay where its emittance 0 (three entries) puts
    them.  Measured: 7 lit blocks, max |z| 0.69, rms z 0.42, frame z -0.02."""
    kw = dict(w=GW, h=GH, rows=16, batches=16, frames=128)
    finite_and_repeatable(bwrt_lib, hidden_light_scene(50.0))
    a = block_means(bwrt_lib, hidden_light_scene(0.0), "weighted", True, 4, **kw)
    b = block_means(bwrt_lib, hidden_light_scene(50.0), "weighted", True, 4, **kw)
    assert_same_expectation(a, b, "buried light")


def black_light_scene(emittance):
    """Scene 07's orange light and geometry, and before it in the table a
    zero-albedo sphere of the given emittance: emitted = emittance * 0."""
    s = scenes._spheres_07()
    sph = [Sphere(vec(2, 1, -3), 0.5, material((0, 0, 0), emittance)), s[0]] + s[3:]
    return scenes.Scene(scenes.camera_07(), sph, [scenes._floor()], scenes._pyramid(), [], name="black_light")


def test_zero_albedo_light_is_never_picked(bwrt_lib):
    """pw = 0: every pick goes to the other light with W / w == 1, so frameSum
    is that of uniform NEE on the scene whose table has the other light alone
    (uniform NEE on the two-entry table spends half its picks on the black one)."""
    with cpu(bwrt_lib, black_light_scene(5.0)) as r:
        assert len(r.lights()) == 2 and not r.lights()["emitted"][0].any()
    two = finite_and_repeatable(bwrt_lib, black_light_scene(5.0))
    with cpu(bwrt_lib, black_light_scene(0.0), "uniform") as r:
        assert len(r.lights()) == 1
        one = state(r, GW, GH, 4, 4, calls=2)
    same_state(two, one)
    with cpu(bwrt_lib, black_light_scene(5.0), "uniform") as r:
        assert not np.array_equal(state(r, GW, GH, 4, 4, calls=2)[-1], two[-1])


def small_normal_scene():
    """tests/test_light_sampling.py's triangle with |n|^2 = 0.64 (kind 2: nl =
    0.8 in the cosine bound) over the floor, lit by two spheres of unequal
    share so that the pick has a choice."""
    a = 0.8 ** 0.5
    tri = Triangle((Vec3 * 3)(vec(-a / 2, 0.6, -0.5), vec(a / 2, 0.6, -0.5), vec(-a / 2, 0.6 + a, -0.5)),
                   material((0.8, 0.8, 0.8)))
    lights = [Sphere(vec(0.6, 1.0, 0.3), 0.2, material((1, 1, 1), 20)), Sphere(vec(-1.5, 2.5, 1.0), 0.3, material((1, 0.5, 0.2), 10))]
    return scenes.Scene(scenes.camera_07(), lights, [scenes._floor()], [tri], [], name="small_normal_two_lights")


def test_non_unit_normals_keep_the_expectation(bwrt_lib):
    """Measured: 7 lit blocks, max |z| 1.24, rms z 0.84, frame z 1.29."""
    finite_and_repeatable(bwrt_lib, small_normal_scene(), mb=2)
    kw = dict(w=GW, h=GH, rows=16, batches=16, frames=512)
    a = block_means(bwrt_lib, small_normal_scene(), "uniform", False, 2, **kw)
    b = block_means(bwrt_lib, small_normal_scene(), "weighted", True, 2, **kw)
    z, zf, lit, ma, sa, sb = z_scores(a, b)
    assert lit.sum() >= 2 and (sa[lit] / ma[lit]).max() <= 0.08
    assert_same_expectation(a, b, "small normal")


def test_only_light_unreachable_from_most_hits(bwrt_lib):
    """The W = 0 branch: one big light fills the view, so most hits lie on it
    (prim == its own).  No direct term, no shadow ray, a valid j in the record:
    the render is uniform NEE's, which returns at the same place."""
    def make():
        return scenes.Scene(scenes.camera_07(), [Sphere(vec(0, 1, -3), 2.5, material((1, 0.9, 0.8), 2))], [scenes._floor()],
                            [], [], name="big_light")
    got = finite_and_repeatable(bwrt_lib, make())
    with cpu(bwrt_lib, make(), "uniform") as r:
        same_state(got, state(r, GW, GH, 4, 4, calls=2))


# ---- composition -----------------------------------------------------------------------

def test_row_shards_equal_the_full_frame(bwrt_lib):
    with cpu(bwrt_lib, scenes.scene_07()) as r:
        full = state(r, W0, H0, 3, 4, calls=2)
    for off in (0, 1):
        with cpu(bwrt_lib, scenes.scene_07()) as r:
            part = state(r, W0, H0, 3, 4, calls=2, row_offset=off, row_stride=2)
        for f, p in zip(full, part):
            assert np.array_equal(f[:, off::2] if f.shape[0] == 6 else f[off::2], p, equal_nan=True)


def weighted_snapshots(lib, name, w, h, bounces, upto):
    have = {}
    with cpu(lib, scenes.SCENES[name]()) as u:
        for f in range(1, upto + 1):
            img = u.render(w, h, 1, bounces, first_frame=1 if f == 1 else 0)
            rng, acc = u.get_state(h, w)
            have[f] = (img, rng, acc)
    return have


@pytest.mark.parametrize("name,w,h,bounces", [("07", 67, 45, 4), ("stress", 48, 27, 4)])
def test_adaptive_replays_uniform_calls(bwrt_lib, name, w, h, bounces):
    """Every pixel after the adaptive calls holds the frameSum, RNG state and
    RGBA of a weighted uniform-call render stopped at its own frame count."""
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_light_sampling(True)
        r.set_light_picking("weighted")
        res = adaptive_sequence(r, scenes.SCENES[name](), w, h, bounces)
    assert len(np.unique(res["n"])) > 1
    check_replay(res, weighted_snapshots(bwrt_lib, name, w, h, bounces, int(res["n"].max())))
    with Renderer.cpu(0, lib=bwrt_lib) as r:  # and uniform NEE's sequence is another one
        r.set_light_sampling(True)
        uni = adaptive_sequence(r, scenes.SCENES[name](), w, h, bounces)
    assert not np.array_equal(uni["accum"], res["accum"], equal_nan=True)


def test_toggling_inside_one_accumulation(bwrt_lib):
    """The mode resets nothing: uniform, weighted, uniform over one accumulation
    equals the same calls on contexts that were set once each."""
    w, h = 33, 17
    with cpu(bwrt_lib, scenes.scene_07(), "uniform") as r:
        r.render(w, h, 2, 4, first_frame=1)
        rng0, acc0 = r.get_state(h, w)
        r.set_light_picking("weighted")
        assert r.frame_counter == 3
        same_state(list(r.get_state(h, w)), [rng0, acc0])
        r.render(w, h, 2, 4)
        rng1, acc1 = r.get_state(h, w)
        r.set_light_picking("uniform")
        r.render(w, h, 2, 4)
        assert r.frame_counter == 7
        mixed = r.get_state(h, w)
    with cpu(bwrt_lib, scenes.scene_07(), "weighted") as r:
        r.init_rand(w, h)
        r.set_state(rng0, acc0, 3)
        r.render(w, h, 2, 4)
        same_state(list(r.get_state(h, w)), [rng1, acc1])
    with cpu(bwrt_lib, scenes.scene_07(), "uniform") as r:
        r.init_rand(w, h)
        r.set_state(rng1, acc1, 5)
        r.render(w, h, 2, 4)
        same_state(list(r.get_state(h, w)), list(mixed))


def test_downstream_passes_run_on_weighted_frames(bwrt_lib):
    w, h = 64, 36
    with cpu(bwrt_lib, scenes.scene_07()) as r:
        r.set_moments(True)
        for i in range(3):
            r.render(w, h, 4, 4, first_frame=1 if i == 0 else 0)
        assert r.moments_batches == 3
        var = r.variance(h, w)
        assert np.isfinite(var).all() and (var > 0).any()
        img, col = r.denoise_var(w, h, want_color=True)
        assert img.shape == (h, w, 4) and np.isfinite(col).all()
        block, frames, batches = r.export_shard(h, w, planes=5)
        assert block.shape == (5, h, w) and (frames, batches) == (12, 3)
        assert np.array_equal(block[:3].transpose(1, 2, 0), r.get_state(h, w)[1])


def test_cli_flag_matches_python(bwrt_lib, tmp_path):
    def run(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)

    assert "--light-picking" in run("--help").stdout
    r = run("--light-picking", "weighted")
    assert r.returncode == 2 and "--light-sampling" in r.stderr
    r = run("--light-sampling", "--light-picking", "power")
    assert r.returncode == 2 and "--light-picking" in r.stderr
    w, h = 64, 36
    common = ("--cpu", "2", "--scene", "07", "--width", str(w), "--height", str(h), "--frames", "3", "--max-bounces", "4",
              "--light-sampling")
    imgs = {}
    for pick in ("uniform", "weighted"):
        out = tmp_path / f"{pick}.ppm"
        r = run(*common, "--light-picking", pick, "--out", str(out))
        assert r.returncode == 0, r.stderr
        imgs[pick] = read_ppm(out)
        with cpu(bwrt_lib, scenes.scene_07(), pick, threads=2) as p:
            img = None
            for f in range(3):  # the CLI renders --frames-per-call 1
                img = p.render(w, h, 1, 4, first_frame=1 if f == 0 else 0)
        assert np.array_equal(imgs[pick], img[..., :3]), pick
    assert not np.array_equal(imgs["uniform"], imgs["weighted"])
