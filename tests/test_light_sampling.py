"""Next-event estimation (rt_set_light_sampling, csrc/rt_light.h; DESIGN.md
section 23) on the CPU backend — no GPU needed.  The HIP kernel computes the
same bits (tests/test_gpu_light_sampling.py compares it with this backend).

What is checked here: the ABI and the light table; that the estimator IS the
default one, bit for bit, wherever it cannot act (empty table, max_bounces 0);
that it has the default estimator's expectation (z scores over batch means) and
a smaller variance; the geometry cases; shards, adaptive calls and the
downstream passes on its frames; the error contract.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bwrt import Renderer, abi, scenes
from bwrt.abi import Sphere, Triangle, Vec3
from bwrt.scenes import material, vec
from test_adaptive import check_replay, adaptive_sequence

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd", "bin",
                   "bwrt_render")
LUM = np.array([0.2126, 0.7152, 0.0722])  # rt_moments.h


def cpu(lib, scene, on=True, threads=0):
    r = Renderer.cpu(threads, lib=lib)
    r.set_scene(scene)
    r.set_light_sampling(on)
    return r


def dark_07():
    s = scenes.scene_07()
    for i in range(s.counts[0]):
        s.spheres[i].mat.emittance = 0.0
    return s


def triangle_light_scene():
    """Scene 07's geometry lit by an emissive triangle alone."""
    s = dark_07()
    tri = Triangle((Vec3 * 3)(vec(-3, 4, -6), vec(3, 4, -6), vec(0, 4, -2)), material((1, 1, 1), 15))
    return scenes.Scene(s.camera, list(s.spheres)[:s.counts[0]], list(s.planes)[:1],
                        list(s.triangles)[:s.counts[2]] + [tri], [], name="triangle_light")


def state(r, w, h, frames=3, mb=4, calls=1, **kw):
    out = []
    for i in range(calls):
        img, acc = r.render(w, h, frames, mb, first_frame=1 if i == 0 else 0, want_accum=True, **kw)
        out.append(img)
        out.append(acc)
    rows = acc.shape[0]
    rng, acc2 = r.get_state(rows, w)
    return out + [rng, acc2]


def same_state(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


# ---- ABI and light table ---------------------------------------------------------

def test_abi_and_defaults(bwrt_lib):
    names = {"rt_set_light_sampling", "rt_get_light_sampling", "rt_get_lights"}
    assert names <= set(abi.declared_functions())
    for n in names:
        assert hasattr(bwrt_lib, n)
    assert abi.RT_LIGHT_RECORD_FLOATS == 8
    with Renderer.cpu(1, lib=bwrt_lib) as r:
        assert r.light_sampling is False
        assert bwrt_lib.rt_get_lights(r.ctx, None, 0) == abi.RT_ERR_NO_SCENE
        r.set_light_sampling(True)
        assert r.light_sampling is True and bwrt_lib.rt_get_light_sampling(r.ctx) == 1
        r.set_light_sampling(0)
        assert r.light_sampling is False
        for bad in (2, -1, 7):
            assert bwrt_lib.rt_set_light_sampling(r.ctx, bad) == abi.RT_ERR_INVALID_ARGUMENT
        assert r.light_sampling is False
    assert bwrt_lib.rt_set_light_sampling(None, 1) == abi.RT_ERR_INVALID_ARGUMENT
    assert bwrt_lib.rt_get_light_sampling(None) == 0


def expected_table(scene):
    rows = []
    for i in range(scene.counts[0]):
        sp = scene.spheres[i]
        e, r = np.float32(sp.mat.emittance), np.float32(sp.radius)
        if np.isfinite(e) and e > 0 and np.isfinite(r) and r > 0:
            alb = np.array([sp.mat.albedo.x, sp.mat.albedo.y, sp.mat.albedo.z], np.float32)
            rows.append(((sp.position.x, sp.position.y, sp.position.z), r * r, e * alb, i))
    return rows


@pytest.mark.parametrize("name,count", [("07", 3), ("stress", 8), ("04_box", 2), ("01", 1), ("empty", 0)])
def test_light_table(bwrt_lib, name, count):
    scene = scenes.SCENES[name]()
    with cpu(bwrt_lib, scene, on=False) as r:
        got = r.lights()
        want = expected_table(scene)
        assert len(got) == count == len(want)
        for g, (c, r2, e, prim) in zip(got, want):
            assert np.array_equal(g["centre"], np.array(c, np.float32))
            assert g["r2"] == np.float32(r2) and g["prim"] == prim
            assert np.array_equal(g["emitted"], e.astype(np.float32))
        # capacity clips the copy, not the count
        raw = np.full((2, 8), -1.0, np.float32)
        n = bwrt_lib.rt_get_lights(r.ctx, raw.ctypes.data_as(C.POINTER(C.c_float)), 1)
        assert n == count
        assert np.all(raw[1] == -1.0) and (count == 0 or raw[0, 3] == got[0]["r2"])


def test_light_table_exclusions(bwrt_lib):
    scene = scenes.scene_07()
    scene.spheres[2].mat.emittance = float("inf")   # the guard scene's light
    scene.spheres[0].mat.emittance = float("nan")
    scene.spheres[3].mat.emittance = -1.0
    with cpu(bwrt_lib, scene) as r:
        assert [int(p) for p in r.lights()["prim"]] == [1]
        scene.spheres[1].radius = 0.0
        r.set_scene(scene)
        assert len(r.lights()) == 0
    with cpu(bwrt_lib, triangle_light_scene()) as r:
        assert len(r.lights()) == 0


# ---- bit identity with the default estimator -------------------------------------

@pytest.mark.parametrize("make,mb", [(dark_07, 4), (triangle_light_scene, 4), (scenes.scene_07, 0)])
def test_identical_where_it_cannot_act(bwrt_lib, make, mb):
    w, h = 67, 45
    with cpu(bwrt_lib, make(), on=False) as a, cpu(bwrt_lib, make(), on=True) as b:
        same_state(state(a, w, h, 3, mb), state(b, w, h, 3, mb))


def test_differs_where_it_acts(bwrt_lib):
    w, h = 67, 45
    with cpu(bwrt_lib, scenes.scene_07(), on=False) as a, cpu(bwrt_lib, scenes.scene_07(), on=True) as b:
        sa, sb = state(a, w, h, 3, 4), state(b, w, h, 3, 4)
    assert not np.array_equal(sa[1], sb[1], equal_nan=True)
    assert not np.array_equal(sa[2], sb[2])


def test_toggling_keeps_the_accumulation(bwrt_lib):
    """The switch resets nothing: off, on, off over one accumulation equals the
    same three calls on contexts that were set once each."""
    w, h = 33, 17
    with cpu(bwrt_lib, scenes.scene_07(), on=False) as r:
        r.render(w, h, 2, 4, first_frame=1)
        rng0, acc0 = r.get_state(h, w)
        r.set_light_sampling(True)
        assert r.frame_counter == 3
        rng1, acc1 = r.get_state(h, w)
        assert np.array_equal(rng0, rng1) and np.array_equal(acc0, acc1)
        r.render(w, h, 2, 4)
        assert r.frame_counter == 5
        mixed = r.get_state(h, w)
    with cpu(bwrt_lib, scenes.scene_07(), on=True) as r:
        r.init_rand(w, h)
        r.set_state(rng0, acc0, 3)
        r.render(w, h, 2, 4)
        want = r.get_state(h, w)
    same_state(mixed, want)


# ---- same expectation, smaller variance -------------------------------------------

W, H, BATCHES, FRAMES = 80, 48, 32, 128


def block_means(lib, scene, on, mb, w=W, h=H, batches=BATCHES, frames=FRAMES, rows=None):
    """(batches, blocks) luminance means over 8x8 blocks and (batches,) frame
    means; every batch starts at frame 1, the context is seeded once."""
    rows = h if rows is None else rows
    out, whole = [], []
    with cpu(lib, scene, on) as r:
        r.init_rand(w, h)
        for _ in range(batches):
            _, acc = r.render(w, h, frames, mb, first_frame=1, want_accum=True)
            lum = (acc.astype(np.float64) / frames) @ LUM
            whole.append(lum.mean())
            out.append(lum[:rows].reshape(rows // 8, 8, w // 8, 8).mean((1, 3)).ravel())
    return np.array(out), np.array(whole)


def z_scores(a, b):
    """z of the block means of b against a, the lit blocks of a, and the
    standard errors; a, b: (blocks means, frame means) of block_means."""
    (ba, fa), (bb, fb) = a, b
    ma, mb_ = ba.mean(0), bb.mean(0)
    sa, sb = ba.std(0, ddof=1) / np.sqrt(len(ba)), bb.std(0, ddof=1) / np.sqrt(len(bb))
    lit = ma > 0.05 * ma.max()
    z = (mb_[lit] - ma[lit]) / np.sqrt(sa[lit] ** 2 + sb[lit] ** 2)
    zf = (fb.mean() - fa.mean()) / np.sqrt(fa.var(ddof=1) / len(fa) + fb.var(ddof=1) / len(fb))
    return z, zf, lit, ma, sa, sb


def assert_same_expectation(a, b, what):
    z, zf, lit, *_ = z_scores(a, b)
    print(f"{what}: lit {int(lit.sum())}, max|z| {np.abs(z).max():.2f}, rms z {np.sqrt((z ** 2).mean()):.2f}, "
          f"frame z {zf:.2f}")
    assert np.abs(z).max() <= 5.0, what
    assert np.sqrt((z ** 2).mean()) <= 1.5, what
    assert abs(zf) <= 4.0, what


_RUNS = {}


def runs_07(lib, mb):
    if mb not in _RUNS:
        _RUNS[mb] = (block_means(lib, scenes.scene_07(), False, mb), block_means(lib, scenes.scene_07(), True, mb))
    return _RUNS[mb]


@pytest.mark.parametrize("mb", [4, 1])
def test_same_expectation(bwrt_lib, mb):
    """Measured on the CPU backend: at 4 bounces 34 lit blocks, max |z| 2.23,
    rms z 1.04, frame z -0.35; at 1 bounce 33 lit blocks, max |z| 1.66, rms z
    0.86, frame z -1.29 (default relative standard error at most 6.2 % and
    3.5 %).  Deterministic.  The pyramid's block is what a direct term that
    ignores its faces' un-normalised normals moves by 5 %, |z| 6.5."""
    d, n = runs_07(bwrt_lib, mb)
    z, zf, lit, ma, sa, sb = z_scores(d, n)
    # the test cannot go blind: the default estimator resolves every lit block
    assert lit.sum() >= 30
    assert (sa[lit] / ma[lit]).max() <= 0.08
    assert_same_expectation(d, n, f"07 at {mb} bounces")


# measured ratio of the summed squared block standard errors over the lit
# blocks, NEE over default (32 batches of 128 frames, 80x48): 0.136 at 4
# bounces, 0.108 at 1.  Pinned at x 1.25: a variance estimate from 32 batches
# wobbles by about sqrt(2 / 31) = 25 %.
VAR_RATIO = {4: 0.136, 1: 0.108}


@pytest.mark.parametrize("mb", [4, 1])
def test_variance_is_smaller(bwrt_lib, mb):
    d, n = runs_07(bwrt_lib, mb)
    _, _, lit, _, sa, sb = z_scores(d, n)
    ratio = (sb[lit] ** 2).sum() / (sa[lit] ** 2).sum()
    print(f"variance ratio at {mb} bounces: {ratio:.4f}")
    assert ratio < 1.0
    assert ratio <= 1.25 * VAR_RATIO[mb]


# ---- geometry cases ----------------------------------------------------------------

GW, GH = 32, 18


def finite_and_repeatable(lib, scene, mb=4, frames=4, spp=1, want_finite=True):
    res = []
    for _ in range(2):
        with cpu(lib, scene) as r:
            r.set_samples_per_pixel(spp)
            res.append(state(r, GW, GH, frames, mb, calls=2))
    same_state(res[0], res[1])
    if want_finite:
        assert np.isfinite(res[0][-1]).all()
    return res[0]


def test_camera_inside_a_light(bwrt_lib):
    scene = scenes.scene_07()
    cam = scenes.camera_07()
    cam.position = vec(-6, 3, -4)  # the centre of light 0: every P is unreachable for it
    scene.set_camera(cam)
    finite_and_repeatable(bwrt_lib, scene)


def test_light_touching_the_floor(bwrt_lib):
    scene = scenes.scene_07()  # the green light: centre y 0.2, radius 0.2
    cam = scenes.camera_07()
    cam.position = vec(-0.5, 0.3, -2.0)
    scene.set_camera(cam)
    finite_and_repeatable(bwrt_lib, scene)


@pytest.mark.parametrize("name,count", [("01", 1), ("stress", 8)])
def test_light_counts(bwrt_lib, name, count):
    scene = scenes.SCENES[name]()
    with cpu(bwrt_lib, scene) as r:
        assert len(r.lights()) == count
    finite_and_repeatable(bwrt_lib, scene)


def test_samples_per_pixel(bwrt_lib):
    res = finite_and_repeatable(bwrt_lib, scenes.scene_07(), spp=3)
    one = finite_and_repeatable(bwrt_lib, scenes.scene_07(), spp=1)
    assert not np.array_equal(res[-1], one[-1])


def hidden_light_scene(emittance):
    """Scene 07 with a fourth light in the middle of its big red sphere (radius
    2): from outside that sphere the light is fully behind it."""
    s = scenes.scene_07()
    sph = list(s.spheres)[:s.counts[0]] + [Sphere(vec(4, 2, -8), 0.5, material((1, 1, 1), emittance))]
    return scenes.Scene(s.camera, sph, list(s.planes)[:1], list(s.triangles)[:s.counts[2]], [], name="hidden_light")


def test_light_behind_an_occluder(bwrt_lib):
    """Every block is shadowed from the hidden light: its presence (a fourth
    table entry, a quarter of the picks, shadow rays that all end on the red
    sphere) leaves the expectation where its emittance 0 (three entries) has
    it.  Measured: 7 lit blocks, max |z| 0.99, rms z 0.53, frame z 0.96."""
    kw = dict(w=GW, h=GH, rows=16, batches=16, frames=128)
    with cpu(bwrt_lib, hidden_light_scene(50.0)) as r:
        assert len(r.lights()) == 4
    a = block_means(bwrt_lib, hidden_light_scene(0.0), True, 4, **kw)
    b = block_means(bwrt_lib, hidden_light_scene(50.0), True, 4, **kw)
    assert_same_expectation(a, b, "hidden light")


def small_normal_scene():
    """A triangle whose un-normalised normal has length 0.8 (|n|^2 = 0.64: the
    flip of random_direction stretches by g = 0.28) in front of the camera, lit
    by one sphere beside the camera, over the floor."""
    a = 0.8 ** 0.5
    tri = Triangle((Vec3 * 3)(vec(-a / 2, 0.6, -0.5), vec(a / 2, 0.6, -0.5), vec(-a / 2, 0.6 + a, -0.5)),
                   material((0.8, 0.8, 0.8)))
    light = Sphere(vec(0.6, 1.0, 0.3), 0.2, material((1, 1, 1), 20))
    return scenes.Scene(scenes.camera_07(), [light], [scenes._floor()], [tri], [], name="small_normal")


def test_non_unit_normals_keep_the_expectation(bwrt_lib):
    """The default estimator on a polygon is not a uniform-hemisphere one
    (rt_light.h "Non-unit normals"); the direct term follows it.  Measured: 7
    lit blocks, max |z| 1.36, rms z 0.84, frame z 1.01."""
    kw = dict(w=GW, h=GH, rows=16, batches=16, frames=512)
    a = block_means(bwrt_lib, small_normal_scene(), False, 2, **kw)
    b = block_means(bwrt_lib, small_normal_scene(), True, 2, **kw)
    z, zf, lit, ma, sa, sb = z_scores(a, b)
    assert lit.sum() >= 2 and (sa[lit] / ma[lit]).max() <= 0.08
    assert_same_expectation(a, b, "small normal")


# ---- shards and adaptive -------------------------------------------------------------

def test_row_shards_equal_the_full_frame(bwrt_lib):
    w, h = 67, 45
    with cpu(bwrt_lib, scenes.scene_07()) as r:
        full = state(r, w, h, 3, 4, calls=2)
    for off in (0, 1):
        with cpu(bwrt_lib, scenes.scene_07()) as r:
            part = state(r, w, h, 3, 4, calls=2, row_offset=off, row_stride=2)
        for f, p in zip(full, part):
            assert np.array_equal(f[:, off::2] if f.shape[0] == 6 else f[off::2], p, equal_nan=True)


_SNAPS = {}


def nee_snapshots(lib, name, w, h, bounces, upto):
    key = (name, w, h, bounces)
    have = _SNAPS.get(key)
    if have is None or max(have) < upto:
        have = {}
        with cpu(lib, scenes.SCENES[name]()) as u:
            for f in range(1, upto + 1):
                img = u.render(w, h, 1, bounces, first_frame=1 if f == 1 else 0)
                rng, acc = u.get_state(h, w)
                have[f] = (img, rng, acc)
        _SNAPS[key] = have
    return have


@pytest.mark.parametrize("name,w,h,bounces", [("07", 67, 45, 4), ("stress", 48, 27, 4)])
def test_adaptive_replays_uniform_nee(bwrt_lib, name, w, h, bounces):
    """Every pixel after the adaptive calls holds the frameSum, RNG state and
    RGBA of a uniform NEE render stopped at its own frame count."""
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_light_sampling(True)
        res = adaptive_sequence(r, scenes.SCENES[name](), w, h, bounces)
    assert len(np.unique(res["n"])) > 1
    check_replay(res, nee_snapshots(bwrt_lib, name, w, h, bounces, int(res["n"].max())))
    # and the default estimator's sequence is another one
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        off = adaptive_sequence(r, scenes.SCENES[name](), w, h, bounces)
    assert not np.array_equal(off["accum"], res["accum"], equal_nan=True)


# ---- downstream passes -----------------------------------------------------------------

def test_downstream_passes_run_on_nee_frames(bwrt_lib):
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
        out = r.temporal_var(w, h, want_color=True)
        assert np.isfinite(out[1]).all()
        block, frames, batches = r.export_shard(h, w, planes=5)
        assert block.shape == (5, h, w) and (frames, batches) == (12, 3)
        assert np.array_equal(block[:3].transpose(1, 2, 0), r.get_state(h, w)[1])


# ---- errors ------------------------------------------------------------------------------

def test_bad_values_touch_nothing(bwrt_lib):
    w, h = 33, 17
    with cpu(bwrt_lib, scenes.scene_07()) as r:
        r.render(w, h, 2, 4, first_frame=1)
        before = r.get_state(h, w)
        assert bwrt_lib.rt_set_light_sampling(r.ctx, 3) == abi.RT_ERR_INVALID_ARGUMENT
        assert "neither 0 nor 1" in bwrt_lib.rt_last_error(r.ctx).decode()
        assert r.light_sampling is True and r.frame_counter == 3
        same_state(before, r.get_state(h, w))
        # a CPU context has no fast mode to combine with
        assert bwrt_lib.rt_set_precision(r.ctx, abi.RT_PRECISION_REFERENCE_FAST) == abi.RT_ERR_UNSUPPORTED


def read_ppm(path):
    data = open(path, "rb").read()
    parts = data.split(None, 4)
    assert parts[0] == b"P6"
    w, h = int(parts[1]), int(parts[2])
    return np.frombuffer(parts[4][-w * h * 3:], np.uint8).reshape(h, w, 3)[::-1]  # the file's rows are flipped


def test_cli_flag_matches_python(bwrt_lib, tmp_path):
    def run(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)

    assert "--light-sampling" in run("--help").stdout
    r = run("--light-sampling", "--precision", "fast")
    assert r.returncode == 2 and "--precision fast" in r.stderr
    w, h = 64, 36
    common = ("--cpu", "2", "--scene", "07", "--width", str(w), "--height", str(h), "--frames", "3", "--max-bounces", "4")
    imgs = {}
    for flag in ((), ("--light-sampling",)):
        out = tmp_path / f"img{len(flag)}.ppm"
        r = run(*common, *flag, "--out", str(out))
        assert r.returncode == 0, r.stderr
        imgs[bool(flag)] = read_ppm(out)
    for on in (False, True):
        with cpu(bwrt_lib, scenes.scene_07(), on=on, threads=2) as p:
            img = None
            for f in range(3):  # the CLI renders --frames-per-call 1
                img = p.render(w, h, 1, 4, first_frame=1 if f == 0 else 0)
        assert np.array_equal(imgs[on], img[..., :3]), on
    assert not np.array_equal(imgs[False], imgs[True])
