"""First-hit feature buffers (rt_render_aov) and the a-trous denoiser
(rt_denoise) on the CPU backend — no GPU needed.  The GPU kernels compute the
same bits (tests/test_gpu_denoise.py compares them with this backend).

The float64 reference is tests/denoise_ref.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
from bwrt import Renderer, abi, scenes
from bwrt.abi import Camera, Plane, Sphere, Vec3

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd", "bin",
                   "bwrt_render")

# max |colour - float64 reference| / (1 + |reference|).  Measured on the CPU
# backend over the cases of test_filter_against_float64 (scene 07, 67x45, 4
# frames, levels 1..6): 2.95e-6 (float32 rounding of sums of up to 25 taps, of
# the guides and of exp_nn, through up to six levels).  Asserted at 8x: room
# for another compiler's float64 libm and for the reference's own error, while
# one wrong tap of weight 1/256 on this frame (colour range ~20) moves a pixel
# by ~1e-2.
FILTER_BOUND = 8 * 2.95e-6


@pytest.fixture(scope="module")
def cpu(bwrt_lib):
    r = Renderer.cpu(0, lib=bwrt_lib)
    yield r
    r.close()


def guides(r, scene, w, h):
    a = r.render_aov(w, h)
    return a, R.hit_points(scene.camera, w, h, a["depth"], a["prim"])


def reference(r, scene, w, h, acc, n, **kw):
    d = r.denoise_params(**kw)
    a, P = guides(r, scene, w, h)
    return R.denoise_ref(acc, n, a["normal"], P, a["prim"], d.iterations, d.sigma_color, d.sigma_normal,
                         d.sigma_plane)


def rgba_within_1lsb(got, ref_color):
    ref = R.tone_map(ref_color)
    return int(np.abs(got.astype(np.int32) - ref.astype(np.int32)).max()) <= 1


@pytest.fixture(scope="module")
def frame07(cpu):
    """Scene 07, 67x45, 4 frames, 4 bounces: (scene, w, h, rgba, frameSum)."""
    scene = scenes.scene_07()
    w, h = 67, 45
    cpu.set_scene(scene)
    img, acc = cpu.render(w, h, 4, 4, first_frame=1, want_accum=True)
    return scene, w, h, img, acc


def test_abi_declares_the_entry_points(bwrt_lib):
    assert {"rt_render_aov", "rt_denoise", "rt_denoise_device", "rt_denoise_params_default",
            "rt_last_denoise_ms"} <= set(abi.declared_functions())
    d = bwrt_lib.rt_denoise_params_default()
    assert d.iterations == 5 and d.sigma_color > 0 and d.sigma_normal > 0 and d.sigma_plane > 0


# ---- feature buffers ---------------------------------------------------------
def test_analytic_features(bwrt_lib):
    cam = Camera(scenes.vec(0, 0, 0), (C.c_float * 2)(0.0, 0.0), float(scenes.PI / np.float32(2)))
    alb = (0.25, 0.5, 0.75)
    scene = scenes.Scene(cam, [Sphere(scenes.vec(0, 0, -5), 1.0, scenes.material(alb, 2.0))])
    w, h = 65, 33
    with Renderer.cpu(2, lib=bwrt_lib) as r:
        r.set_scene(scene)
        r.set_background(0.125, 0.25, 0.5)
        a = r.render_aov(w, h)
    cy, cx = h // 2, w // 2
    assert a["prim"][cy, cx] == 0
    assert a["depth"][cy, cx] == 4.0
    assert a["normal"][cy, cx].tolist() == [0.0, 0.0, 1.0]
    assert a["albedo"][cy, cx].tolist() == list(alb)
    for y, x in ((0, 0), (h - 1, w - 1)):
        assert a["prim"][y, x] == -1
        assert a["depth"][y, x] == np.inf
        assert a["normal"][y, x].tolist() == [0.0, 0.0, 0.0]
        assert a["albedo"][y, x].tolist() == [0.125, 0.25, 0.5]


def feature_scene():
    cam = Camera(scenes.vec(0.3, 1.2, 0.5), (C.c_float * 2)(0.2, -0.15), 1.3)
    m = scenes.material
    sph = [Sphere(scenes.vec(-1.5, 1.0, -5), 1.0, m((0.9, 0.2, 0.1))),
           Sphere(scenes.vec(0.5, 0.6, -3.5), 0.6, m((0.1, 0.8, 0.3))),
           Sphere(scenes.vec(2.5, 1.5, -7), 1.5, m((0.2, 0.3, 0.9)))]
    floor = Plane(scenes.vec(0, 0, 0), (Vec3 * 2)(scenes.vec(0, 0, 2), scenes.vec(1.5, 0, 0)), m((0.5, 0.5, 0.5)))
    return scenes.Scene(cam, sph, [floor])


def test_features_against_float64(cpu):
    scene = feature_scene()
    w, h = 64, 36
    cpu.set_scene(scene)
    a = cpu.render_aov(w, h)
    prim, depth, normal = R.first_hit(scene, w, h)
    ambiguous = np.zeros((h, w), bool)
    for dx, dy in ((0.05, 0.05), (-0.05, 0.05), (0.05, -0.05), (-0.05, -0.05)):
        ambiguous |= R.first_hit(scene, w, h, dx=dx, dy=dy)[0] != prim
    assert ambiguous.mean() <= 0.05
    assert len(np.unique(prim[~ambiguous])) == 5  # three spheres, the plane, the sky
    ok = ~ambiguous
    assert np.array_equal(a["prim"][ok], prim[ok])
    hit = ok & (prim >= 0)
    assert np.all(a["depth"][ok & (prim < 0)] == np.inf)
    assert np.max(np.abs(a["depth"][hit] - depth[hit]) / depth[hit]) <= 1e-4
    assert np.max(np.abs(a["normal"][hit] - normal[hit])) <= 1e-4
    albedo = np.array([[0.9, 0.2, 0.1], [0.1, 0.8, 0.3], [0.2, 0.3, 0.9], [0.5, 0.5, 0.5]], np.float32)
    assert np.array_equal(a["albedo"][hit], albedo[prim[hit]])


def test_features_of_a_shard_are_rows_of_the_frame(cpu):
    cpu.set_scene(scenes.scene_07())
    full = cpu.render_aov(67, 45)
    part = cpu.render_aov(67, 45, row_offset=1, row_stride=3)
    for k in full:
        assert np.array_equal(part[k], full[k][1::3], equal_nan=True), k


# ---- the filter --------------------------------------------------------------
@pytest.mark.parametrize("iterations", range(1, 7))
def test_filter_against_float64(cpu, frame07, iterations):
    scene, w, h, img, acc = frame07
    rgba, col = cpu.denoise(w, h, iterations=iterations, want_color=True)
    ref = reference(cpu, scene, w, h, acc, 4, iterations=iterations)
    err = R.rel_err(col, ref)
    print(f"iterations {iterations}: max |d| / (1 + |ref|) = {err:.3e}")
    assert err <= FILTER_BOUND
    assert rgba_within_1lsb(rgba, ref)
    assert not np.array_equal(rgba, img)


def test_identity_with_zero_iterations(cpu, frame07):
    scene, w, h, img, acc = frame07
    rgba, col = cpu.denoise(w, h, iterations=0, want_color=True)
    assert np.array_equal(rgba, img)
    assert np.array_equal(col, (np.float32(1) / np.float32(4)) * acc)


def test_state_is_untouched(bwrt_lib, oracle):
    scene = scenes.scene_07()
    w, h = 64, 36
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_scene(scene)
        r.render(w, h, 2, 4, first_frame=1)
        rng0, acc0 = r.get_state(h, w)
        frame0 = r.frame_counter
        r.render_aov(w, h)
        r.denoise(w, h)
        rng1, acc1 = r.get_state(h, w)
        assert r.frame_counter == frame0 == 3
        assert np.array_equal(rng0, rng1) and np.array_equal(acc0, acc1, equal_nan=True)
        img = r.render(w, h, 2, 4)
        rng2, acc2 = r.get_state(h, w)
    st = oracle.OracleState(w, h)
    oracle.render(scene, st, 4, 4, first_frame=1)
    assert np.array_equal(img, st.rgba)
    assert np.array_equal(acc2, st.accum, equal_nan=True)
    assert np.array_equal(rng2, st.rng)


def special_frame(r, w=48, h=48):
    """Scene 01 (a sphere on black sky: hit and miss regions), 2 frames, then a
    NaN, a +inf and a huge pixel written into frameSum through set_state.
    Returns (scene, w, h, frameSum, the three pixels)."""
    scene = scenes.scene_01()
    r.set_scene(scene)
    r.render(w, h, 2, 1, first_frame=1)
    rng, acc = r.get_state(h, w)
    prim = r.render_aov(w, h)["prim"]
    assert (prim >= 0).any() and (prim < 0).any()
    nan_px, inf_px, huge_px = (h // 2, w // 2), (2, 3), (h // 2 + 3, w // 2 - 2)
    assert prim[nan_px] >= 0 and prim[inf_px] < 0 and prim[huge_px] >= 0
    acc[nan_px] = np.nan
    acc[inf_px] = np.inf
    acc[huge_px] = 1e30
    r.set_state(rng, acc, 3)
    return scene, w, h, acc, (nan_px, inf_px, huge_px)


def test_special_values(bwrt_lib):
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        scene, w, h, acc, (nan_px, inf_px, huge_px) = special_frame(r)
        rgba, col = r.denoise(w, h, iterations=4, want_color=True)
        ref = reference(r, scene, w, h, acc, 2, iterations=4)
    assert np.isnan(col[nan_px]).all()
    assert np.all(col[inf_px] == np.inf)
    bad = ~np.isfinite(col).all(-1)
    bad[nan_px] = bad[inf_px] = False
    assert not bad.any()
    assert np.all(col[huge_px] == np.float32(0.5) * np.float32(1e30))  # every neighbour's weight is 0
    assert R.rel_err(col, ref) <= FILTER_BOUND


def test_extreme_sigmas(cpu, frame07):
    scene, w, h, img, acc = frame07
    inf = float("inf")
    rgba, col = cpu.denoise(w, h, iterations=3, sigma_color=inf, sigma_normal=inf, sigma_plane=inf,
                            want_color=True)
    ref = reference(cpu, scene, w, h, acc, 4, iterations=3, sigma_color=inf, sigma_normal=inf, sigma_plane=inf)
    assert R.rel_err(col, ref) <= FILTER_BOUND
    # edge-blind: an interior pixel far from the sky is the plain B3 blur of level 0
    _, col1 = cpu.denoise(w, h, iterations=1, sigma_color=inf, sigma_normal=inf, sigma_plane=inf, want_color=True)
    c0 = ((np.float32(1) / np.float32(4)) * acc).astype(np.float64)
    prim = cpu.render_aov(w, h)["prim"]
    y, x = 5, 30
    assert (prim[y - 2:y + 3, x - 2:x + 3] >= 0).all()
    k = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    blur = np.einsum("i,j,ijc->c", k, k, c0[y - 2:y + 3, x - 2:x + 3])
    assert np.allclose(col1[y, x], blur, rtol=1e-5)
    # a vanishing colour sigma: every tap but the centre weighs nothing
    _, colp = cpu.denoise(w, h, iterations=5, sigma_color=1e-30, want_color=True)
    assert np.array_equal(colp, (np.float32(1) / np.float32(4)) * acc)


def test_thread_invariance(bwrt_lib):
    out = []
    for threads in (1, 4):
        with Renderer.cpu(threads, lib=bwrt_lib) as r:
            r.set_scene(scenes.scene_07())
            r.render(67, 45, 2, 4, first_frame=1)
            a = r.render_aov(67, 45)
            rgba, col = r.denoise(67, 45, iterations=6, want_color=True)
            out.append((a, rgba, col))
    for k in out[0][0]:
        assert np.array_equal(out[0][0][k], out[1][0][k], equal_nan=True)
    assert np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2], equal_nan=True)


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (64, 32), (65, 33)])
def test_shapes(cpu, w, h):
    scene = scenes.scene_07()
    cpu.set_scene(scene)
    img, acc = cpu.render(w, h, 2, 4, first_frame=1, want_accum=True)
    rgba, col = cpu.denoise(w, h, iterations=6, want_color=True)
    assert rgba.shape == (h, w, 4) and col.shape == (h, w, 3)
    ref = reference(cpu, scene, w, h, acc, 2, iterations=6)
    assert R.rel_err(col, ref) <= FILTER_BOUND
    assert rgba_within_1lsb(rgba, ref)


def test_errors(bwrt_lib):
    lib = bwrt_lib
    with Renderer.cpu(1, lib=lib) as r:
        d = lib.rt_denoise_params_default()
        call = lambda p: lib.rt_denoise(r.ctx, C.byref(p), None, None)  # noqa: E731
        assert call(d) == abi.RT_ERR_NO_SCENE
        p = abi.RenderParams(8, 8, 1, 0, 0, 0, 1)
        assert lib.rt_render_aov(r.ctx, C.byref(p), None, None, None, None) == abi.RT_ERR_NO_SCENE
        r.set_scene(scenes.scene_07())
        assert call(d) == abi.RT_ERR_INVALID_ARGUMENT  # nothing accumulated (frame counter 1)
        assert b"no frame" in lib.rt_last_error(r.ctx)
        r.render(16, 9, 1, 2, first_frame=1)
        assert call(d) == abi.RT_OK
        for field, value in (("iterations", -1), ("iterations", abi.RT_DENOISE_MAX_ITERATIONS + 1),
                             ("sigma_color", 0.0), ("sigma_normal", -1.0), ("sigma_plane", float("nan"))):
            bad = lib.rt_denoise_params_default()
            setattr(bad, field, value)
            assert call(bad) == abi.RT_ERR_INVALID_ARGUMENT, field
        assert lib.rt_denoise_device(r.ctx, C.byref(d), None, None) == abi.RT_ERR_UNSUPPORTED  # CPU context
        r.reset_accumulation()
        assert call(d) == abi.RT_ERR_INVALID_ARGUMENT
        r.render(16, 9, 1, 2, first_frame=1, row_offset=1, row_stride=2)  # the state is now a row shard
        assert call(d) == abi.RT_ERR_UNSUPPORTED
        assert lib.rt_last_denoise_ms(r.ctx) >= 0.0
    with Renderer.cpu(1, lib=lib) as r:
        assert lib.rt_last_denoise_ms(r.ctx) == -1.0


def test_guides_follow_the_camera(cpu):
    """The kept guides are recomputed after rt_controls / rt_set_camera."""
    scene = scenes.scene_07()
    cpu.set_scene(scene)
    w, h = 48, 27
    cpu.render(w, h, 2, 3, first_frame=1)
    cpu.denoise(w, h)
    assert cpu.controls(["LEFT"], 0.1) & abi.CONTROLS_MOVED
    img, acc = cpu.render(w, h, 2, 3, want_accum=True)
    _, col = cpu.denoise(w, h, want_color=True)
    scene.set_camera(cpu.get_camera())
    ref = reference(cpu, scene, w, h, acc, 2)
    assert R.rel_err(col, ref) <= FILTER_BOUND


def test_quality_of_the_defaults(bwrt_lib):
    """The condition for shipping the defaults: on the sweep's case (scene 07,
    160x90, 8 frames, 4 bounces) the denoised frame is closer to a 2048-frame
    render than the raw one."""
    w, h = 160, 90
    scene = scenes.scene_07()
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_scene(scene)
        truth = r.render(w, h, 2048, 4, first_frame=1).astype(np.int32)
    with Renderer.cpu(0, lib=bwrt_lib) as r:  # fresh RNG streams, as tools/denoise_sigma_sweep.py
        r.set_scene(scene)
        raw = r.render(w, h, 8, 4, first_frame=1)
        den = r.denoise(w, h)
    e_raw = np.abs(raw[..., :3] - truth[..., :3]).mean()
    e_den = np.abs(den[..., :3] - truth[..., :3]).mean()
    print(f"mean |error| raw {e_raw:.3f}, denoised {e_den:.3f}, ratio {e_den / e_raw:.3f}")
    assert e_den < e_raw


def test_cli_denoise_and_aov(tmp_path):
    raw, den, prefix = tmp_path / "raw.ppm", tmp_path / "den.ppm", tmp_path / "f"
    base = [CLI, "--cpu", "2", "--width", "64", "--height", "36", "--frames", "3", "--max-bounces", "3"]
    subprocess.run(base + ["--out", str(raw)], check=True, capture_output=True)
    res = subprocess.run(base + ["--out", str(den), "--denoise", "--aov", str(prefix)], check=True,
                         capture_output=True, text=True)
    assert "denoise: 5 levels" in res.stdout
    files = [den] + [tmp_path / f"f_{k}.ppm" for k in ("albedo", "normal", "depth")]
    for f in files:
        assert f.stat().st_size == raw.stat().st_size, f
    assert den.read_bytes() != raw.read_bytes()
    assert len({f.read_bytes() for f in files}) == 4
