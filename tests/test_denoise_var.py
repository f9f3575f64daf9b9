"""The variance-guided a-trous filter (rt_denoise_var) on the CPU backend — no
GPU needed.  The GPU kernels compute the same bits (tests/test_gpu_denoise_var.py
compares them with this backend).

The float64 reference is tests/denoise_var_ref.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import denoise_var_ref as V
from bwrt import Renderer, abi, scenes

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd", "bin",
                   "bwrt_render")

# The frame of the float64 comparison: scene 07 under a sky (rt_set_background),
# 67x45, 4 bounces, 8 one-frame calls.  Under the scene's own black sky nine
# pixels in ten have seen no light after 8 frames and the frame's median
# variance, the floor of the variance metric, is 0.
SKY = (0.25, 0.35, 0.5)

# max |colour - float64 reference| / (1 + |reference|) and max |variance -
# reference| / (eps_v + |reference|), eps_v the median of the frame's input
# variance v0.  Measured on the CPU backend over the cases of
# test_filter_against_float64 (both modes, levels 1..6): colour 2.86e-6
# (float32 rounding of sums of up to 25 taps, of the guides and of exp_nn,
# through up to six levels and their sigma passes); variance, tracked 1.08e-5
# (eps_v 1.0e-3), spatial 1.35e-5 (eps_v 3.8e-2; the spatial v0 is s2 / s0 -
# m1^2 in float32: it cancels luminance squares of ~1).  Asserted at 8x.
COLOR_BOUND = 8 * 2.86e-6
VAR_BOUND = {"tracked": 8 * 1.08e-5, "spatial": 8 * 1.35e-5}
MAX_MARKED = 0.02
# the float64 comparisons run at SVGF's 4 standard deviations, where the
# luminance term decides most taps (the default, 32, is wide: DESIGN.md section 11)
SIGMA = 4.0

# max |16 dim - bright| / (mean(bright) + |bright|) of the filtered colours of
# scene 07 and of the same scene with every emittance times 2^-4
# (test_brightness_equivariance, default parameters).  Measured on the CPU
# backend: tracked 1.26e-7, spatial 0 (the 1e-10 floor of the sigma is the one
# term that does not scale; rt_denoise with its fixed default sigma_color: 4.1
# and 4.0).  Asserted at 8x.
EQUIVARIANCE_BOUND = 8 * 1.26e-7


@pytest.fixture(scope="module")
def cpu(bwrt_lib):
    r = Renderer.cpu(0, lib=bwrt_lib)
    yield r
    r.close()


def accumulate(r, w, h, calls=8, bounces=4, track=True):
    """`calls` one-frame render calls from frame 1; returns the last (rgba, frameSum)."""
    r.set_moments(track)
    for i in range(calls):
        out = r.render(w, h, 1, bounces, first_frame=1 if i == 0 else 0, want_accum=True)
    return out


def reference(r, scene, w, h, acc, n, var0=None, masked=None, **kw):
    d = r.denoise_var_params(**kw)
    a = r.render_aov(w, h)
    P = R.hit_points(scene.camera, w, h, a["depth"], a["prim"])
    return V.denoise_var_ref(acc, n, a["normal"], P, a["prim"], d.iterations, d.sigma_lum, d.sigma_normal,
                             d.sigma_plane, var0=var0, masked=masked)


@pytest.fixture(scope="module", params=["tracked", "spatial"])
def frame07(request, bwrt_lib):
    """(mode, renderer, scene, w, h, rgba, frameSum, tracked variance or None)."""
    mode = request.param
    scene = scenes.scene_07()
    w, h = 67, 45
    r = Renderer.cpu(0, lib=bwrt_lib)
    r.set_scene(scene)
    r.set_background(*SKY)
    img, acc = accumulate(r, w, h, track=mode == "tracked")
    var0 = r.variance(h, w) if mode == "tracked" else None
    assert r.moments_batches == (8 if mode == "tracked" else 0)
    yield mode, r, scene, w, h, img, acc, var0
    r.close()


def test_abi_declares_the_entry_points(bwrt_lib):
    names = {"rt_denoise_var", "rt_denoise_var_device", "rt_denoise_var_params_default", "rt_last_denoise_var_ms"}
    assert names <= set(abi.declared_functions())
    for n in names:
        assert hasattr(bwrt_lib, n)
    d = bwrt_lib.rt_denoise_var_params_default()
    assert d.iterations == 5 and d.sigma_lum == 32.0 and d.min_batches == 4
    dn = bwrt_lib.rt_denoise_params_default()
    assert d.sigma_normal == dn.sigma_normal and d.sigma_plane == dn.sigma_plane


@pytest.mark.parametrize("iterations", range(1, 7))
def test_filter_against_float64(frame07, iterations):
    mode, r, scene, w, h, img, acc, var0 = frame07
    rgba, col, var = r.denoise_var(w, h, want_color=True, want_var=True, iterations=iterations, sigma_lum=SIGMA)
    rc, rv, marked = reference(r, scene, w, h, acc, 8, var0=var0, iterations=iterations, sigma_lum=SIGMA)
    v0 = r.denoise_var(w, h, want_var=True, iterations=0)[1]
    eps = float(np.median(v0))
    keep = ~marked
    e_c = V.rel_err(col, rc, 1.0, keep[..., None])
    e_v = V.rel_err(var, rv, eps, keep)
    print(f"{mode} {iterations}: colour {e_c:.3e}, variance {e_v:.3e} (eps_v {eps:.3e}), marked {marked.mean():.4f}")
    assert eps > 0
    assert marked.mean() <= MAX_MARKED
    assert e_c <= COLOR_BOUND
    assert e_v <= VAR_BOUND[mode]
    assert not np.array_equal(rgba, img)
    ok = np.abs(rgba.astype(np.int32) - R.tone_map(rc).astype(np.int32)).max(-1) <= 1
    assert ok[keep].all()


def test_identity_with_zero_iterations(frame07):
    mode, r, scene, w, h, img, acc, var0 = frame07
    rgba, col, var = r.denoise_var(w, h, want_color=True, want_var=True, iterations=0)
    assert np.array_equal(rgba, img)
    assert np.array_equal(col, (np.float32(1) / np.float32(8)) * acc)
    if mode == "tracked":
        assert np.array_equal(var, var0)
    else:
        ref = reference(r, scene, w, h, acc, 8, iterations=0)[1]
        assert V.rel_err(var, ref, float(np.median(ref))) <= VAR_BOUND["spatial"]
        assert (var >= 0).all() and (var > 0).mean() > 0.5


def test_min_batches_selects_the_estimate(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 33, 17
    with Renderer.cpu(2, lib=bwrt_lib) as r:
        r.set_scene(scene)
        r.set_background(*SKY)
        accumulate(r, w, h, calls=3, track=True)
        tracked = r.variance(h, w)
        v = lambda **kw: r.denoise_var(w, h, want_var=True, iterations=0, **kw)[1]  # noqa: E731
        spatial = v()  # J = 3 < min_batches = 4
        assert not np.array_equal(spatial, tracked)
        assert np.array_equal(v(min_batches=3), tracked)
        assert np.array_equal(v(min_batches=2), tracked)
        r.render(w, h, 1, 4)
        assert np.array_equal(v(), r.variance(h, w))  # J = 4
        r.set_moments(False)
        off = v(min_batches=2)
    with Renderer.cpu(2, lib=bwrt_lib) as r:  # the spatial estimate of the same frame, never tracked
        r.set_scene(scene)
        r.set_background(*SKY)
        accumulate(r, w, h, calls=4, track=False)
        assert np.array_equal(r.denoise_var(w, h, want_var=True, iterations=0)[1], off)


def special_frame(r, w=48, h=48):
    """Scene 07 under the sky (hit and miss regions), 4 one-frame calls, then a
    NaN and a +inf pixel written into frameSum through set_state (which ends
    the tracking: the spatial estimate serves).  Returns (scene, w, h,
    frameSum, the two pixels)."""
    scene = scenes.scene_07()
    r.set_scene(scene)
    r.set_background(*SKY)
    accumulate(r, w, h, calls=4, bounces=2)
    rng, acc = r.get_state(h, w)
    prim = r.render_aov(w, h)["prim"]
    nan_px, inf_px = (h // 4, w // 2), (h - 3, 3)
    assert prim[nan_px] >= 0 and prim[inf_px] < 0
    acc[nan_px] = np.nan
    acc[inf_px] = np.inf
    r.set_state(rng, acc, 5)
    return scene, w, h, acc, (nan_px, inf_px)


def check_special(col, var, ref, eps, pixels):
    nan_px, inf_px = pixels
    rc, rv, marked = ref
    assert np.isnan(col[nan_px]).all() and np.all(col[inf_px] == np.inf)  # pass through
    bad = ~(np.isfinite(col).all(-1) & np.isfinite(var))
    bad[nan_px] = bad[inf_px] = False
    assert not bad.any()  # they spoil no neighbour
    keep = ~marked
    keep[nan_px] = keep[inf_px] = False
    assert marked.mean() <= MAX_MARKED
    assert V.rel_err(col, rc, 1.0, keep[..., None]) <= COLOR_BOUND
    assert V.rel_err(var, rv, eps, keep) <= VAR_BOUND["spatial"]


def test_special_values(bwrt_lib):
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        scene, w, h, acc, pixels = special_frame(r)
        assert r.moments_batches == 0
        masked = np.zeros((h, w), bool)
        for px in pixels:
            masked[px] = True
        rgba, col, var = r.denoise_var(w, h, want_color=True, want_var=True, iterations=4, sigma_lum=SIGMA)
        ref = reference(r, scene, w, h, acc, 4, masked=masked, iterations=4, sigma_lum=SIGMA)
        eps = float(np.median(reference(r, scene, w, h, acc, 4, masked=masked, iterations=0)[1]))
        # the spoiled pixels' taps are skipped: the rest is the filter of the frame without them
        check_special(col, var, ref, eps, pixels)
        col0 = r.denoise_var(w, h, want_color=True, iterations=0)[1]
        assert not np.array_equal(col[~masked], col0[~masked])


def test_flat_frames_come_back_unchanged(bwrt_lib):
    """An all-miss frame (both modes) and an emitter-only frame whose samples
    are all equal (tracked: zero variance; spatially its rim is an edge like any
    other); colours that are powers of two, so every weighted mean is exact: the
    input colours, bit for bit."""
    cam = scenes.Camera(scenes.vec(0, 0, 0), (C.c_float * 2)(0.0, 0.0), float(scenes.PI / np.float32(2)))
    empty = scenes.Scene(cam, [scenes.Sphere(scenes.vec(0, 0, 50), 1.0, scenes.material((1, 1, 1), 1))])  # behind
    w, h = 48, 27
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        for scene, bg, all_miss in ((empty, (0.5, 0.25, 0.125), True), (scenes.scene_01(), (0, 0, 0), False)):
            for track in ((True, False) if all_miss else (True,)):
                r.set_scene(scene)
                r.set_background(*bg)
                img, acc = accumulate(r, w, h, calls=4, bounces=1, track=track)
                prim = r.render_aov(w, h)["prim"]
                assert (prim < 0).all() if all_miss else ((prim >= 0).any() and (prim < 0).any())
                if track:
                    assert not r.variance(h, w).any()  # every sample equal
                rgba, col, var = r.denoise_var(w, h, want_color=True, want_var=True, iterations=5, min_batches=2)
                assert np.array_equal(col, np.float32(0.25) * acc)
                assert np.array_equal(rgba, img)
                assert len(np.unique(col.reshape(-1, 3), axis=0)) == (1 if all_miss else 2)
                if track:
                    assert not var.any()


def dim_scene(factor):
    scene = scenes.scene_07()
    for i in range(scene.counts[0]):
        scene.spheres[i].mat.emittance *= factor
    return scene


def test_brightness_equivariance(bwrt_lib):
    """The property a fixed sigma cannot have: every emittance times 2^-4
    (exact in float) gives exactly 2^-4 of frameSum, and the filtered colour
    follows, up to the 1e-10 floor of the sigma.  rt_denoise with its default
    sigma_color is printed as the contrast."""
    w, h = 67, 45
    out = {}
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        for name, factor in (("bright", 1.0), ("dim", 0.0625)):
            for mode in ("tracked", "spatial"):
                r.set_scene(dim_scene(factor))
                r.init_rand(w, h)  # the same RNG streams for every run
                _, acc = accumulate(r, w, h, track=mode == "tracked")
                col = r.denoise_var(w, h, want_color=True)[1]
                fixed = r.denoise(w, h, want_color=True)[1]
                out[name, mode] = acc, col, fixed
    for mode in ("tracked", "spatial"):
        (acc_b, col_b, fix_b), (acc_d, col_d, fix_d) = out["bright", mode], out["dim", mode]
        assert np.array_equal(np.float32(16) * acc_d, acc_b) and acc_b.any()
        s = float(col_b.mean())
        err = lambda d, b: float(np.max(np.abs(16.0 * d.astype(np.float64) - b) / (s + np.abs(b))))  # noqa: E731
        e_var, e_fix = err(col_d, col_b), err(fix_d, fix_b)
        print(f"{mode}: rt_denoise_var {e_var:.3e}; rt_denoise with the default sigma_color {e_fix:.3e}")
        assert e_var <= EQUIVARIANCE_BOUND
        assert not np.array_equal(col_b, np.float32(0.125) * acc_b)  # it did filter


def test_thread_invariance(bwrt_lib):
    out = []
    for threads in (1, 4):
        with Renderer.cpu(threads, lib=bwrt_lib) as r:
            r.set_scene(scenes.scene_07())
            accumulate(r, 67, 45, calls=4)
            out.append(r.denoise_var(67, 45, want_color=True, want_var=True, iterations=6))
            r.set_moments(False)
            out[-1] += r.denoise_var(67, 45, want_color=True, want_var=True, iterations=6)
    for a, b in zip(*out):
        assert np.array_equal(a, b, equal_nan=True)


def neutrality_sequence(r, scene, w, h, track):
    """Renders interleaved with the readout and the filter; everything a render
    leaves behind, after every step."""
    r.set_scene(scene)
    r.set_moments(track)
    seen = []

    def snap(img):
        seen.append((img, r.frame_counter) + r.get_state(h, w))

    snap(r.render(w, h, 1, 4, first_frame=1))
    snap(r.render(w, h, 2, 4))
    if track:
        r.variance(h, w)
    r.denoise_var(w, h, min_batches=2)
    snap(r.render(w, h, 1, 4))
    r.denoise_var(w, h, iterations=6)
    r.denoise(w, h)
    snap(r.render(w, h, 3, 4))
    r.reset_accumulation()
    snap(r.render(w, h, 1, 4))
    r.denoise_var(w, h)
    snap(r.render(w, h, 1, 4))
    if track:
        assert r.moments_batches == 2
        r.variance(h, w)
    return seen


def same_sequences(on, off):
    assert len(on) == len(off) == 6
    for a, b in zip(on, off):
        assert np.array_equal(a[0], b[0])  # RGBA
        assert a[1] == b[1]  # frame counter
        assert np.array_equal(a[2], b[2])  # RNG state
        assert np.array_equal(a[3], b[3], equal_nan=True)  # frameSum


def test_neutrality(bwrt_lib):
    scene = scenes.scene_07()
    runs = []
    for track in (True, False):
        with Renderer.cpu(0, lib=bwrt_lib) as r:
            runs.append(neutrality_sequence(r, scene, 67, 45, track))
    same_sequences(*runs)


def test_moments_survive_the_filter(bwrt_lib):
    """The filter reads the tracked moments and writes none of them."""
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_scene(scenes.scene_07())
        accumulate(r, 67, 45, calls=4)
        before = r.variance(45, 67, want_lum=True)
        r.denoise_var(67, 45, iterations=6)
        after = r.variance(45, 67, want_lum=True)
        assert r.moments_batches == 4
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# rt_denoise, rt_denoise_var, rt_temporal with the default filter and rt_denoise
# again: every pass that shares the guides and the two colour buffers
PASS_CALLS = (
    lambda r, w, h: r.denoise(w, h, want_color=True),
    lambda r, w, h: r.denoise_var(w, h, want_color=True, want_var=True),
    lambda r, w, h: r.temporal(w, h, denoise={}, want_color=True, want_length=True),
    lambda r, w, h: r.denoise(w, h, want_color=True),
)


def passes(make, calls, w=67, h=45):
    """The PASS_CALLS `calls`, in that order, on one fresh context (`make`)
    that holds scene 07 under the sky after 8 tracked one-frame calls."""
    with make() as r:
        r.set_scene(scenes.scene_07())
        r.set_background(*SKY)
        r.init_rand(w, h)
        accumulate(r, w, h)
        assert r.moments_batches == 8
        return [PASS_CALLS[i](r, w, h) for i in calls]


def same_results(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_passes_carry_nothing_over(bwrt_lib):
    """The four passes in a row on one accumulated frame: each gives what it
    gives alone on a fresh context, and rt_denoise gives the same bits before
    and after the others used its colour buffers and guides."""
    def make():
        return Renderer.cpu(0, lib=bwrt_lib)
    row = passes(make, range(4))
    assert same_results(row[0], row[3])
    for i in range(3):
        assert same_results(passes(make, [i])[0], row[i]), i
    assert not np.array_equal(row[0][1], row[1][1])  # (two filters; the first temporal call has no history)


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (333, 187)])
def test_shapes(cpu, w, h):
    scene = scenes.scene_07()
    cpu.set_scene(scene)
    cpu.set_background(*SKY)
    for track in (True, False):
        img, acc = accumulate(cpu, w, h, calls=4, track=track)
        var0 = cpu.variance(h, w) if track else None
        rgba, col, var = cpu.denoise_var(w, h, want_color=True, want_var=True, iterations=5, sigma_lum=SIGMA)
        assert rgba.shape == (h, w, 4) and col.shape == (h, w, 3) and var.shape == (h, w)
        rc, rv, marked = reference(cpu, scene, w, h, acc, 4, var0=var0, iterations=5, sigma_lum=SIGMA)
        keep = ~marked
        assert marked.mean() <= MAX_MARKED
        assert V.rel_err(col, rc, 1.0, keep[..., None]) <= COLOR_BOUND
        if w * h > 15:  # (a handful of pixels has no median variance to measure against)
            eps = float(np.median(cpu.denoise_var(w, h, want_var=True, iterations=0)[1]))
            assert V.rel_err(var, rv, eps, keep) <= VAR_BOUND["tracked" if track else "spatial"]
    cpu.set_moments(False)
    cpu.set_background(0, 0, 0)


def test_errors(bwrt_lib):
    lib = bwrt_lib
    with Renderer.cpu(1, lib=lib) as r:
        d = lib.rt_denoise_var_params_default()
        call = lambda p: lib.rt_denoise_var(r.ctx, C.byref(p), None, None, None)  # noqa: E731
        assert call(d) == abi.RT_ERR_NO_SCENE
        r.set_scene(scenes.scene_07())
        assert call(d) == abi.RT_ERR_INVALID_ARGUMENT  # nothing accumulated (frame counter 1)
        assert b"no frame" in lib.rt_last_error(r.ctx)
        assert lib.rt_last_denoise_var_ms(r.ctx) == -1.0
        r.render(16, 9, 1, 2, first_frame=1)
        assert call(d) == abi.RT_OK
        assert lib.rt_last_denoise_var_ms(r.ctx) >= 0.0
        for field, value in (("iterations", -1), ("iterations", abi.RT_DENOISE_MAX_ITERATIONS + 1),
                             ("sigma_lum", 0.0), ("sigma_lum", float("nan")), ("sigma_normal", -1.0),
                             ("sigma_plane", float("nan")), ("min_batches", 1)):
            bad = lib.rt_denoise_var_params_default()
            setattr(bad, field, value)
            assert call(bad) == abi.RT_ERR_INVALID_ARGUMENT, field
        assert lib.rt_denoise_var(r.ctx, None, None, None, None) == abi.RT_ERR_INVALID_ARGUMENT
        assert lib.rt_denoise_var_device(r.ctx, C.byref(d), None, None) == abi.RT_ERR_UNSUPPORTED  # CPU context
        r.reset_accumulation()
        assert call(d) == abi.RT_ERR_INVALID_ARGUMENT
        r.render(16, 9, 1, 2, first_frame=1, row_offset=1, row_stride=2)  # the state is now a row shard
        assert call(d) == abi.RT_ERR_UNSUPPORTED


def test_quality_of_the_defaults(bwrt_lib):
    """The sweep's case (scene 07, 160x90, 8 frames as 8 calls, 4 bounces): the
    frame filtered with the default parameters is closer to a 2048-frame render
    than the raw one."""
    w, h = 160, 90
    scene = scenes.scene_07()
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_scene(scene)
        truth = r.render(w, h, 2048, 4, first_frame=1).astype(np.int32)
    with Renderer.cpu(0, lib=bwrt_lib) as r:  # fresh RNG streams, as tools/denoise_var_sweep.py
        r.set_scene(scene)
        raw, _ = accumulate(r, w, h)
        assert r.moments_batches == 8
        den = r.denoise_var(w, h)
        fixed = r.denoise(w, h)
    e = [np.abs(x[..., :3] - truth[..., :3]).mean() for x in (raw, den, fixed)]
    print(f"mean |error| raw {e[0]:.3f}, rt_denoise_var {e[1]:.3f} (ratio {e[1] / e[0]:.3f}), "
          f"rt_denoise {e[2]:.3f} (ratio {e[2] / e[0]:.3f})")
    assert e[1] < e[0]


def test_cli_denoise_var(tmp_path):
    raw, den = tmp_path / "raw.ppm", tmp_path / "den.ppm"
    base = [CLI, "--cpu", "2", "--width", "64", "--height", "36", "--frames", "4", "--max-bounces", "3"]
    subprocess.run(base + ["--out", str(raw)], check=True, capture_output=True)
    res = subprocess.run(base + ["--out", str(den), "--denoise-var", "--sigma-lum", "3", "--min-batches", "2"],
                         check=True, capture_output=True, text=True)
    assert "denoise-var: 5 levels, tracked variance of 4 batches" in res.stdout
    assert den.stat().st_size == raw.stat().st_size and den.read_bytes() != raw.read_bytes()
    res = subprocess.run(base + ["--out", str(den), "--denoise-var", "--min-batches", "5"], check=True,
                         capture_output=True, text=True)
    assert "denoise-var: 5 levels, spatial variance" in res.stdout
    res = subprocess.run(base + ["--denoise", "--denoise-var"], capture_output=True, text=True)
    assert res.returncode == 2 and "--denoise-var" in res.stderr
