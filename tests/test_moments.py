"""Luminance moment tracking (rt_set_moments, rt_get_variance) on the CPU
backend — no GPU needed.  The GPU kernel computes the same bits
(tests/test_gpu_moments.py compares it with this backend).

The float64 reference is tests/moments_ref.py.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import moments_ref as R
from bwrt import Renderer, abi, scenes

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd", "bin",
                   "bwrt_render")

BATCHES = (1, 1, 3, 2)  # frames per render call of the reference sequence

# max |M - float64 reference| / (scale + |reference|) and the same for var,
# scale = the frame's mean luminance.  Measured on the CPU backend over the case
# of test_update_against_float64 (scene 07, 67x45, 4 bounces, batches 1, 1, 3,
# 2; mean luminance 0.106): M 1.70e-7, var 2.98e-7 (float32 rounding of the four
# Welford steps and of frameSum differences whose operands reach ~100 times the
# scale).  Asserted at 8x: a missing or doubled factor moves either by O(1).
MOMENT_BOUND_M = 8 * 1.70e-7
MOMENT_BOUND_VAR = 8 * 2.98e-7

# ln of R = sum_p mean(var_p) / sum_p empirical variance of the replicate means
# (test_estimator_is_a_variance_of_the_mean).  Measured on the CPU backend:
# R = 1.0086, |ln R| = 0.0086; 3x that is below the floor ln 1.1, which
# therefore is the bound (inside the cap 0.5 < R < 2 that rejects a missing or
# doubled division by J - 1 or n).
LN_R_MEASURED = 0.0086
LN_R_BOUND = min(max(3 * LN_R_MEASURED, math.log(1.1)), math.log(2.0) * 0.999)


@pytest.fixture(scope="module")
def cpu(bwrt_lib):
    r = Renderer.cpu(0, lib=bwrt_lib)
    yield r
    r.close()


def tracked_sequence(r, scene, w, h, batches=BATCHES, bounces=4, **shard):
    """Scene set, tracking on, one render call per batch from frame 1.
    Returns the frameSum snapshots after each call."""
    r.set_scene(scene)
    r.set_moments(True)
    snaps = []
    for i, k in enumerate(batches):
        _, acc = r.render(w, h, k, bounces, first_frame=1 if i == 0 else 0, want_accum=True, **shard)
        snaps.append(acc)
    return snaps


def test_abi_declares_the_entry_points(bwrt_lib):
    names = {"rt_set_moments", "rt_get_moments", "rt_moments_batches", "rt_get_variance"}
    assert names <= set(abi.declared_functions())
    for n in names:
        assert hasattr(bwrt_lib, n)
    with Renderer.cpu(1, lib=bwrt_lib) as r:
        assert r.moments is False and r.moments_batches == 0  # off by default
        r.set_moments(True)
        assert r.moments is True and r.moments_batches == 0
        r.set_moments(False)
        assert r.moments is False


def test_update_against_float64(cpu):
    scene = scenes.scene_07()
    w, h = 67, 45
    snaps = tracked_sequence(cpu, scene, w, h)
    assert cpu.moments_batches == len(BATCHES)
    var, M = cpu.variance(h, w, want_lum=True)
    rvar, rM = R.variance_ref(snaps, BATCHES)
    scale = float(rM.mean())
    e_m, e_v = R.rel_err(M, rM, scale), R.rel_err(var, rvar, scale)
    print(f"scale {scale:.4f}: M {e_m:.3e}, var {e_v:.3e}")
    assert scale > 0.05 and (rvar > 0).mean() > 0.05  # a frame with light and noise in it
    assert e_m <= MOMENT_BOUND_M
    assert e_v <= MOMENT_BOUND_VAR
    # M is the mean luminance of frameSum / n
    n = sum(BATCHES)
    assert np.allclose(M, R.lum(snaps[-1]) / n, rtol=1e-5, atol=1e-5 * scale)
    cpu.set_moments(False)


def test_lifecycle(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 33, 17
    lib = bwrt_lib
    with Renderer.cpu(2, lib=lib) as r:
        r.set_scene(scene)
        no_var = lambda: lib.rt_get_variance(r.ctx, None, None)  # noqa: E731
        # off: renders track nothing
        r.render(w, h, 1, 2, first_frame=1)
        assert r.moments_batches == 0 and no_var() == abi.RT_ERR_INVALID_ARGUMENT
        # enabled in mid-accumulation: not live until a frame-1 render
        r.set_moments(True)
        r.render(w, h, 1, 2)
        assert r.moments_batches == 0
        r.render(w, h, 1, 2, first_frame=1)
        assert r.moments_batches == 1
        assert no_var() == abi.RT_ERR_INVALID_ARGUMENT  # J < 2
        assert b"variance" in lib.rt_last_error(r.ctx)
        r.render(w, h, 3, 2)
        assert r.moments_batches == 2 and no_var() == abi.RT_OK
        r.render(w, h, 2, 2, first_frame=5)  # the expected next frame, given explicitly
        assert r.moments_batches == 3
        # a non-contiguous first frame ends it; a frame-1 render revives it
        r.render(w, h, 1, 2, first_frame=9)
        assert r.moments_batches == 0 and no_var() == abi.RT_ERR_INVALID_ARGUMENT
        r.render(w, h, 1, 2)
        assert r.moments_batches == 0
        r.render(w, h, 1, 2, first_frame=1)
        r.render(w, h, 1, 2)
        assert r.moments_batches == 2
        # rt_set_state
        rng, acc = r.get_state(h, w)
        r.set_state(rng, acc, r.frame_counter)
        assert r.moments_batches == 0
        r.render(w, h, 1, 2)
        assert r.moments_batches == 0
        # resets of the frame counter restart tracking at the next render
        for restart in (r.reset_accumulation, lambda: r.set_camera(scene.camera),
                        lambda: r.controls(["LEFT"], 0.05), lambda: r.set_scene(scene)):
            r.render(w, h, 1, 2, first_frame=1)
            r.render(w, h, 1, 2)
            r.render(w, h, 1, 2)
            assert r.moments_batches == 3
            restart()
            assert r.frame_counter == 1
            r.render(w, h, 2, 2)
            assert r.moments_batches == 1
        # a shape change (the implicit rt_init_rand) ends it, also with an explicit later frame
        r.render(w, h, 1, 2)
        assert r.moments_batches == 2
        r.render(w + 1, h, 1, 2, first_frame=4)
        assert r.moments_batches == 0
        r.render(w + 1, h, 1, 2, first_frame=1)
        r.render(w + 1, h, 1, 2)
        assert r.moments_batches == 2
        r.init_rand(w + 1, h)
        assert r.moments_batches == 0
        # off ends it and drops the count
        r.render(w + 1, h, 1, 2)
        r.render(w + 1, h, 1, 2)
        assert r.moments_batches == 2
        r.set_moments(False)
        assert r.moments_batches == 0 and no_var() == abi.RT_ERR_INVALID_ARGUMENT
        r.set_moments(True)
        r.render(w + 1, h, 1, 2)
        assert r.moments_batches == 0


def test_restart_equals_a_fresh_context(bwrt_lib):
    """After rt_reset_accumulation the moments are those of the new
    accumulation alone: nothing of the old one is read."""
    scene = scenes.scene_07()
    w, h = 33, 17
    with Renderer.cpu(2, lib=bwrt_lib) as r:
        tracked_sequence(r, scene, w, h, (2, 1, 1))
        rng, _ = r.get_state(h, w)
        r.reset_accumulation()
        for k in (1, 2):
            r.render(w, h, k, 4)
        got = r.variance(h, w, want_lum=True)
    with Renderer.cpu(2, lib=bwrt_lib) as r:
        r.set_scene(scene)
        r.init_rand(w, h)
        r.set_state(rng, np.zeros((h, w, 3), np.float32), 1)
        r.set_moments(True)
        for k in (1, 2):
            r.render(w, h, k, 4)
        want = r.variance(h, w, want_lum=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_shard_equals_rows_of_the_frame(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 67, 45
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        tracked_sequence(r, scene, w, h)
        full = r.variance(h, w, want_lum=True)
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        tracked_sequence(r, scene, w, h, row_offset=1, row_stride=3)
        rows = len(range(1, h, 3))
        assert r.moments_batches == len(BATCHES)
        part = r.variance(rows, w, want_lum=True)
    assert np.array_equal(part[0], full[0][1::3]) and np.array_equal(part[1], full[1][1::3])
    assert (full[0] > 0).any()


def test_thread_invariance(bwrt_lib):
    out = []
    for threads in (1, 4):
        with Renderer.cpu(threads, lib=bwrt_lib) as r:
            tracked_sequence(r, scenes.scene_07(), 67, 45)
            out.append(r.variance(45, 67, want_lum=True))
    # and rt_render_cpu's per-call thread count
    with Renderer.cpu(1, lib=bwrt_lib) as r:
        r.set_scene(scenes.scene_07())
        r.set_moments(True)
        for i, k in enumerate(BATCHES):
            r.render_cpu(67, 45, k, 4, first_frame=1 if i == 0 else 0, threads=3)
        assert r.moments_batches == len(BATCHES)
        out.append(r.variance(45, 67, want_lum=True))
    for o in out[1:]:
        assert np.array_equal(o[0], out[0][0]) and np.array_equal(o[1], out[0][1])


def neutrality_sequence(r, scene, w, h, track):
    """Renders interleaved with the readout and the denoiser; everything a
    render leaves behind, after every step."""
    r.set_scene(scene)
    r.set_moments(track)
    seen = []

    def snap(img):
        seen.append((img, r.frame_counter) + r.get_state(h, w))

    snap(r.render(w, h, 1, 4, first_frame=1))
    snap(r.render(w, h, 2, 4))
    if track:
        r.variance(h, w)
    snap(r.render(w, h, 1, 4))
    seen.append((r.denoise(w, h), r.frame_counter) + r.get_state(h, w))
    snap(r.render(w, h, 3, 4))
    r.reset_accumulation()
    snap(r.render(w, h, 1, 4))
    snap(r.render(w, h, 1, 4))
    if track:
        assert r.moments_batches == 2
        r.variance(h, w)
    snap(r.render(w, h, 2, 4, first_frame=7))  # ends the tracking, not the accumulation
    return seen


def test_neutrality(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 67, 45
    runs = []
    for track in (True, False):
        with Renderer.cpu(0, lib=bwrt_lib) as r:
            runs.append(neutrality_sequence(r, scene, w, h, track))
    assert len(runs[0]) == len(runs[1]) == 8
    for on, off in zip(*runs):
        assert np.array_equal(on[0], off[0])  # RGBA
        assert on[1] == off[1]  # frame counter
        assert np.array_equal(on[2], off[2])  # RNG state
        assert np.array_equal(on[3], off[3], equal_nan=True)  # frameSum


def estimator_ratio(r, scene, w=48, h=27, calls=16, replicates=64, bounces=4):
    """R of the docstring below, with tracking on in `r`."""
    r.set_scene(scene)
    r.set_moments(True)
    var, mean = [], []
    for _ in range(replicates):
        r.reset_accumulation()  # the RNG streams continue: an independent replicate
        for _ in range(calls):
            r.render(w, h, 1, bounces)
        assert r.moments_batches == calls
        v, m = r.variance(h, w, want_lum=True)
        var.append(v.astype(np.float64))
        mean.append(m.astype(np.float64))
    return float(np.mean(var, 0).sum() / np.var(mean, 0, ddof=1).sum())


def test_estimator_is_a_variance_of_the_mean(bwrt_lib):
    """64 independent replicates of 16 one-frame calls (scene 07, 48x27):
    R = sum_p mean over replicates(var_p) / sum_p empirical variance of the 64
    replicate means M_p estimates 1."""
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        ratio = estimator_ratio(r, scenes.scene_07())
    print(f"R = {ratio:.4f}, |ln R| = {abs(math.log(ratio)):.4f}")
    assert 0.5 < ratio < 2.0
    assert abs(math.log(ratio)) <= LN_R_BOUND


def test_batch_sizes_do_not_bias_the_estimate(bwrt_lib):
    """Batches of unequal sizes: E[M2] = sigma^2 (J - 1) still, so the same
    ratio over 64 replicates of the calls 1, 1, 3, 2, 4, 5 stays inside the
    cap."""
    scene = scenes.scene_07()
    w, h, ks = 48, 27, (1, 1, 3, 2, 4, 5)
    var, mean = [], []
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_scene(scene)
        r.set_moments(True)
        for _ in range(64):
            r.reset_accumulation()
            for k in ks:
                r.render(w, h, k, 4)
            v, m = r.variance(h, w, want_lum=True)
            var.append(v.astype(np.float64))
            mean.append(m.astype(np.float64))
    ratio = float(np.mean(var, 0).sum() / np.var(mean, 0, ddof=1).sum())
    print(f"R = {ratio:.4f}")
    assert 0.5 < ratio < 2.0


def test_cli_moments_and_var_aov(tmp_path):
    out, prefix = tmp_path / "img.ppm", tmp_path / "f"
    base = [CLI, "--cpu", "2", "--width", "64", "--height", "36", "--frames", "4", "--max-bounces", "3"]
    res = subprocess.run(base + ["--out", str(out), "--moments", "--aov", str(prefix)],
                         check=True, capture_output=True, text=True)
    assert "moments: 4 batches" in res.stdout
    var = tmp_path / "f_var.ppm"
    assert var.stat().st_size == out.stat().st_size
    assert var.read_bytes() != out.read_bytes()
    plain = tmp_path / "plain.ppm"
    subprocess.run(base + ["--out", str(plain)], check=True, capture_output=True)
    assert plain.read_bytes() == out.read_bytes()  # tracking changes no pixel
    # one render call holds one batch: no variance
    res = subprocess.run(base + ["--frames-per-call", "4", "--moments", "--aov", str(prefix)],
                         capture_output=True, text=True)
    assert res.returncode != 0 and "rt_get_variance" in res.stderr
