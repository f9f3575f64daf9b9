"""The variance-guided a-trous filter on the MI355X: the HIP kernels (both
level variants) against the CPU backend, bit for bit in colour, variance and
RGBA (both run the arithmetic of csrc/rt_denoise_var.h), the device-stream entry
point, and neutrality.  The GPU context renders (and tracks); the CPU context
renders the same frames from the same seeds.
"""
import numpy as np
import pytest

from bwrt import Renderer, scenes
from test_denoise_var import (SIGMA, SKY, accumulate, neutrality_sequence, passes, same_results, same_sequences,
                              special_frame)

pytestmark = pytest.mark.gpu

MODES = {"tracked": 2, "spatial": 9}  # min_batches against the 8 tracked batches


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def tracked_frame(r, scene, w, h, calls=8):
    r.set_scene(scene)
    r.set_background(*SKY)
    r.init_rand(w, h)  # the seeds: both backends render the same frames
    img, acc = accumulate(r, w, h, calls=calls)
    assert r.moments_batches == calls
    return img


def results(r, w, h, levels):
    return {(m, it): r.denoise_var(w, h, want_color=True, want_var=True, iterations=it, min_batches=mb, sigma_lum=SIGMA)
            for m, mb in MODES.items() for it in levels}


@pytest.fixture(scope="module")
def cpu07(bwrt_lib):
    """Scene 07 under the sky, 67x45, 8 tracked one-frame calls on the CPU
    backend: the raw RGBA and every (mode, level count) result, computed once."""
    with Renderer.cpu(0, lib=bwrt_lib) as c:
        img = tracked_frame(c, scenes.scene_07(), 67, 45)
        yield img, results(c, 67, 45, range(0, 7))


@pytest.mark.parametrize("variant", ["direct", "tiled"])
def test_filter_equals_cpu_every_level_count(monkeypatch, bwrt_lib, cpu07, variant):
    img, want = cpu07
    monkeypatch.setenv("BWRT_DENOISE_KERNEL", variant)  # read at rt_create (BWRT_TUNING=1)
    with Renderer(0, lib=bwrt_lib) as r:
        assert np.array_equal(tracked_frame(r, scenes.scene_07(), 67, 45), img)
        got = results(r, 67, 45, range(0, 7))
        assert r.last_denoise_var_ms() > 0
    for key in want:
        for g, c in zip(got[key], want[key]):
            assert same(g, c), (variant, key)
    assert np.array_equal(want["tracked", 0][0], img)  # iterations == 0: the render's RGBA
    assert not same(want["tracked", 5][1], want["spatial", 5][1])


@pytest.fixture(scope="module")
def cpu_row(bwrt_lib):
    """test_denoise_var.passes: the four passes in a row on the CPU backend."""
    return passes(lambda: Renderer.cpu(0, lib=bwrt_lib), range(4))


@pytest.mark.parametrize("variant", ["direct", "tiled"])
def test_passes_carry_nothing_over(monkeypatch, bwrt_lib, cpu_row, variant):
    """rt_denoise, rt_denoise_var, rt_temporal with the default filter and
    rt_denoise again on one context: the CPU backend's bits (each of which
    equals the call made alone, tests/test_denoise_var.py), so the shared colour
    buffers and guides carry nothing from one pass to the next."""
    monkeypatch.setenv("BWRT_DENOISE_KERNEL", variant)
    row = passes(lambda: Renderer(0, lib=bwrt_lib), range(4))
    for i, (g, c) in enumerate(zip(row, cpu_row)):
        assert same_results(g, c), (variant, i)
    assert same_results(row[0], row[3])


@pytest.mark.parametrize("variant", [None, "direct", "tiled"])
@pytest.mark.parametrize("w,h", [(333, 187), (5, 3), (1, 1)])
def test_filter_equals_cpu_shapes(monkeypatch, bwrt_lib, variant, w, h):
    if variant:
        monkeypatch.setenv("BWRT_DENOISE_KERNEL", variant)
    scene = scenes.scene_07()
    with Renderer(0, lib=bwrt_lib) as r, Renderer.cpu(0, lib=bwrt_lib) as c:
        assert np.array_equal(tracked_frame(r, scene, w, h), tracked_frame(c, scene, w, h))
        got, want = results(r, w, h, (5,)), results(c, w, h, (5,))
    for key in want:
        for g, x in zip(got[key], want[key]):
            assert same(g, x), (variant, key)


@pytest.mark.parametrize("variant", ["direct", "tiled"])
def test_filter_equals_cpu_special_values(monkeypatch, bwrt_lib, variant):
    monkeypatch.setenv("BWRT_DENOISE_KERNEL", variant)
    with Renderer(0, lib=bwrt_lib) as r, Renderer.cpu(0, lib=bwrt_lib) as c:
        scene, w, h, acc, (nan_px, inf_px) = special_frame(r)
        rng, acc = r.get_state(h, w)
        c.set_scene(scene)
        c.set_background(*SKY)
        c.init_rand(w, h)
        c.set_state(rng, acc, 5)
        g = r.denoise_var(w, h, want_color=True, want_var=True, iterations=4, sigma_lum=SIGMA)
        x = c.denoise_var(w, h, want_color=True, want_var=True, iterations=4, sigma_lum=SIGMA)
    assert np.array_equal(g[0], x[0]) and same(g[1], x[1]) and same(g[2], x[2])
    assert np.isnan(g[1][nan_px]).all() and np.all(g[1][inf_px] == np.inf)
    bad = ~(np.isfinite(g[1]).all(-1) & np.isfinite(g[2]))
    bad[nan_px] = bad[inf_px] = False
    assert not bad.any()


def test_device_output_on_a_callers_stream(bwrt_lib):
    """A tracked render, the filter of its frame, a render and an rt_denoise
    queued back to back on a caller's stream, no host synchronisation between
    them."""
    import torch
    scene = scenes.scene_07()
    w, h = 160, 90
    with Renderer(0, lib=bwrt_lib) as gpu:
        gpu.set_scene(scene)
        gpu.set_background(*SKY)
        gpu.init_rand(w, h)
        gpu.set_moments(True)
        raw, buf, buf2 = (torch.zeros(h * w, dtype=torch.int32, device="cuda") for _ in range(3))
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()  # (the zero fills ran on torch's default stream, unordered with `stream`)
        s = stream.cuda_stream
        gpu.render_device(gpu.params(w, h, 2, 4, first_frame=1), raw.data_ptr(), s)
        gpu.render_device(gpu.params(w, h, 1, 4), raw.data_ptr(), s)
        gpu.denoise_var_device(buf.data_ptr(), s, min_batches=2)
        rng, acc = gpu.get_state(h, w)  # waits for the render; the frame the filter saw
        frame = gpu.frame_counter
        gpu.render_device(gpu.params(w, h, 1, 4), raw.data_ptr(), s)
        gpu.denoise_device(buf2.data_ptr(), s)
        stream.synchronize()
        got = buf.cpu().numpy().view(np.uint8).reshape(h, w, 4)
        assert gpu.last_denoise_var_ms() > 0
        want2 = gpu.denoise(w, h)  # the 4-frame state through the host path
        assert np.array_equal(buf2.cpu().numpy().view(np.uint8).reshape(h, w, 4), want2)
    with Renderer.cpu(0, lib=bwrt_lib) as c:  # the same three tracked frames
        c.set_scene(scene)
        c.set_background(*SKY)
        c.init_rand(w, h)
        c.set_moments(True)
        c.render(w, h, 2, 4, first_frame=1)
        raw3 = c.render(w, h, 1, 4)
        assert c.frame_counter == frame and same(c.get_state(h, w)[1], acc)
        want = c.denoise_var(w, h, min_batches=2)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, raw3)


def test_repeated_calls_give_identical_bits(bwrt_lib):
    with Renderer(0, lib=bwrt_lib) as r:
        tracked_frame(r, scenes.scene_07(), 333, 187)
        for mb in MODES.values():
            first = r.denoise_var(333, 187, want_color=True, want_var=True, min_batches=mb)
            for _ in range(4):
                again = r.denoise_var(333, 187, want_color=True, want_var=True, min_batches=mb)
                assert all(same(a, b) for a, b in zip(first, again))


def test_precision_mode_does_not_reach_the_filter(bwrt_lib, cpu07):
    img, want = cpu07
    with Renderer(0, lib=bwrt_lib) as r:
        tracked_frame(r, scenes.scene_07(), 67, 45)  # exact frames
        r.set_precision("fast")
        got = r.denoise_var(67, 45, want_color=True, want_var=True, iterations=5, min_batches=2, sigma_lum=SIGMA)
    assert all(same(g, c) for g, c in zip(got, want["tracked", 5]))


def test_neutrality(bwrt_lib):
    scene = scenes.scene_07()
    runs = []
    for track in (True, False):
        with Renderer(0, lib=bwrt_lib) as r:
            runs.append(neutrality_sequence(r, scene, 67, 45, track))
    same_sequences(*runs)
