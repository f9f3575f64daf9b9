"""First-hit feature buffers and the a-trous denoiser on the MI355X: the HIP
kernels against the CPU backend, bit for bit (both run the arithmetic of
csrc/rt_path.h and csrc/rt_denoise.h), against the float64 reference
(tests/denoise_ref.py) and the oracle.  The GPU context renders; its state goes
to a CPU context through get_state / set_state.
"""
import numpy as np
import pytest

import denoise_ref as R
from bwrt import Renderer, scenes
from test_denoise import FILTER_BOUND, reference, rgba_within_1lsb, special_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cpu(bwrt_lib):
    r = Renderer.cpu(0, lib=bwrt_lib)
    yield r
    r.close()


def mirror(gpu_r, cpu_r, scene, w, h):
    """The GPU context's progressive state of a full w x h frame into cpu_r."""
    rng, acc = gpu_r.get_state(h, w)
    cpu_r.set_scene(scene)
    cpu_r.init_rand(w, h)
    cpu_r.set_state(rng, acc, gpu_r.frame_counter)
    return acc


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- feature buffers ---------------------------------------------------------
@pytest.mark.parametrize("name,w,h,off,stride", [
    ("07", 67, 45, 0, 1),
    ("07", 67, 45, 1, 3),
    ("04_box", 67, 45, 0, 1),   # quads
    ("stress", 99, 54, 0, 1),   # the wave-synchronous BVH walk with a partial last wave
])
def test_features_equal_cpu(gpu, cpu, name, w, h, off, stride):
    scene = scenes.SCENES[name]()
    gpu.set_scene(scene)
    cpu.set_scene(scene)
    g = gpu.render_aov(w, h, off, stride)
    c = cpu.render_aov(w, h, off, stride)
    for k in c:
        assert same(g[k], c[k]), k
    assert (c["prim"] >= 0).any()


# ---- the filter --------------------------------------------------------------
@pytest.fixture(scope="module")
def frame07(gpu, cpu):
    """Scene 07, 67x45, 4 frames on the GPU; the CPU context holds the same
    state.  The CPU results per level count are computed once."""
    scene = scenes.scene_07()
    w, h = 67, 45
    gpu.set_scene(scene)
    img = gpu.render(w, h, 4, 4, first_frame=1)
    acc = mirror(gpu, cpu, scene, w, h)
    rng, _ = gpu.get_state(h, w)
    want = {it: cpu.denoise(w, h, iterations=it, want_color=True) for it in range(0, 7)}
    return scene, w, h, img, acc, rng, want


def variant_renderer(monkeypatch, bwrt_lib, variant, scene, w, h, rng, acc, frame):
    if variant:
        monkeypatch.setenv("BWRT_DENOISE_KERNEL", variant)  # read at rt_create (BWRT_TUNING=1)
    r = Renderer(0, lib=bwrt_lib)
    r.set_scene(scene)
    r.init_rand(w, h)
    r.set_state(rng, acc, frame)
    return r


@pytest.mark.parametrize("variant", ["direct", "tiled"])
def test_filter_equals_cpu_every_level_count(monkeypatch, bwrt_lib, frame07, variant):
    scene, w, h, img, acc, rng, want = frame07
    r = variant_renderer(monkeypatch, bwrt_lib, variant, scene, w, h, rng, acc, 5)
    try:
        for it in range(0, 7):
            rgba, col = r.denoise(w, h, iterations=it, want_color=True)
            assert same(col, want[it][1]), (variant, it)
            assert np.array_equal(rgba, want[it][0]), (variant, it)
        assert np.array_equal(want[0][0], img)  # iterations == 0: the render's RGBA
        assert r.last_denoise_ms() > 0
    finally:
        r.close()


@pytest.mark.parametrize("variant", ["direct", "tiled"])
@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (64, 32), (65, 33)])
def test_filter_equals_cpu_shapes(monkeypatch, bwrt_lib, cpu, variant, w, h):
    scene = scenes.scene_07()
    monkeypatch.setenv("BWRT_DENOISE_KERNEL", variant)
    with Renderer(0, lib=bwrt_lib) as r:
        r.set_scene(scene)
        r.render(w, h, 2, 4, first_frame=1)
        mirror(r, cpu, scene, w, h)
        for it in (1, 6):
            g = r.denoise(w, h, iterations=it, want_color=True)
            c = cpu.denoise(w, h, iterations=it, want_color=True)
            assert np.array_equal(g[0], c[0]) and same(g[1], c[1]), (variant, it)


@pytest.mark.parametrize("variant", ["direct", "tiled"])
def test_filter_equals_cpu_special_values(monkeypatch, bwrt_lib, cpu, variant):
    monkeypatch.setenv("BWRT_DENOISE_KERNEL", variant)
    with Renderer(0, lib=bwrt_lib) as r:
        scene, w, h, acc, (nan_px, inf_px, huge_px) = special_frame(r)
        mirror(r, cpu, scene, w, h)
        g = r.denoise(w, h, iterations=4, want_color=True)
        c = cpu.denoise(w, h, iterations=4, want_color=True)
    assert np.array_equal(g[0], c[0]) and same(g[1], c[1])
    assert np.isnan(g[1][nan_px]).all() and np.all(g[1][inf_px] == np.inf)
    bad = ~np.isfinite(g[1]).all(-1)
    bad[nan_px] = bad[inf_px] = False
    assert not bad.any()


@pytest.fixture(scope="module")
def frame1080(gpu, cpu):
    scene = scenes.scene_07()
    w, h = 1920, 1080
    gpu.set_scene(scene)
    gpu.render(w, h, 2, 2, first_frame=1)
    acc = mirror(gpu, cpu, scene, w, h)
    rng, _ = gpu.get_state(h, w)
    return scene, w, h, acc, rng, cpu.denoise(w, h, iterations=5, want_color=True)


@pytest.mark.parametrize("variant", [None, "direct", "tiled"])
def test_filter_equals_cpu_1080p(monkeypatch, bwrt_lib, frame1080, variant):
    """The full grid at the headline size: the default variant choice and each
    forced variant."""
    scene, w, h, acc, rng, want = frame1080
    r = variant_renderer(monkeypatch, bwrt_lib, variant, scene, w, h, rng, acc, 3)
    try:
        rgba, col = r.denoise(w, h, iterations=5, want_color=True)
    finally:
        r.close()
    assert np.array_equal(rgba, want[0])
    assert same(col, want[1])


@pytest.mark.parametrize("iterations", [1, 3, 6])
def test_filter_against_float64(gpu, frame07, iterations):
    scene, w, h, img, acc, rng, want = frame07
    gpu.set_scene(scene)
    gpu.init_rand(w, h)
    gpu.set_state(rng, acc, 5)
    rgba, col = gpu.denoise(w, h, iterations=iterations, want_color=True)
    ref = reference(gpu, scene, w, h, acc, 4, iterations=iterations)
    assert R.rel_err(col, ref) <= FILTER_BOUND
    assert rgba_within_1lsb(rgba, ref)


def test_device_output_on_a_callers_stream(gpu):
    import torch
    scene = scenes.scene_07()
    w, h = 160, 90
    gpu.set_scene(scene)
    gpu.init_rand(w, h)
    raw = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    buf = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()  # (the zero fills ran on torch's default stream, unordered with `stream`)
    # a render and the denoise of its frame queued back to back, no host synchronisation between them
    gpu.render_device(gpu.params(w, h, 3, 4, first_frame=1), raw.data_ptr(), stream.cuda_stream)
    gpu.denoise_device(buf.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    got = buf.cpu().numpy().view(np.uint8).reshape(h, w, 4)
    want = gpu.denoise(w, h)  # the same frame through the host path, on the context's stream
    assert np.array_equal(got, want)
    assert not np.array_equal(got, raw.cpu().numpy().view(np.uint8).reshape(h, w, 4))
    assert gpu.last_denoise_ms() > 0
    # a render on the context's stream right after a denoise on the caller's is ordered after it
    gpu.denoise_device(buf.data_ptr(), stream.cuda_stream)
    img = gpu.render(w, h, 1, 4)
    stream.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint8).reshape(h, w, 4), want)
    assert img.shape == (h, w, 4)


def test_precision_mode_does_not_reach_the_denoiser(bwrt_lib, frame07):
    scene, w, h, img, acc, rng, want = frame07
    with Renderer(0, lib=bwrt_lib) as r:
        r.set_precision("fast")
        r.set_scene(scene)
        r.init_rand(w, h)
        r.set_state(rng, acc, 5)
        a = r.render_aov(w, h)
        rgba, col = r.denoise(w, h, iterations=5, want_color=True)
    assert np.array_equal(rgba, want[5][0]) and same(col, want[5][1])
    with Renderer.cpu(0, lib=bwrt_lib) as c:
        c.set_scene(scene)
        ca = c.render_aov(w, h)
    for k in ca:
        assert same(a[k], ca[k]), k


def test_state_is_untouched(bwrt_lib, oracle):
    scene = scenes.scene_07()
    w, h = 64, 36
    with Renderer(0, lib=bwrt_lib) as r:
        r.set_scene(scene)
        r.render(w, h, 2, 4, first_frame=1)
        rng0, acc0 = r.get_state(h, w)
        r.render_aov(w, h)
        r.denoise(w, h)
        rng1, acc1 = r.get_state(h, w)
        assert r.frame_counter == 3
        assert np.array_equal(rng0, rng1) and same(acc0, acc1)
        img = r.render(w, h, 2, 4)
        rng2, acc2 = r.get_state(h, w)
    st = oracle.OracleState(w, h)
    oracle.render(scene, st, 4, 4, first_frame=1)
    assert np.array_equal(img, st.rgba)
    assert same(acc2, st.accum)
    assert np.array_equal(rng2, st.rng)
