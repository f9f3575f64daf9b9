"""Adaptive sampling on the MI355X against the CPU backend, bit for bit: the
selection kernels, both list render kernels, the moment update and the resolve
pass run the arithmetic of csrc/rt_adaptive.h and csrc/rt_path.h over
bit-identical state, so counts, frameSum, RNG state, RGBA, moments and
statistics all agree exactly (tests/test_adaptive.py checks the CPU backend
against uniform renders and float64).
"""
import ctypes as C

import numpy as np
import pytest

from bwrt import Renderer, abi, scenes
import lifecycle_trace
import view_trace
from test_adaptive import DEFAULTS, KS, RESTARTS, START, adaptive_sequence, refused_after_restart, start

pytestmark = pytest.mark.gpu

KEYS = ("n", "j", "rng", "accum", "rgba", "color", "var", "lum")


def same(got, want):
    assert got["stats"] == want["stats"]
    for key in KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    for a, b in zip(got["took"], want["took"]):
        assert np.array_equal(a, b)


def both(lib, scene, w, h, bounces, kernel=None, spp=1, **kw):
    """The same sequence on a GPU and on a CPU context; `kernel`: what the
    name of the list render kernel must contain."""
    with Renderer(0, lib=lib) as g:
        g.set_samples_per_pixel(spp)
        got = adaptive_sequence(g, scene, w, h, bounces, **kw)
        name = g.last_kernel_name()
    with Renderer.cpu(0, lib=lib) as c:
        c.set_samples_per_pixel(spp)
        want = adaptive_sequence(c, scene, w, h, bounces, **kw)
    same(got, want)
    if kernel:
        assert kernel in name, name
    return got, name


# the three replay sequences, the larger frames (800x450: the smallest full frame
# the launch policy gives the sorted kernel) and the smallest ones
@pytest.mark.parametrize("name,w,h,bounces,kernel", [
    ("07", 67, 45, 4, "rt_render_list_kernel<256>"),
    ("04_box", 64, 36, 3, "rt_render_list_kernel<256>"),
    ("stress", 96, 54, 8, "rt_render_kernel<256,hit_global,bvh,list>"),
    ("07", 333, 187, 4, "rt_render_list_kernel<256"),
    ("07", 800, 450, 4, "rt_render_list_kernel<256"),
    ("07", 5, 3, 4, "rt_render_list_kernel<256>"),
    ("07", 1, 1, 4, "rt_render_list_kernel<256>"),
])
def test_sequences_equal_cpu(bwrt_lib, name, w, h, bounces, kernel):
    got, _ = both(bwrt_lib, scenes.SCENES[name](), w, h, bounces, kernel=kernel)
    if w * h > 100:
        assert 0 < got["stats"][0][0] < w * h


# deep paths take the small-block and the global-record choices of the policy
@pytest.mark.parametrize("bounces,kernel", [
    (0, "rt_render_list_kernel<256>"),
    (1, "rt_render_list_kernel<256>"),
    (12, "rt_render_list_kernel<256,grec>"),
    (32, "rt_render_list_kernel<64,grec>"),
])
def test_max_bounces(bwrt_lib, bounces, kernel):
    both(bwrt_lib, scenes.scene_07(), 67, 45, bounces, kernel=kernel)


def test_guard_scene(bwrt_lib):
    """The scene on which the reference's isnan(g) guard (Main.cu:139) decides
    half the pixels (scenegen.guard_scene; tests/test_reference_text.py pins the
    CPU backend on it to the reference's own text): a list kernel that lost the
    guard would leave NaN in frameSum where the CPU backend has none."""
    from scenegen import guard_scene
    got, _ = both(bwrt_lib, guard_scene(), 160, 90, 4, kernel="rt_render_list_kernel<256")
    assert np.isfinite(got["accum"]).all()
    assert got["stats"][0][0] > 0  # the list kernels did run


def test_samples_per_pixel(bwrt_lib):
    both(bwrt_lib, scenes.scene_07(), 67, 45, 4, kernel="rt_render_kernel<256,list>", spp=2)


# the one-path-per-lane list kernel's other instantiations (samplesPerPixel 2
# takes it whatever the scene): 64-lane groups from 16 bounces on (the record
# stack of 256 lanes passes 48 KB), the hit table in global memory, both on the BVH
@pytest.mark.parametrize("name,w,h,bounces,kernel", [
    ("07", 67, 45, 16, "rt_render_kernel<64,list>"),
    ("big", 24, 16, 4, "rt_render_kernel<256,hit_global,list>"),
    ("big", 24, 16, 16, "rt_render_kernel<64,hit_global,list>"),
    ("stress", 96, 54, 16, "rt_render_kernel<64,hit_global,bvh,list>"),
])
def test_simple_kernel_instantiations(bwrt_lib, monkeypatch, name, w, h, bounces, kernel):
    if name == "big":  # 408 primitives, no BVH: over 16 KB of hit table
        monkeypatch.setenv("BWRT_BVH_MIN", "100000000")
        scene = scenes.stress_scene(n_triangles=400, n_spheres=8)
    else:
        scene = scenes.SCENES[name]()
    got, got_name = both(bwrt_lib, scene, w, h, bounces, spp=2)
    assert got_name == kernel
    assert got["stats"][0][0] > 0  # the list kernel did run


def test_forced_kernels_equal_the_policy(bwrt_lib, monkeypatch):
    scene = scenes.scene_07()
    w, h, mb = 67, 45, 4
    runs = {}
    for which, kernel in ((None, "rt_render_list_kernel<256>"), ("simple", "rt_render_kernel<256,list>"),
                          ("queued", "rt_render_list_kernel<256>")):
        if which:
            monkeypatch.setenv("BWRT_ADAPTIVE_KERNEL", which)
        with Renderer(0, lib=bwrt_lib) as g:
            runs[which] = adaptive_sequence(g, scene, w, h, mb)
            assert g.last_kernel_name() == kernel
    same(runs["simple"], runs[None])
    same(runs["queued"], runs[None])
    monkeypatch.setenv("BWRT_ADAPTIVE_KERNEL", "queued")  # no queued kernel for BVH scenes: the policy holds
    with Renderer(0, lib=bwrt_lib) as g:
        adaptive_sequence(g, scenes.SCENES["stress"](), 48, 27, 3, ks=(1,))
        assert g.last_kernel_name() == "rt_render_kernel<256,hit_global,bvh,list>"


def exact_list(r, scene, w, h, mb, size, tol):
    """A list of exactly `size` pixels made with min_frames / max_frames after
    calls that split the counts: the first call (radius 0, `tol`) takes `size`
    pixels to 9 frames, the second forces every other pixel to 10, the third
    selects the pixels below 10.  Returns per call (selected, counts, state)."""
    start(r, scene, w, h, mb)
    out = []
    calls = ([dict(samples=1, tolerance=tol, lum_floor=0.01, radius=0),
              dict(samples=2, tolerance=1e30, min_frames=9),
              dict(samples=3, tolerance=1e30, min_frames=10)] if size else
             [dict(samples=3, tolerance=0.1, max_frames=1)])
    for p in calls:
        img, st = r.render_adaptive(w, h, mb, **p)
        out.append((st["selected"], st["frames_total"], r.counts(h, w), r.get_state(h, w), img,
                    r.variance(h, w, want_lum=True)))
    return out


@pytest.mark.parametrize("size", [0, 1, 64, 65, 256])
def test_list_of_exactly(bwrt_lib, size):
    scene = scenes.scene_07()
    w, h, mb = 67, 45, 4
    with Renderer.cpu(0, lib=bwrt_lib) as c:
        tol = 0.1
        if size:
            # radius 0: pixel p is hot when sqrt(v_p) / (M_p + floor) > tolerance; a
            # tolerance between the size-th and the next largest ratio takes `size` pixels
            start(c, scene, w, h, mb)
            var, M = c.variance(h, w, want_lum=True)
            ratio = np.sort((np.sqrt(var.astype(np.float64)) / (M.astype(np.float64) + np.float32(0.01))).ravel())[::-1]
            assert ratio[size] > 0 and ratio[size - 1] > ratio[size] * (1 + 1e-5)  # a gap float32 resolves
            tol = float(np.float32(0.5 * (ratio[size - 1] + ratio[size])))
        want = exact_list(c, scene, w, h, mb, size, tol)
    assert [x[0] for x in want] == ([size, w * h - size, size] if size else [0])
    with Renderer(0, lib=bwrt_lib) as g:
        got = exact_list(g, scene, w, h, mb, size, tol)
    for a, b in zip(got, want):
        assert a[:2] == b[:2]
        for x, y in zip(a[2] + a[3] + (a[4],) + a[5], b[2] + b[3] + (b[4],) + b[5]):
            assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("own_stream", [False, True])
def test_device_entry_point(bwrt_lib, own_stream):
    """rt_render_adaptive_device with an rt_render_device queued directly before
    it, a second adaptive call and a restarting render (first_frame 1) directly
    behind it, on a caller's stream and on the context's own."""
    import torch
    scene = scenes.scene_07()
    w, h, mb = 67, 45, 4
    with Renderer.cpu(0, lib=bwrt_lib) as c:
        start(c, scene, w, h, mb)
        for k in (3, 2):
            img_want, _ = c.render_adaptive(w, h, mb, samples=k, **DEFAULTS)
        mid = c.counts(h, w) + c.get_state(h, w) + c.variance(h, w, want_lum=True)
        stats_want = c.adaptive_stats()
        restart_want = c.render(w, h, 2, mb, first_frame=1)
        end = c.counts(h, w) + c.get_state(h, w)
    with Renderer(0, lib=bwrt_lib) as g:
        g.set_scene(scene)
        g.init_rand(w, h)
        g.set_moments(True)
        buf = torch.zeros(h * w, dtype=torch.int32, device="cuda")
        buf2 = torch.zeros(h * w, dtype=torch.int32, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        sp = None if own_stream else stream.cuda_stream
        for i, k in enumerate(START):
            g.render_device(g.params(w, h, k, mb, first_frame=1 if i == 0 else 0), buf.data_ptr(), sp)
        g.render_adaptive_device(buf.data_ptr(), sp, mb, samples=3, **DEFAULTS)
        g.render_adaptive_device(buf.data_ptr(), sp, mb, samples=2, **DEFAULTS)
        # (a second pair of sequences checks the state between the adaptive calls and the restart)
        got_mid = g.counts(h, w) + g.get_state(h, w) + g.variance(h, w, want_lum=True)  # waits for the calls
        st = g.adaptive_stats()
        assert (st["selected"], st["frames_total"]) == (stats_want["selected"], stats_want["frames_total"])
        assert st["render_ms"] > 0 and st["select_ms"] > 0 and st["resolve_ms"] > 0
        img_mid = buf.cpu().numpy().view(np.uint8).reshape(h, w, 4)
        g.render_adaptive_device(buf.data_ptr(), sp, mb, samples=1, tolerance=1e30)  # selects nothing
        g.render_device(g.params(w, h, 2, mb, first_frame=1), buf2.data_ptr(), sp)  # directly behind: restarts
        got_end = g.counts(h, w) + g.get_state(h, w)
        g.synchronize()
        stream.synchronize()
        img_end = buf2.cpu().numpy().view(np.uint8).reshape(h, w, 4)
    for x, y in zip(got_mid, mid):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(img_mid, img_want)
    for x, y in zip(got_end, end):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(img_end, restart_want)


def test_five_identical_sequences(bwrt_lib):
    scene = scenes.scene_07()
    with Renderer(0, lib=bwrt_lib) as g:
        runs = [adaptive_sequence(g, scene, 333, 187, 4) for _ in range(5)]
    for other in runs[1:]:
        same(other, runs[0])


def test_unselecting_call_is_neutral(bwrt_lib):
    scene = scenes.scene_07()
    w, h, mb = 67, 45, 4
    with Renderer(0, lib=bwrt_lib) as g:
        start(g, scene, w, h, mb)
        last = g.render(w, h, 1, mb)
        before = g.get_state(h, w) + g.variance(h, w, want_lum=True)
        img, st = g.render_adaptive(w, h, mb, samples=5, tolerance=1e30)
        assert st["selected"] == 0 and st["frames_total"] == 9 * w * h
        assert np.array_equal(img, last)
        for x, y in zip(before, g.get_state(h, w) + g.variance(h, w, want_lum=True)):
            assert np.array_equal(x, y, equal_nan=True)
        n, j = g.counts(h, w)
        assert (n == 9).all() and (j == 5).all()


def test_errors_and_state_on_the_gpu(bwrt_lib):
    lib = bwrt_lib
    scene = scenes.scene_07()
    w, h, mb = 67, 45, 4
    with Renderer(0, lib=lib) as g:
        start(g, scene, w, h, mb)
        d = g.adaptive_params()
        g.set_precision("fast")
        assert lib.rt_render_adaptive(g.ctx, C.byref(d), mb, None, None, None) == abi.RT_ERR_UNSUPPORTED
        assert lib.rt_render_adaptive_device(g.ctx, C.byref(d), mb, None, None) == abi.RT_ERR_UNSUPPORTED
        g.set_precision("exact")
        assert lib.rt_render_adaptive_device(g.ctx, C.byref(d), mb, 2, None) == abi.RT_ERR_INVALID_ARGUMENT  # alignment
        g.render_adaptive(w, h, mb)
        p = g.params(w, h, 1, mb)
        assert lib.rt_render_ex(g.ctx, C.byref(p), None, None) == abi.RT_ERR_UNSUPPORTED
        assert lib.rt_render_device(g.ctx, C.byref(p), None, None) == abi.RT_ERR_UNSUPPORTED
        dn = g.denoise_params()
        assert lib.rt_denoise(g.ctx, C.byref(dn), None, None) == abi.RT_ERR_UNSUPPORTED
        assert lib.rt_denoise_device(g.ctx, C.byref(dn), None, None) == abi.RT_ERR_UNSUPPORTED
        arr = (C.c_void_p * 1)(g.ctx.value)
        assert lib.rt_render_multi(arr, 1, w, h, 1, None) == abi.RT_ERR_UNSUPPORTED
        assert g.frame_counter == 9 and g.moments_batches == 4
        g.render(w, h, 2, mb, first_frame=1)  # ends the state
        g.render(w, h, 2, mb)
        assert lib.rt_denoise(g.ctx, C.byref(dn), None, None) == abi.RT_OK


@pytest.mark.parametrize("own_stream", [False, True])
def test_device_call_refused_after_a_restart(bwrt_lib, own_stream):
    """tests/test_adaptive.py's case for rt_render_adaptive_device, from the
    tracked uniform and from the non-uniform state."""
    import torch
    lib = bwrt_lib
    stream = torch.cuda.Stream()
    sp = None if own_stream else stream.cuda_stream
    for i, restart in enumerate(sorted(RESTARTS)):
        refused_after_restart(lib, lambda: Renderer(0, lib=lib), restart, bool(i & 1),
                              lambda r, d: lib.rt_render_adaptive_device(r.ctx, C.byref(d), 2, None, sp))
    stream.synchronize()


def test_lifecycle_trace_equals_cpu(bwrt_lib):
    """The seeded call sequences of tests/lifecycle_trace.py through launch(),
    the GPU adaptive call and the device readbacks: every record equals the CPU
    context's of the same library."""
    for seed in lifecycle_trace.SEEDS:
        got = lifecycle_trace.trace(bwrt_lib, seed, gpu=True)
        want = lifecycle_trace.trace(bwrt_lib, seed)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, (seed, i)


def test_view_trace_equals_cpu(bwrt_lib):
    """The seeded call sequences of tests/view_trace.py (views, the temporal
    history sets, the assembled frame of a shard context) on a GPU context:
    every record equals the CPU context's of the same library."""
    for seed in view_trace.SEEDS:
        got = view_trace.trace(bwrt_lib, seed, gpu=True)
        want = view_trace.trace(bwrt_lib, seed)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, (seed, i)
        assert len(got) == len(want) == view_trace.STEPS
