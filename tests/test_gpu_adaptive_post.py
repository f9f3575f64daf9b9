"""The denoisers and the reprojection on a non-uniform accumulation
(rt_set_adaptive_filters) on the MI355X against the CPU backend, bit for bit:
the count-aware kernels (level 0 of rt_denoise in both shapes and its
conversion pass, the input stage of rt_denoise_var, the reprojection) run the
arithmetic of csrc/rt_atrous.h, rt_denoise.h, rt_denoise_var.h and
rt_temporal.h over bit-identical state (tests/test_gpu_adaptive.py), so RGBA,
colour, variance and history length all agree exactly
(tests/test_adaptive_post.py checks the CPU backend against the uniform passes
and float64).
"""
import ctypes as C

import numpy as np
import pytest

import adaptive_post_ref as A
from bwrt import Renderer, abi, scenes
from test_adaptive import DEFAULTS, START, start

pytestmark = pytest.mark.gpu

VARIANTS = [None, "direct", "tiled"]  # BWRT_DENOISE_KERNEL (read at rt_create under BWRT_TUNING=1)
MIN_BATCHES = (4, 6)  # replay: all tracked / J_p 4..7 split; mixed: J_p 2 and 4 split / all spatial


def sequence(r, kind, w, h, mb, iterations):
    """The frame of test 3 (`replay`) or test 4 (`mixed`) of
    tests/test_adaptive_post.py, then every pass on it."""
    scene = scenes.scene_07()
    if kind == "replay":
        A.replay_state(r, scene, w, h, mb)
    else:
        A.mixed_state(r, scene, w, h, mb)
    out = A.all_passes(r, w, h, iterations=iterations, min_batches=MIN_BATCHES)
    out["counts"] = r.counts(h, w)
    return out


_CPU = {}


def cpu_sequence(lib, kind, w, h, mb, iterations):
    """The CPU backend's results, computed once per case and kept unchanged."""
    key = (kind, w, h, mb, iterations)
    if key not in _CPU:
        with Renderer.cpu(0, lib=lib) as c:
            _CPU[key] = sequence(c, kind, w, h, mb, iterations)
        for t in _CPU[key].values():
            for a in t:
                a.setflags(write=False)
    return _CPU[key]


def gpu_equals_cpu(monkeypatch, lib, variant, kind, w, h, mb, iterations):
    if variant:
        monkeypatch.setenv("BWRT_DENOISE_KERNEL", variant)
    with Renderer(0, lib=lib) as g:
        got = sequence(g, kind, w, h, mb, iterations)
    want = cpu_sequence(lib, kind, w, h, mb, iterations)
    A.same_pass_results(got, want)
    return want


# 67x45 at 6 levels: step 32 exceeds the height, so the tiled kernel's phases run past the frame
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", ["replay", "mixed"])
def test_sequences_equal_cpu(monkeypatch, bwrt_lib, variant, kind):
    want = gpu_equals_cpu(monkeypatch, bwrt_lib, variant, kind, 67, 45, 4, A.ITERATIONS)
    n, j = want["counts"]
    assert len(np.unique(n)) >= 3
    split = j >= (6 if kind == "replay" else 4)
    assert 0.05 < split.mean() < 0.95  # one frame, both variance sources
    assert not np.array_equal(want["dv", 5, 4][2], want["dv", 5, 6][2])


# width not a multiple of 64 with ragged tile rows; frames smaller than a window
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("w,h", [(333, 187), (5, 3), (1, 1)])
@pytest.mark.parametrize("kind", ["replay", "mixed"])
def test_shapes_equal_cpu(monkeypatch, bwrt_lib, variant, kind, w, h):
    want = gpu_equals_cpu(monkeypatch, bwrt_lib, variant, kind, w, h, 4, (0, 5))
    if w * h > 100:
        assert len(np.unique(want["counts"][0])) >= 3


@pytest.mark.parametrize("variant", ["direct", "tiled"])
def test_max_bounces_0(monkeypatch, bwrt_lib, variant):
    gpu_equals_cpu(monkeypatch, bwrt_lib, variant, "mixed", 67, 45, 0, (0, 5))


def two_views(r, w, h, mb):
    """Both views non-uniform at their temporal calls; the second has a history
    of per-pixel lengths."""
    scene = scenes.scene_07()
    A.first_view(r, scene, w, h, mb)
    out = []
    for view in (0, 1):
        for k in (3, 1):
            r.render_adaptive(w, h, mb, samples=k, **DEFAULTS)
        out.append(A.all_passes(r, w, h, iterations=(5,)))
        if view == 0:
            A.second_view(r, scene, w, h, mb)
    return out


def test_temporal_with_history_equals_cpu(bwrt_lib):
    w, h, mb = 67, 45, 4
    with Renderer(0, lib=bwrt_lib) as g, Renderer.cpu(0, lib=bwrt_lib) as c:
        got, want = two_views(g, w, h, mb), two_views(c, w, h, mb)
    for a, b in zip(got, want):
        A.same_pass_results(a, b)
    ln0, ln1 = want[0]["tp"][2], want[1]["tp"][2]
    assert len(np.unique(ln0)) >= 3 and (ln1 > ln0.max()).any()  # per-pixel lengths, then reprojected ones


@pytest.mark.parametrize("own_stream", [False, True])
def test_device_entry_points(bwrt_lib, own_stream):
    """The uniform start, two rt_render_adaptive_device calls and the three
    _device passes queued back to back, no host synchronisation in between, on
    a caller's stream and on the context's own: the filters must be ordered
    behind the adaptive call's update and resolve passes."""
    import torch
    scene = scenes.scene_07()
    w, h, mb = 160, 90, 4
    with Renderer.cpu(0, lib=bwrt_lib) as c:
        start(c, scene, w, h, mb)
        c.set_adaptive_filters(True)
        for k in (3, 2):
            raw = c.render_adaptive(w, h, mb, samples=k, **DEFAULTS)[0]
        want = (c.denoise(w, h), c.denoise_var(w, h, min_batches=6), c.temporal(w, h, denoise={}))
        counts = c.counts(h, w)
    assert 0.05 < (counts[1] >= 6).mean() < 0.95
    with Renderer(0, lib=bwrt_lib) as g:
        g.set_scene(scene)
        g.init_rand(w, h)
        g.set_moments(True)
        g.set_adaptive_filters(True)
        bufs = [torch.zeros(h * w, dtype=torch.int32, device="cuda") for _ in range(4)]
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()  # (the zero fills ran on torch's default stream, unordered with `stream`)
        sp = None if own_stream else stream.cuda_stream
        for i, k in enumerate(START):
            g.render_device(g.params(w, h, k, mb, first_frame=1 if i == 0 else 0), bufs[0].data_ptr(), sp)
        g.render_adaptive_device(bufs[0].data_ptr(), sp, mb, samples=3, **DEFAULTS)
        g.render_adaptive_device(bufs[0].data_ptr(), sp, mb, samples=2, **DEFAULTS)
        g.denoise_device(bufs[1].data_ptr(), sp)
        g.denoise_var_device(bufs[2].data_ptr(), sp, min_batches=6)
        g.temporal_device(bufs[3].data_ptr(), sp, denoise={})
        g.synchronize()
        stream.synchronize()
        got = [b.cpu().numpy().view(np.uint8).reshape(h, w, 4) for b in bufs]
        for x, y in zip(g.counts(h, w), counts):
            assert np.array_equal(x, y)
    assert np.array_equal(got[0], raw)
    for i, (x, y) in enumerate(zip(got[1:], want)):
        assert np.array_equal(x, y), i
        assert not np.array_equal(x, raw)


def test_five_identical_sequences(bwrt_lib):
    with Renderer(0, lib=bwrt_lib) as g:
        runs = [sequence(g, "mixed", 333, 187, 4, (5,)) for _ in range(5)]
    for other in runs[1:]:
        A.same_pass_results(other, runs[0])


def test_switch_on_the_gpu(bwrt_lib):
    lib = bwrt_lib
    w, h, mb = 67, 45, 4
    with Renderer(0, lib=lib) as g:
        assert g.adaptive_filters is False
        dn, dv, tp = g.denoise_params(), g.denoise_var_params(), g.temporal_params()
        calls = (lambda: lib.rt_denoise(g.ctx, C.byref(dn), None, None),
                 lambda: lib.rt_denoise_device(g.ctx, C.byref(dn), None, None),
                 lambda: lib.rt_denoise_var(g.ctx, C.byref(dv), None, None, None),
                 lambda: lib.rt_denoise_var_device(g.ctx, C.byref(dv), None, None),
                 lambda: lib.rt_temporal(g.ctx, C.byref(tp), None, None, None, None),
                 lambda: lib.rt_temporal_device(g.ctx, C.byref(tp), None, None, None))
        start(g, scenes.scene_07(), w, h, mb)
        g.render_adaptive(w, h, mb, samples=2, **DEFAULTS)
        for call in calls:
            assert call() == abi.RT_ERR_UNSUPPORTED
        g.set_adaptive_filters(True)
        for call in calls:
            assert call() == abi.RT_OK
        g.synchronize()
        p = g.params(w, h, 1, mb)
        assert lib.rt_render_device(g.ctx, C.byref(p), None, None) == abi.RT_ERR_UNSUPPORTED
        arr = (C.c_void_p * 1)(g.ctx.value)
        assert lib.rt_render_multi(arr, 1, w, h, 1, None) == abi.RT_ERR_UNSUPPORTED
        g.set_adaptive_filters(False)
        for call in calls:
            assert call() == abi.RT_ERR_UNSUPPORTED
