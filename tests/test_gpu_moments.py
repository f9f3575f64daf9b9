"""Luminance moment tracking on the MI355X: the update kernel behind every
render-kernel family against the CPU backend, bit for bit (both run the
arithmetic of csrc/rt_moments.h over bit-identical frameSums), on the context's
and on a caller's stream, and its neutrality.
"""
import numpy as np
import pytest

from bwrt import Renderer, scenes
from test_moments import BATCHES, neutrality_sequence

pytestmark = pytest.mark.gpu


def run(r, scene, w, h, bounces, batches=BATCHES, kernel=None, **shard):
    """Reseed, tracking on, one render call per batch; the variance readout.
    `kernel`: the family every call must have launched (GPU contexts)."""
    r.set_scene(scene)
    r.init_rand(w, h, shard.get("row_offset", 0), shard.get("row_stride", 1))
    r.set_moments(True)
    for i, k in enumerate(batches):
        r.render(w, h, k, bounces, first_frame=1 if i == 0 else 0, **shard)
        if kernel:
            assert r.last_kernel_name().startswith(kernel), r.last_kernel_name()
    rows = len(range(shard.get("row_offset", 0), h, shard.get("row_stride", 1)))
    return (r.moments_batches,) + r.variance(rows, w, want_lum=True) + r.get_state(rows, w)


def same_run(a, b):
    assert a[0] == b[0] == 4
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y, equal_nan=True)
    assert (a[1] > 0).any()


# the launch policy gives a small frame to the pair kernel when a call holds
# samples * (bounces + 1) >= 8 queries per pixel (batches of 2 frames and more
# at 4 bounces), and frames above 1400 pixels per CU (256 CUs: 358,400) to the
# sorted kernel
@pytest.mark.parametrize("name,w,h,bounces,batches,shard,kernel", [
    ("07", 67, 45, 4, (2, 2, 3, 2), {}, "rt_render_pair_kernel<"),
    ("07", 67, 45, 4, BATCHES, {}, None),
    ("07", 333, 187, 4, BATCHES, {}, None),
    ("07", 67, 45, 4, BATCHES, {"row_offset": 1, "row_stride": 3}, None),
    ("07", 333, 187, 4, BATCHES, {"row_offset": 1, "row_stride": 3}, None),
    ("07", 800, 450, 4, BATCHES, {}, "rt_render_sorted_kernel<"),
    ("stress", 96, 54, 8, BATCHES, {}, "rt_render_bvh_refill_kernel<"),
])
def test_moments_equal_cpu(bwrt_lib, name, w, h, bounces, batches, shard, kernel):
    scene = scenes.SCENES[name]()
    with Renderer(0, lib=bwrt_lib) as g:
        got = run(g, scene, w, h, bounces, batches, kernel=kernel, **shard)
    with Renderer.cpu(0, lib=bwrt_lib) as c:
        want = run(c, scene, w, h, bounces, batches, **shard)
    same_run(got, want)


@pytest.mark.parametrize("own_stream", [False, True])
def test_render_device_back_to_back(bwrt_lib, own_stream):
    """Every batch through rt_render_device with the next render queued
    directly behind: on a caller's stream, and on the context's own stream
    (whose renders record no event between them)."""
    import torch
    scene = scenes.scene_07()
    w, h = 67, 45
    with Renderer(0, lib=bwrt_lib) as g:
        g.set_scene(scene)
        g.init_rand(w, h)
        g.set_moments(True)
        buf = torch.zeros(h * w, dtype=torch.int32, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        sp = None if own_stream else stream.cuda_stream
        for i, k in enumerate(BATCHES):
            g.render_device(g.params(w, h, k, 4, first_frame=1 if i == 0 else 0), buf.data_ptr(), sp)
        assert g.moments_batches == len(BATCHES)
        got = (g.moments_batches,) + g.variance(h, w, want_lum=True) + g.get_state(h, w)  # waits for the renders
        stream.synchronize()
    with Renderer.cpu(0, lib=bwrt_lib) as c:
        want = run(c, scene, w, h, 4)
    same_run(got, want)


def test_streams_alternate(bwrt_lib):
    """Batches alternating between a caller's stream and the context's: each
    update is ordered after the previous one on the other stream."""
    import torch
    scene = scenes.scene_07()
    w, h = 333, 187
    with Renderer(0, lib=bwrt_lib) as g:
        g.set_scene(scene)
        g.init_rand(w, h)
        g.set_moments(True)
        buf = torch.zeros(h * w, dtype=torch.int32, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        for i, k in enumerate(BATCHES):
            g.render_device(g.params(w, h, k, 4, first_frame=1 if i == 0 else 0), buf.data_ptr(),
                            stream.cuda_stream if i % 2 == 0 else None)
        got = (g.moments_batches,) + g.variance(h, w, want_lum=True) + g.get_state(h, w)
        stream.synchronize()
    with Renderer.cpu(0, lib=bwrt_lib) as c:
        want = run(c, scene, w, h, 4)
    same_run(got, want)


def test_neutrality(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 67, 45
    runs = []
    for track in (True, False):
        with Renderer(0, lib=bwrt_lib) as r:
            runs.append(neutrality_sequence(r, scene, w, h, track))
    for on, off in zip(*runs):
        assert np.array_equal(on[0], off[0])  # RGBA
        assert on[1] == off[1]  # frame counter
        assert np.array_equal(on[2], off[2])  # RNG state
        assert np.array_equal(on[3], off[3], equal_nan=True)  # frameSum
