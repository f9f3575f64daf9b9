"""Next-event estimation on the MI355X: the HIP kernel of csrc/rt_kernel_nee.h
against the CPU backend, bit for bit (both run the arithmetic of csrc/rt_light.h
and csrc/rt_path.h): every render call's frameSum, RNG state and RGBA.
tests/test_light_sampling.py checks the estimator itself on the CPU backend.
"""
import ctypes as C

import numpy as np
import pytest

from bwrt import Renderer, abi, scenes
from test_adaptive import adaptive_sequence
from test_gpu_adaptive import same
from test_light_sampling import dark_07, state, same_state, triangle_light_scene

pytestmark = pytest.mark.gpu


def pair(lib, scene, w, h, mb, frames=3, calls=1, spp=1, kernel=None, on=True, **kw):
    """The same calls on a GPU and a CPU context with light sampling on."""
    with Renderer(0, lib=lib) as g:
        g.set_scene(scene)
        g.set_light_sampling(on)
        g.set_samples_per_pixel(spp)
        got = state(g, w, h, frames, mb, calls=calls, **kw)
        name = g.last_kernel_name()
        assert g.last_kernel_ms() > 0
    with Renderer.cpu(0, lib=lib) as c:
        c.set_scene(scene)
        c.set_light_sampling(on)
        c.set_samples_per_pixel(spp)
        want = state(c, w, h, frames, mb, calls=calls, **kw)
    same_state(got, want)
    if kernel is not None:
        assert name == kernel, name
    return got


@pytest.mark.parametrize("name,w,h,mb,kernel", [
    ("07", 67, 45, 4, "rt_render_nee_kernel<256>"),
    ("07", 333, 187, 4, "rt_render_nee_kernel<256>"),
    ("07", 5, 3, 4, "rt_render_nee_kernel<256>"),
    ("07", 1, 1, 4, "rt_render_nee_kernel<256>"),  # width / 2 == 0: the NaN camera ray
    ("04_box", 67, 45, 3, "rt_render_nee_kernel<256>"),  # quads, normals of length 200
    ("stress", 96, 54, 8, "rt_render_nee_kernel<256,hit_global,bvh>"),  # the BVH walk, 8 lights
    ("07", 67, 45, 0, None),  # no level can act: the default launch policy's kernel
    ("07", 67, 45, 1, "rt_render_nee_kernel<256>"),
    ("07", 67, 45, 11, "rt_render_nee_kernel<256>"),  # the last depth with 256 lanes: 48 KB of records
    ("07", 67, 45, 12, "rt_render_nee_kernel<64>"),
    ("07", 67, 45, 32, "rt_render_nee_kernel<64>"),
    ("stress", 48, 27, 32, "rt_render_nee_kernel<64,hit_global,bvh>"),
])
def test_renders_equal_cpu(bwrt_lib, name, w, h, mb, kernel):
    pair(bwrt_lib, scenes.SCENES[name](), w, h, mb, kernel=kernel)


def test_hit_table_in_global_memory(bwrt_lib, monkeypatch):
    monkeypatch.setenv("BWRT_BVH_MIN", "100000000")
    scene = scenes.stress_scene(n_triangles=400, n_spheres=8)  # 408 primitives: over 16 KB of hit table
    pair(bwrt_lib, scene, 24, 16, 4, kernel="rt_render_nee_kernel<256,hit_global>")
    pair(bwrt_lib, scene, 24, 16, 12, kernel="rt_render_nee_kernel<64,hit_global>")


def test_samples_per_pixel(bwrt_lib):
    pair(bwrt_lib, scenes.scene_07(), 67, 45, 4, spp=3, kernel="rt_render_nee_kernel<256>")


@pytest.mark.parametrize("off", [0, 1])
def test_row_shard(bwrt_lib, off):
    pair(bwrt_lib, scenes.scene_07(), 67, 45, 4, row_offset=off, row_stride=2, kernel="rt_render_nee_kernel<256>")


def test_continued_accumulation(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 67, 45
    res = {}
    for gpu in (True, False):
        with (Renderer(0, lib=bwrt_lib) if gpu else Renderer.cpu(0, lib=bwrt_lib)) as r:
            r.set_scene(scene)
            r.set_light_sampling(True)
            a = r.render(w, h, 3, 4, first_frame=1)
            b = r.render(w, h, 5, 4)
            assert r.frame_counter == 9
            res[gpu] = [a, b, *r.get_state(h, w)]
    same_state(res[True], res[False])


@pytest.mark.parametrize("make,mb", [(dark_07, 4), (triangle_light_scene, 4), (scenes.scene_07, 0)])
def test_identities_against_the_default_gpu_render(bwrt_lib, make, mb):
    """Empty light table and zero bounces: bit-identical to the default
    estimator's GPU render."""
    w, h = 67, 45
    res = []
    for on in (False, True):
        with Renderer(0, lib=bwrt_lib) as g:
            g.set_scene(make())
            g.set_light_sampling(on)
            res.append(state(g, w, h, 3, mb, calls=2))
    same_state(res[0], res[1])


@pytest.mark.parametrize("name,w,h,mb,kernel", [
    ("07", 67, 45, 4, "rt_render_nee_kernel<256,list>"),
    ("stress", 96, 54, 8, "rt_render_nee_kernel<256,hit_global,bvh,list>"),
])
def test_adaptive_calls_equal_cpu(bwrt_lib, name, w, h, mb, kernel):
    scene = scenes.SCENES[name]()
    with Renderer(0, lib=bwrt_lib) as g:
        g.set_light_sampling(True)
        got = adaptive_sequence(g, scene, w, h, mb)
        assert g.last_kernel_name() == kernel
    with Renderer.cpu(0, lib=bwrt_lib) as c:
        c.set_light_sampling(True)
        want = adaptive_sequence(c, scene, w, h, mb)
    same(got, want)
    assert 0 < got["stats"][0][0] < w * h


# the list instantiations the cases above do not reach: 64-lane groups (12
# bounces: the 4-dword record stack of 256 lanes passes 48 KB), the hit table in
# global memory (test_hit_table_in_global_memory's scene), both on the BVH
@pytest.mark.parametrize("name,w,h,mb,kernel", [
    ("07", 67, 45, 12, "rt_render_nee_kernel<64,list>"),
    ("stress", 96, 54, 12, "rt_render_nee_kernel<64,hit_global,bvh,list>"),
    ("big", 24, 16, 4, "rt_render_nee_kernel<256,hit_global,list>"),
    ("big", 24, 16, 12, "rt_render_nee_kernel<64,hit_global,list>"),
])
def test_adaptive_list_instantiations(bwrt_lib, monkeypatch, name, w, h, mb, kernel):
    if name == "big":
        monkeypatch.setenv("BWRT_BVH_MIN", "100000000")
        scene = scenes.stress_scene(n_triangles=400, n_spheres=8)
    else:
        scene = scenes.SCENES[name]()
    with Renderer(0, lib=bwrt_lib) as g:
        g.set_light_sampling(True)
        got = adaptive_sequence(g, scene, w, h, mb)
        assert g.last_kernel_name() == kernel
    with Renderer.cpu(0, lib=bwrt_lib) as c:
        c.set_light_sampling(True)
        want = adaptive_sequence(c, scene, w, h, mb)
    same(got, want)
    assert got["stats"][0][0] > 0  # the list kernel did run


def test_device_entry_point_with_a_filter_behind(bwrt_lib):
    """rt_render_device on the context's stream, rt_denoise_var_device queued
    directly behind it."""
    import torch
    scene = scenes.scene_07()
    w, h, mb = 64, 36, 4
    with Renderer.cpu(0, lib=bwrt_lib) as c:
        c.set_scene(scene)
        c.set_light_sampling(True)
        c.set_moments(True)
        for i in range(3):
            img_want = c.render(w, h, 2, mb, first_frame=1 if i == 0 else 0)
        dn_want = c.denoise_var(w, h)
        st_want = c.get_state(h, w)
    with Renderer(0, lib=bwrt_lib) as g:
        g.set_scene(scene)
        g.set_light_sampling(True)
        g.set_moments(True)
        buf = torch.zeros(h * w, dtype=torch.int32, device="cuda")
        dn = torch.zeros(h * w, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for i in range(3):
            g.render_device(g.params(w, h, 2, mb, first_frame=1 if i == 0 else 0), buf.data_ptr(), None)
        g.denoise_var_device(dn.data_ptr(), None)
        g.synchronize()
        assert g.last_kernel_name() == "rt_render_nee_kernel<256>"
        st = g.get_state(h, w)
        img = buf.cpu().numpy().view(np.uint8).reshape(h, w, 4)
        dn_img = dn.cpu().numpy().view(np.uint8).reshape(h, w, 4)
    same_state(st, st_want)
    assert np.array_equal(img, img_want)
    assert np.array_equal(dn_img, dn_want)


def test_three_identical_sequences(bwrt_lib):
    scene = scenes.scene_07()
    runs = []
    for _ in range(3):
        with Renderer(0, lib=bwrt_lib) as g:
            g.set_scene(scene)
            g.set_light_sampling(True)
            runs.append(state(g, 67, 45, 3, 4, calls=2))
    same_state(runs[0], runs[1])
    same_state(runs[0], runs[2])


def test_error_contract(bwrt_lib):
    """Fast precision with the switch on, in either order of the two setters:
    render calls return RT_ERR_UNSUPPORTED and touch nothing."""
    w, h = 33, 17
    for order in ("switch_first", "precision_first"):
        with Renderer(0, lib=bwrt_lib) as g:
            g.set_scene(scenes.scene_07())
            g.render(w, h, 2, 4, first_frame=1)
            before = g.get_state(h, w)
            if order == "switch_first":
                g.set_light_sampling(True)
                g.set_precision("fast")
            else:
                g.set_precision("fast")
                g.set_light_sampling(True)
            p = g.params(w, h, 2, 4)
            out = np.zeros((h, w, 4), np.uint8)
            assert bwrt_lib.rt_render_ex(g.ctx, C.byref(p), out.ctypes.data, None) == abi.RT_ERR_UNSUPPORTED
            assert "light sampling" in bwrt_lib.rt_last_error(g.ctx).decode()
            assert bwrt_lib.rt_render(g.ctx, w, h, 1, out.ctypes.data) == abi.RT_ERR_UNSUPPORTED
            # another frame shape: not even the shard state is re-made
            q = g.params(w + 1, h, 2, 4, first_frame=1)
            assert bwrt_lib.rt_render_ex(g.ctx, C.byref(q), out.ctypes.data, None) == abi.RT_ERR_UNSUPPORTED
            assert g.frame_counter == 3 and not out.any()
            same_state(before, g.get_state(h, w))
            assert bwrt_lib.rt_set_light_sampling(g.ctx, 2) == abi.RT_ERR_INVALID_ARGUMENT
            # either setter alone lifts the refusal
            if order == "switch_first":
                g.set_precision("exact")
            else:
                g.set_light_sampling(False)
            g.render(w, h, 1, 4)
            assert g.frame_counter == 4
