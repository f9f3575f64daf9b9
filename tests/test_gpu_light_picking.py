"""Weighted light picking on the MI355X: the weighted instantiations of
csrc/rt_kernel_nee.h against the CPU backend, bit for bit (both run the
arithmetic of csrc/rt_light.h and csrc/rt_path.h): every render call's
frameSum, RNG state and RGBA.  tests/test_light_picking.py checks the
estimator itself on the CPU backend.

The weight passes have no size threshold (two passes over the whole table,
nothing cached), so the table sizes below — 1, 2, 3, 8 and 40 lights — only
have to cover an empty, a short and a long loop.
"""
import numpy as np
import pytest

from bwrt import Renderer, scenes
from test_adaptive import adaptive_sequence
from test_gpu_adaptive import same
from test_light_sampling import dark_07, state, same_state, triangle_light_scene
from test_light_picking import black_light_scene, eight_lights, small_normal_scene

pytestmark = pytest.mark.gpu


def pair(lib, scene, w, h, mb, frames=3, calls=1, spp=1, kernel=None, **kw):
    """The same calls on a GPU and a CPU context with weighted light sampling."""
    with Renderer(0, lib=lib) as g:
        g.set_scene(scene)
        g.set_light_sampling(True)
        g.set_light_picking("weighted")
        g.set_samples_per_pixel(spp)
        got = state(g, w, h, frames, mb, calls=calls, **kw)
        name = g.last_kernel_name()
        assert g.last_kernel_ms() > 0
    with Renderer.cpu(0, lib=lib) as c:
        c.set_scene(scene)
        c.set_light_sampling(True)
        c.set_light_picking("weighted")
        c.set_samples_per_pixel(spp)
        want = state(c, w, h, frames, mb, calls=calls, **kw)
    same_state(got, want)
    if kernel is not None:
        assert name == kernel, name
    return got


@pytest.mark.parametrize("name,w,h,mb,kernel", [
    ("07", 67, 45, 4, "rt_render_nee_kernel<256,weighted>"),
    ("07", 5, 3, 4, "rt_render_nee_kernel<256,weighted>"),
    ("07", 1, 1, 4, "rt_render_nee_kernel<256,weighted>"),  # width / 2 == 0: the NaN camera ray
    ("04_box", 67, 45, 3, "rt_render_nee_kernel<256,weighted>"),  # quads, normals of length 200: no NEE level on them
    ("stress", 96, 54, 8, "rt_render_nee_kernel<256,hit_global,bvh,weighted>"),  # the BVH walk, 8 lights
    ("07", 67, 45, 0, None),  # no level can act: the default launch policy's kernel
    ("07", 67, 45, 1, "rt_render_nee_kernel<256,weighted>"),
    ("07", 67, 45, 11, "rt_render_nee_kernel<256,weighted>"),  # the last depth with 256 lanes
    ("07", 67, 45, 12, "rt_render_nee_kernel<64,weighted>"),
    ("stress", 48, 27, 12, "rt_render_nee_kernel<64,hit_global,bvh,weighted>"),
])
def test_renders_equal_cpu(bwrt_lib, name, w, h, mb, kernel):
    got = pair(bwrt_lib, scenes.SCENES[name](), w, h, mb, kernel=kernel)
    if mb == 0:
        with Renderer(0, lib=bwrt_lib) as g:
            g.set_scene(scenes.SCENES[name]())
            state(g, w, h, 3, mb)
            default = g.last_kernel_name()
        with Renderer(0, lib=bwrt_lib) as g:
            g.set_scene(scenes.SCENES[name]())
            g.set_light_sampling(True)
            g.set_light_picking("weighted")
            state(g, w, h, 3, mb)
            assert g.last_kernel_name() == default and "nee" not in default


@pytest.mark.parametrize("make,mb", [(eight_lights, 4), (small_normal_scene, 2), (lambda: black_light_scene(5.0), 4),
                                     (scenes.scene_01, 4)])
def test_table_sizes_and_weight_cases(bwrt_lib, make, mb):
    """8 lights over 18x of distance, a kind-2 normal (nl != 1), a zero-power
    light (w = 0), one light (W / w == 1)."""
    pair(bwrt_lib, make(), 67, 45, mb, kernel="rt_render_nee_kernel<256,weighted>")


def test_hit_table_in_global_memory_and_a_long_table(bwrt_lib, monkeypatch):
    monkeypatch.setenv("BWRT_BVH_MIN", "100000000")
    scene = scenes.stress_scene(n_triangles=400, n_spheres=48, n_emissive=40)  # over 16 KB of hit table, 40 lights
    with Renderer.cpu(1, lib=bwrt_lib) as c:
        c.set_scene(scene)
        assert len(c.lights()) == 40
    pair(bwrt_lib, scene, 24, 16, 4, kernel="rt_render_nee_kernel<256,hit_global,weighted>")
    pair(bwrt_lib, scene, 24, 16, 12, kernel="rt_render_nee_kernel<64,hit_global,weighted>")


def test_samples_per_pixel(bwrt_lib):
    pair(bwrt_lib, scenes.scene_07(), 67, 45, 4, spp=3, kernel="rt_render_nee_kernel<256,weighted>")


@pytest.mark.parametrize("off", [0, 1])
def test_row_shard(bwrt_lib, off):
    pair(bwrt_lib, scenes.scene_07(), 67, 45, 4, row_offset=off, row_stride=2, kernel="rt_render_nee_kernel<256,weighted>")


def test_continued_accumulation(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 67, 45
    res = {}
    for gpu in (True, False):
        with (Renderer(0, lib=bwrt_lib) if gpu else Renderer.cpu(0, lib=bwrt_lib)) as r:
            r.set_scene(scene)
            r.set_light_sampling(True)
            r.set_light_picking("weighted")
            a = r.render(w, h, 3, 4, first_frame=1)
            b = r.render(w, h, 5, 4)
            assert r.frame_counter == 9
            res[gpu] = [a, b, *r.get_state(h, w)]
    same_state(res[True], res[False])


def test_toggling_selects_the_kernel(bwrt_lib):
    """The mode picks the instantiation per call, inside one accumulation, and
    is stored without effect while light sampling is off."""
    w, h = 67, 45
    res = {}
    for gpu in (True, False):
        with (Renderer(0, lib=bwrt_lib) if gpu else Renderer.cpu(0, lib=bwrt_lib)) as r:
            r.set_scene(scenes.scene_07())
            r.set_light_picking("weighted")
            r.render(w, h, 2, 4, first_frame=1)
            names = [r.last_kernel_name()]
            r.set_light_sampling(True)
            r.render(w, h, 2, 4)
            names.append(r.last_kernel_name())
            r.set_light_picking("uniform")
            r.render(w, h, 2, 4)
            names.append(r.last_kernel_name())
            res[gpu] = list(r.get_state(h, w))
            if gpu:
                assert "nee" not in names[0]
                assert names[1:] == ["rt_render_nee_kernel<256,weighted>", "rt_render_nee_kernel<256>"]
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
            g.set_light_picking("weighted" if on else "uniform")
            res.append(state(g, w, h, 3, mb, calls=2))
    same_state(res[0], res[1])


@pytest.mark.parametrize("name,w,h,mb,kernel", [
    ("07", 67, 45, 4, "rt_render_nee_kernel<256,list,weighted>"),
    ("stress", 96, 54, 8, "rt_render_nee_kernel<256,hit_global,bvh,list,weighted>"),
    ("07", 67, 45, 12, "rt_render_nee_kernel<64,list,weighted>"),
    ("stress", 96, 54, 12, "rt_render_nee_kernel<64,hit_global,bvh,list,weighted>"),
    ("big", 24, 16, 4, "rt_render_nee_kernel<256,hit_global,list,weighted>"),
    ("big", 24, 16, 12, "rt_render_nee_kernel<64,hit_global,list,weighted>"),
])
def test_adaptive_calls_equal_cpu(bwrt_lib, monkeypatch, name, w, h, mb, kernel):
    if name == "big":
        monkeypatch.setenv("BWRT_BVH_MIN", "100000000")
        scene = scenes.stress_scene(n_triangles=400, n_spheres=8)
    else:
        scene = scenes.SCENES[name]()
    with Renderer(0, lib=bwrt_lib) as g:
        g.set_light_sampling(True)
        g.set_light_picking("weighted")
        got = adaptive_sequence(g, scene, w, h, mb)
        assert g.last_kernel_name() == kernel
    with Renderer.cpu(0, lib=bwrt_lib) as c:
        c.set_light_sampling(True)
        c.set_light_picking("weighted")
        want = adaptive_sequence(c, scene, w, h, mb)
    same(got, want)
    assert got["stats"][0][0] > 0  # the list kernel did run


def test_three_identical_sequences(bwrt_lib):
    scene = scenes.scene_07()
    runs = []
    for _ in range(3):
        with Renderer(0, lib=bwrt_lib) as g:
            g.set_scene(scene)
            g.set_light_sampling(True)
            g.set_light_picking("weighted")
            runs.append(state(g, 67, 45, 3, 4, calls=2))
    same_state(runs[0], runs[1])
    same_state(runs[0], runs[2])
