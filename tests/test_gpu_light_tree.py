"""The light hierarchy on the MI355X: the tree instantiations of
csrc/rt_kernel_nee.h against the CPU backend, bit for bit (both run the
arithmetic of csrc/rt_light.h and csrc/rt_path.h): every render call's frameSum,
RNG state and RGBA, and rt_light_pick_probabilities word for word.
tests/test_light_tree.py checks the pick itself on the CPU backend.

The descent has no size threshold; the table sizes — 2, 3, 5, 8, 40 and 256
lights — cover a tree that is one level, odd trees whose leaves sit at two
depths, short and long descents, the hit table in LDS, in global memory and
behind the BVH walk.
"""
import numpy as np
import pytest

from bwrt import Renderer, scenes
from light_tree_cases import RENDER_TABLES, TABLES, far_points, points_of, renderer
from test_adaptive import adaptive_sequence
from test_gpu_adaptive import same
from test_light_sampling import dark_07, same_state, state

pytestmark = pytest.mark.gpu

W0, H0 = 67, 45


def pair(lib, name, w, h, mb, frames=3, calls=1, spp=1, kernel=None, **kw):
    """The same calls on a GPU and a CPU context with the hierarchy on."""
    res = []
    for gpu in (True, False):
        with renderer(lib, name, gpu=gpu) as r:
            r.set_samples_per_pixel(spp)
            res.append(state(r, w, h, frames, mb, calls=calls, **kw))
            if gpu:
                got = r.last_kernel_name()
                assert r.last_kernel_ms() > 0
    same_state(res[0], res[1])
    if kernel is not None:
        assert got == kernel, got
    return res[0]


@pytest.mark.parametrize("name,mb,kernel", [
    ("2", 2, "rt_render_nee_kernel<256,tree>"),  # the root's children are the two leaves; a kind-2 normal
    ("3", 4, "rt_render_nee_kernel<256,tree>"),
    ("5", 4, "rt_render_nee_kernel<256,tree>"),
    ("8", 4, "rt_render_nee_kernel<256,tree>"),
    ("3", 11, "rt_render_nee_kernel<256,tree>"),  # the last depth with 256 lanes
    ("3", 12, "rt_render_nee_kernel<64,tree>"),
    ("8", 12, "rt_render_nee_kernel<64,tree>"),
    ("256", 4, "rt_render_nee_kernel<256,hit_global,bvh,tree>"),  # the BVH walk, 8 levels
    ("256", 12, "rt_render_nee_kernel<64,hit_global,bvh,tree>"),
    ("mixed", 4, "rt_render_nee_kernel<256,tree,polygons>"),
    ("mixed", 12, "rt_render_nee_kernel<64,tree,polygons>"),
    ("quads", 4, "rt_render_nee_kernel<256,tree,polygons>"),  # polygons alone
])
def test_renders_equal_cpu(bwrt_lib, name, mb, kernel):
    pair(bwrt_lib, name, W0, H0, mb, kernel=kernel)


@pytest.mark.parametrize("name,mb,kernel", [
    ("40", 4, "rt_render_nee_kernel<256,hit_global,tree>"),
    ("40", 12, "rt_render_nee_kernel<64,hit_global,tree>"),
    ("long_mixed", 4, "rt_render_nee_kernel<256,hit_global,tree,polygons>"),  # 40 spheres and 4 triangles
    ("long_mixed", 12, "rt_render_nee_kernel<64,hit_global,tree,polygons>"),
])
def test_hit_table_in_global_memory(bwrt_lib, monkeypatch, name, mb, kernel):
    monkeypatch.setenv("BWRT_BVH_MIN", "100000000")
    pair(bwrt_lib, name, 24, 16, mb, kernel=kernel)


@pytest.mark.parametrize("mb,kernel", [(8, "rt_render_nee_kernel<256,hit_global,bvh,tree,polygons>"),
                                       (12, "rt_render_nee_kernel<64,hit_global,bvh,tree,polygons>")])
def test_polygons_behind_the_bvh_walk(bwrt_lib, mb, kernel):
    """8 spheres and 4 emissive triangles of the stress scene"""
    with renderer(bwrt_lib, "stress_tris") as r:
        assert len(r.lights()) == 12 and len(r.light_tree()) == 23
    pair(bwrt_lib, "stress_tris", 48, 27, mb, kernel=kernel)


def test_samples_per_pixel(bwrt_lib):
    pair(bwrt_lib, "3", W0, H0, 4, spp=3, kernel="rt_render_nee_kernel<256,tree>")


@pytest.mark.parametrize("off", [0, 1])
def test_row_shard(bwrt_lib, off):
    pair(bwrt_lib, "8", W0, H0, 4, row_offset=off, row_stride=2, kernel="rt_render_nee_kernel<256,tree>")


def test_continued_accumulation(bwrt_lib):
    res = {}
    for gpu in (True, False):
        with renderer(bwrt_lib, "8", gpu=gpu) as r:
            a = r.render(W0, H0, 3, 4, first_frame=1)
            b = r.render(W0, H0, 5, 4)
            assert r.frame_counter == 9
            res[gpu] = [a, b, *r.get_state(H0, W0)]
    same_state(res[True], res[False])


def test_the_switch_selects_the_kernel(bwrt_lib):
    """`,tree` where the switch acts, today's names where it does not: light
    sampling off, uniform picking, a one-record table, max_bounces 0 — inside
    one accumulation, equal to the CPU backend's."""
    res = {}
    for gpu in (True, False):
        with (Renderer(0, lib=bwrt_lib) if gpu else Renderer.cpu(0, lib=bwrt_lib)) as r:
            r.set_scene(scenes.scene_07())
            r.set_light_hierarchy(True)
            r.set_light_picking("weighted")
            r.render(W0, H0, 2, 4, first_frame=1)
            names = [r.last_kernel_name()]
            r.set_light_sampling(True)
            r.render(W0, H0, 2, 4)
            names.append(r.last_kernel_name())
            r.set_light_picking("uniform")
            r.render(W0, H0, 2, 4)
            names.append(r.last_kernel_name())
            r.set_light_picking("weighted")
            r.set_light_hierarchy(False)
            r.render(W0, H0, 2, 4)
            names.append(r.last_kernel_name())
            r.set_light_hierarchy(True)
            r.render(W0, H0, 2, 0)
            names.append(r.last_kernel_name())
            res[gpu] = list(r.get_state(H0, W0))
            if gpu:
                assert "nee" not in names[0] and "nee" not in names[4]
                assert names[1:4] == ["rt_render_nee_kernel<256,tree>", "rt_render_nee_kernel<256>",
                                      "rt_render_nee_kernel<256,weighted>"]
    same_state(res[True], res[False])
    with Renderer(0, lib=bwrt_lib) as g:  # one record: the table walk's kernel
        g.set_scene(scenes.scene_01())
        g.set_light_sampling(True)
        g.set_light_picking("weighted")
        g.set_light_hierarchy(True)
        state(g, W0, H0, 2, 4)
        assert g.last_kernel_name() == "rt_render_nee_kernel<256,weighted>"


def test_no_table_is_the_default_gpu_render(bwrt_lib):
    res = []
    for on in (False, True):
        with Renderer(0, lib=bwrt_lib) as g:
            g.set_scene(dark_07())
            g.set_light_sampling(on)
            g.set_light_picking("weighted" if on else "uniform")
            g.set_light_hierarchy(on)
            res.append(state(g, W0, H0, 3, 4, calls=2))
    same_state(res[0], res[1])


@pytest.mark.parametrize("name,w,h,mb,kernel", [
    ("3", 48, 27, 4, "rt_render_nee_kernel<256,list,tree>"),
    ("3", 48, 27, 12, "rt_render_nee_kernel<64,list,tree>"),
    ("256", 48, 27, 4, "rt_render_nee_kernel<256,hit_global,bvh,list,tree>"),
    ("256", 48, 27, 12, "rt_render_nee_kernel<64,hit_global,bvh,list,tree>"),
    ("40", 24, 16, 4, "rt_render_nee_kernel<256,hit_global,list,tree>"),
    ("40", 24, 16, 12, "rt_render_nee_kernel<64,hit_global,list,tree>"),
    ("mixed", 48, 27, 4, "rt_render_nee_kernel<256,list,tree,polygons>"),
    ("mixed", 48, 27, 12, "rt_render_nee_kernel<64,list,tree,polygons>"),
    ("long_mixed", 24, 16, 4, "rt_render_nee_kernel<256,hit_global,list,tree,polygons>"),
    ("long_mixed", 24, 16, 12, "rt_render_nee_kernel<64,hit_global,list,tree,polygons>"),
    ("stress_tris", 48, 27, 4, "rt_render_nee_kernel<256,hit_global,bvh,list,tree,polygons>"),
    ("stress_tris", 48, 27, 12, "rt_render_nee_kernel<64,hit_global,bvh,list,tree,polygons>"),
])
def test_adaptive_calls_equal_cpu(bwrt_lib, monkeypatch, name, w, h, mb, kernel):
    """All twelve `list,tree` instantiations: both block sizes; the hit table in
    LDS, in global memory and behind the BVH walk; sphere-only and polygon-aware"""
    if name in ("40", "long_mixed"):
        monkeypatch.setenv("BWRT_BVH_MIN", "100000000")
    make, shapes, _ = RENDER_TABLES[name]
    res = []
    for gpu in (True, False):
        with (Renderer(0, lib=bwrt_lib) if gpu else Renderer.cpu(0, lib=bwrt_lib)) as r:
            r.set_light_sampling(True)
            r.set_light_picking("weighted")
            r.set_light_shapes(shapes)
            r.set_light_hierarchy(True)
            res.append(adaptive_sequence(r, make(), w, h, mb))
            if gpu:
                assert r.last_kernel_name() == kernel, r.last_kernel_name()
    same(res[0], res[1])
    assert res[0]["stats"][0][0] > 0  # the list kernel did run


def test_three_identical_sequences(bwrt_lib):
    runs = []
    for _ in range(3):
        with renderer(bwrt_lib, "8", gpu=True) as g:
            runs.append(state(g, W0, H0, 3, 4, calls=2))
    same_state(runs[0], runs[1])
    same_state(runs[0], runs[2])


@pytest.mark.parametrize("name", list(TABLES))
def test_pick_probabilities_equal_cpu(bwrt_lib, name):
    """The CPU test's point sets (and the far points of its underflow case),
    under the hierarchy, the table walk and the uniform pick: word for word, a
    NaN equal to any NaN."""
    make = TABLES[name][0]
    with renderer(bwrt_lib, name) as c, renderer(bwrt_lib, name, gpu=True) as g:
        lights, tree = c.lights(), c.light_tree()
        assert g.light_tree().tobytes() == tree.tobytes()
        pts, prims, _ = points_of(name, lights, tree, make())
        fp, fi = far_points(lights, make())
        pts, prims = np.concatenate([pts, fp]), np.concatenate([prims, fi])
        for pick, hierarchy in (("weighted", True), ("weighted", False), ("uniform", False)):
            for r in (c, g):
                r.set_light_picking(pick)
                r.set_light_hierarchy(hierarchy)
            a, b = c.light_pick_probabilities(pts, prims), g.light_pick_probabilities(pts, prims)
            assert a.shape == (len(pts), len(lights))
            nan = np.isnan(a)
            assert np.array_equal(nan, np.isnan(b))
            assert np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]), (pick, hierarchy)
        assert (a > 0).all() and (a[0] == a).all()  # (the last mode: uniform)
