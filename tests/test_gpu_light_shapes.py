"""Polygon lights on the MI355X: the polygon-aware instantiations of
csrc/rt_kernel_nee.h against the CPU backend, bit for bit (both run the
arithmetic of csrc/rt_light.h and csrc/rt_path.h): every render call's
frameSum, RNG state and RGBA.  tests/test_light_shapes.py checks the estimator
itself on the CPU backend.
"""
import numpy as np
import pytest

from bwrt import Renderer, abi, scenes
from test_adaptive import adaptive_sequence
from test_gpu_adaptive import same
from test_light_sampling import same_state, state
from test_light_shapes import (box_with_emissive_quad, forty_quads, mixed, quad_panel, stress_with_emissive_triangles,
                               triangle_panel)

pytestmark = pytest.mark.gpu


def setup(r, scene, shapes="all", pick="uniform", on=True, spp=1):
    r.set_scene(scene)
    r.set_light_sampling(on)
    r.set_light_picking(pick)
    r.set_light_shapes(shapes)
    r.set_samples_per_pixel(spp)
    return r


def pair(lib, scene, w, h, mb, frames=3, calls=1, spp=1, pick="uniform", kernel=None, **kw):
    """The same calls on a GPU and a CPU context under RT_LIGHT_SHAPES_ALL."""
    with Renderer(0, lib=lib) as g:
        got = state(setup(g, scene, pick=pick, spp=spp), w, h, frames, mb, calls=calls, **kw)
        name = g.last_kernel_name()
        assert g.last_kernel_ms() > 0
    with Renderer.cpu(0, lib=lib) as c:
        want = state(setup(c, scene, pick=pick, spp=spp), w, h, frames, mb, calls=calls, **kw)
    same_state(got, want)
    if kernel is not None:
        if pick == "weighted":
            kernel = kernel.replace(",polygons>", ",weighted,polygons>")
        assert name == kernel, name
    return got


B, BVH = "rt_render_nee_kernel<256,polygons>", "rt_render_nee_kernel<256,hit_global,bvh,polygons>"


@pytest.mark.parametrize("pick", ["uniform", "weighted"])
@pytest.mark.parametrize("make,w,h,mb,kernel", [
    (quad_panel, 67, 45, 4, B),
    (triangle_panel, 67, 45, 4, B),
    (mixed, 67, 45, 4, B),
    (quad_panel, 5, 3, 4, B),
    (triangle_panel, 5, 3, 4, B),
    (mixed, 5, 3, 4, B),
    (quad_panel, 1, 1, 4, B),  # width / 2 == 0: the NaN camera ray
    (triangle_panel, 1, 1, 4, B),
    (mixed, 1, 1, 4, B),
    (box_with_emissive_quad, 67, 45, 3, B),  # the QUADS hit loop
    (stress_with_emissive_triangles, 96, 54, 8, BVH),  # the BVH walk, the deferred shadow ray
    (mixed, 67, 45, 0, None),  # no level can act: the default launch policy's kernel
    (mixed, 67, 45, 1, B),
    (mixed, 67, 45, 11, B),  # the last depth with 256 lanes
    (mixed, 67, 45, 12, "rt_render_nee_kernel<64,polygons>"),
    (stress_with_emissive_triangles, 48, 27, 12, "rt_render_nee_kernel<64,hit_global,bvh,polygons>"),
])
def test_renders_equal_cpu(bwrt_lib, make, w, h, mb, kernel, pick):
    pair(bwrt_lib, make(), w, h, mb, pick=pick, kernel=kernel)
    if mb == 0:
        with Renderer(0, lib=bwrt_lib) as g:
            state(setup(g, make(), on=False), w, h, 3, mb)
            default = g.last_kernel_name()
        with Renderer(0, lib=bwrt_lib) as g:
            state(setup(g, make(), pick=pick), w, h, 3, mb)
            assert g.last_kernel_name() == default and "nee" not in default


@pytest.mark.parametrize("pick", ["uniform", "weighted"])
def test_hit_table_in_global_memory_and_a_long_table(bwrt_lib, monkeypatch, pick):
    """Over 16 KB of hit table (no BVH), 40 quad lights and 8 sphere lights."""
    monkeypatch.setenv("BWRT_BVH_MIN", "100000000")
    s = scenes.stress_scene(n_triangles=400, n_spheres=48, n_emissive=8)
    n = s.counts
    scene = scenes.Scene(s.camera, list(s.spheres)[:n[0]], list(s.planes)[:n[1]], list(s.triangles)[:n[2]],
                         list(forty_quads().quads)[:40], name="big")
    with Renderer.cpu(1, lib=bwrt_lib) as c:
        assert len(setup(c, scene).lights()) == 48
    pair(bwrt_lib, scene, 24, 16, 4, pick=pick, kernel="rt_render_nee_kernel<256,hit_global,polygons>")
    pair(bwrt_lib, scene, 24, 16, 12, pick=pick, kernel="rt_render_nee_kernel<64,hit_global,polygons>")


def test_forty_quads(bwrt_lib):
    pair(bwrt_lib, forty_quads(), 67, 45, 4, pick="weighted", kernel=B)


def test_samples_per_pixel(bwrt_lib):
    pair(bwrt_lib, mixed(), 67, 45, 4, spp=3, kernel=B)


@pytest.mark.parametrize("off", [0, 1])
def test_row_shard(bwrt_lib, off):
    pair(bwrt_lib, mixed(), 67, 45, 4, row_offset=off, row_stride=2, kernel=B)


def test_continued_accumulation(bwrt_lib):
    w, h = 67, 45
    res = {}
    for gpu in (True, False):
        with (Renderer(0, lib=bwrt_lib) if gpu else Renderer.cpu(0, lib=bwrt_lib)) as r:
            setup(r, mixed())
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
            setup(r, mixed(), on=False)
            r.render(w, h, 2, 4, first_frame=1)
            names = [r.last_kernel_name()]
            r.set_light_sampling(True)
            r.render(w, h, 2, 4)
            names.append(r.last_kernel_name())
            r.set_light_shapes("spheres")
            r.render(w, h, 2, 4)
            names.append(r.last_kernel_name())
            res[gpu] = list(r.get_state(h, w))
            if gpu:
                assert "nee" not in names[0]
                assert names[1:] == [B, "rt_render_nee_kernel<256>"]
    same_state(res[True], res[False])


@pytest.mark.parametrize("name", ["07", "stress"])
def test_all_without_a_polygon_emitter_is_the_spheres_kernel(bwrt_lib, name):
    res, names = [], []
    for shapes in ("spheres", "all"):
        with Renderer(0, lib=bwrt_lib) as g:
            res.append(state(setup(g, scenes.SCENES[name](), shapes), 67, 45, 3, 4, calls=2))
            names.append(g.last_kernel_name())
    same_state(res[0], res[1])
    assert names[0] == names[1] and "polygons" not in names[0] and "nee" in names[0]


@pytest.mark.parametrize("shapes,on,mb", [("all", False, 4), ("spheres", True, 4), ("all", True, 0)])
def test_identities_against_the_default_gpu_render(bwrt_lib, shapes, on, mb):
    """Light sampling off, SPHERES on a polygon-lit scene and zero bounces:
    bit-identical to the default estimator's GPU render."""
    res = []
    for default in (True, False):
        with Renderer(0, lib=bwrt_lib) as g:
            setup(g, triangle_panel(), "spheres" if default else shapes, on=False if default else on)
            res.append(state(g, 67, 45, 3, mb, calls=2))
            assert "nee" not in g.last_kernel_name()
    same_state(res[0], res[1])


def test_reference_fast_stays_refused(bwrt_lib):
    with Renderer(0, lib=bwrt_lib) as g:
        setup(g, quad_panel())
        g.set_precision("fast")
        out = np.zeros((9, 16, 4), np.uint8)
        assert bwrt_lib.rt_render(g.ctx, 16, 9, 1, out.ctypes.data) == abi.RT_ERR_UNSUPPORTED
        assert "light sampling" in bwrt_lib.rt_last_error(g.ctx).decode() and not out.any()


@pytest.mark.parametrize("pick", ["uniform", "weighted"])
@pytest.mark.parametrize("name,w,h,mb,kernel", [
    ("quad", 67, 45, 4, "rt_render_nee_kernel<256,list,polygons>"),
    ("stress", 96, 54, 8, "rt_render_nee_kernel<256,hit_global,bvh,list,polygons>"),
    ("quad", 67, 45, 12, "rt_render_nee_kernel<64,list,polygons>"),
    ("stress", 96, 54, 12, "rt_render_nee_kernel<64,hit_global,bvh,list,polygons>"),
    ("big", 24, 16, 4, "rt_render_nee_kernel<256,hit_global,list,polygons>"),
    ("big", 24, 16, 12, "rt_render_nee_kernel<64,hit_global,list,polygons>"),
])
def test_adaptive_calls_equal_cpu(bwrt_lib, monkeypatch, name, w, h, mb, kernel, pick):
    if name == "big":
        monkeypatch.setenv("BWRT_BVH_MIN", "100000000")
        s = scenes.stress_scene(n_triangles=400, n_spheres=8)
        n = s.counts
        scene = scenes.Scene(s.camera, list(s.spheres)[:n[0]], list(s.planes)[:n[1]], list(s.triangles)[:n[2]],
                             list(quad_panel().quads)[:4], name="big")
    else:
        scene = quad_panel() if name == "quad" else stress_with_emissive_triangles()
    if pick == "weighted":
        kernel = kernel.replace(",polygons>", ",weighted,polygons>")
    res = []
    for gpu in (True, False):
        with (Renderer(0, lib=bwrt_lib) if gpu else Renderer.cpu(0, lib=bwrt_lib)) as r:
            r.set_light_sampling(True)
            r.set_light_picking(pick)
            r.set_light_shapes("all")
            res.append(adaptive_sequence(r, scene, w, h, mb))
            if gpu:
                assert r.last_kernel_name() == kernel
    same(res[0], res[1])
    assert res[0]["stats"][0][0] > 0  # the list kernel did run


def test_three_identical_sequences(bwrt_lib):
    runs = []
    for _ in range(3):
        with Renderer(0, lib=bwrt_lib) as g:
            runs.append(state(setup(g, mixed(), pick="weighted"), 67, 45, 3, 4, calls=2))
    same_state(runs[0], runs[1])
    same_state(runs[0], runs[2])
