"""The sorted kernel's sky path (rt_render_sorted_kernel, render_sky_group)
against the CPU fallback, bit for bit: RGBA8, frameSum and RNG state, with the
sky table on (BWRT_SKY=2: built at a view's first launch) and off
(BWRT_SKY=0), on the cases of test_sky_table.py — every workgroup size, LDS
and global records, launch-order feedback."""
import numpy as np
import pytest

import sky_cases as S
from bwrt import scenes

pytestmark = pytest.mark.gpu

MB = 2


@pytest.fixture(scope="module")
def cpu(bwrt_lib):
    from bwrt import Renderer
    r = Renderer.cpu(0, lib=bwrt_lib)
    yield r
    r.close()


def fresh(bwrt_lib, monkeypatch, **env):
    """A renderer created under BWRT_* launch knobs (read at rt_create)."""
    from bwrt import Renderer
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return Renderer(0, lib=bwrt_lib)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def sorted_renderer(bwrt_lib, monkeypatch, block, grec, sky, tile_w=8, tile_sq=0):
    return fresh(bwrt_lib, monkeypatch, BWRT_SPREAD=0, BWRT_BLOCK=block, BWRT_GREC=grec, BWRT_ORDER=1,
                 BWRT_ORDER_PERIOD=2, BWRT_SKY=sky, BWRT_TILE=tile_w, BWRT_TILE_SQ=tile_sq)


def step(r, w, h, frames, mb, first, off=0, stride=1):
    """One render call and the full state after it."""
    img = r.render(w, h, frames, mb, first_frame=first, row_offset=off, row_stride=stride)
    rng, acc = r.get_state(len(range(off, h, stride)), w)
    return img, rng, acc


def same(a, b):
    for x, y, what in zip(a, b, ("RGBA8", "RNG state", "frameSum")):
        assert np.array_equal(x, y, equal_nan=what == "frameSum"), what


_REF = {}


def reference(cpu, case):
    """The checker's state for a case, computed once: FRAMES frames, then a
    continuation of 3 more."""
    if case[0] not in _REF:
        _, make, w, h, off, stride, _, _ = case
        cpu.set_scene(make())
        cpu.set_background(*S.BG)
        cpu.init_rand(w, h, off, stride)
        _REF[case[0]] = (step(cpu, w, h, S.FRAMES, MB, 1, off, stride), step(cpu, w, h, 3, MB, 0, off, stride))
    return _REF[case[0]]


def check_kernel(r, block, sky):
    name = r.last_kernel_name()
    assert name.startswith(f"rt_render_sorted_kernel<{block}"), name
    assert name.endswith("+sky") == bool(sky), name


@pytest.mark.parametrize("grec", [0, 1])
@pytest.mark.parametrize("block", [64, 128, 256])
def test_sky_cases_match_the_cpu_fallback(bwrt_lib, cpu, monkeypatch, block, grec):
    for tile in sorted({(c[6], c[7]) for c in S.ORDINARY}):
        for sky in (2, 0):
            r = sorted_renderer(bwrt_lib, monkeypatch, block, grec, sky, *tile)
            try:
                for case in [c for c in S.ORDINARY if (c[6], c[7]) == tile]:
                    _, make, w, h, off, stride, _, _ = case
                    first, more = reference(cpu, case)
                    r.set_scene(make())
                    r.set_background(*S.BG)
                    r.init_rand(w, h, off, stride)
                    same(step(r, w, h, S.FRAMES, MB, 1, off, stride), first)
                    check_kernel(r, block, sky)
                    # continuation: first_frame > 1, frameSum loaded, in a second launch
                    same(step(r, w, h, 3, MB, 0, off, stride), more)
                    check_kernel(r, block, sky)
            finally:
                r.close()


@pytest.mark.parametrize("sky", [2, 1, 0])
def test_view_changes_between_renders(bwrt_lib, cpu, monkeypatch, sky):
    """One context through a camera move, a scene change and a background
    change; BWRT_SKY=1 (the default policy) builds a view's table at the view's
    second launch, so each view is rendered twice."""
    w, h = 160, 90
    r = sorted_renderer(bwrt_lib, monkeypatch, 256, 0, sky)
    try:
        def both(frames, has_table, new_view=True):
            for x in (r, cpu):
                x.init_rand(w, h)
            same(step(r, w, h, frames, MB, 1), step(cpu, w, h, frames, MB, 1))
            assert r.last_kernel_name().endswith("+sky") == (has_table and (sky == 2 or (sky == 1 and not new_view)))
            same(step(r, w, h, 2, MB, 0), step(cpu, w, h, 2, MB, 0))
            assert r.last_kernel_name().endswith("+sky") == (sky != 0 and has_table)

        for x in (r, cpu):
            x.set_scene(scenes.scene_07())
            x.set_background(*S.BG)
        both(4, True)
        cam = r.get_camera()
        cam.angle[0], cam.angle[1] = 0.7, 0.25  # what was sky is not any more
        for x in (r, cpu):
            x.set_camera(cam)
        both(4, True)
        for x in (r, cpu):
            x.set_scene(S.with_camera(scenes.scene_04_box(), 1.3, 0.2))
        both(4, True)
        for x in (r, cpu):
            x.set_background(0.9, 0.1, 0.4)  # not part of the table's key: the kernel reads it
        both(4, True, new_view=False)
        for x in (r, cpu):  # the camera inside a sphere: an empty table, no sky launch
            x.set_scene(S.with_camera(scenes.scene_07(), pos=(0.1, 0.75, -4.0)))
        both(2, False)
    finally:
        r.close()


@pytest.mark.parametrize("sky", [2, 0])
def test_max_bounces_0_one_pixel_and_empty_scene(bwrt_lib, cpu, monkeypatch, sky):
    r = sorted_renderer(bwrt_lib, monkeypatch, 128, 0, sky)
    try:
        for scene, w, h, mb in ((scenes.scene_07(), 160, 90, 0), (scenes.scene_07(), 1, 1, 4),
                                (scenes.empty_scene(), 100, 37, 3), (scenes.scene_07(), 1024, 40, 1)):
            for x in (r, cpu):
                x.set_scene(scene)
                x.set_background(*S.BG)
                x.init_rand(w, h)
            same(step(r, w, h, 5, mb, 1), step(cpu, w, h, 5, mb, 1))
            assert r.last_kernel_name().startswith("rt_render_sorted_kernel<128")
            assert r.last_kernel_name().endswith("+sky") == (sky == 2 and (w, h) != (1, 1))
    finally:
        r.close()


def test_full_frame_with_launch_order_feedback(bwrt_lib, cpu, monkeypatch):
    """Config 3's frame (the product instantiation, global records, the
    reordered groups indexing the table) over three launches: blockIdx order,
    then reordered; the default policy, so the table arrives at the second."""
    w, h, mb = 1920, 1080, 4
    r = fresh(bwrt_lib, monkeypatch, BWRT_ORDER_PERIOD=2)
    try:
        for x in (r, cpu):
            x.set_scene(scenes.scene_07())
            x.set_background(*S.BG)
            x.init_rand(w, h)
        for i in range(3):
            same(step(r, w, h, 1, mb, 0), step(cpu, w, h, 1, mb, 0))
            assert r.last_kernel_name() == "rt_render_sorted_kernel<256,grec>+order" + ("+sky" if i else "")
    finally:
        r.close()
