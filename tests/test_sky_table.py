"""The host-side sky table (rt_sky_table, csrc/rt_sky.cpp) against the
unchanged CPU fallback — no GPU.

A set bit claims that every camera ray of the tile misses.  The fallback
traces every ray, so for each pixel of a sky tile its state after FRAMES
frames must be what a miss in every frame leaves: frameSum the sequential sum
of the background, the RNG state advanced by the jitter's rejection loops
only — the state the same pixel reaches in the EMPTY scene under the same
camera, where every ray misses by construction."""
import numpy as np
import pytest

import sky_cases as S
from bwrt import scenes


@pytest.fixture(scope="module")
def cpu(bwrt_lib):
    from bwrt import Renderer
    r = Renderer.cpu(0, lib=bwrt_lib)
    yield r
    r.close()


def render_state(r, scene, w, h, off, stride, mb=2):
    r.set_scene(scene)
    r.set_background(*S.BG)
    r.init_rand(w, h, off, stride)
    r.render(w, h, S.FRAMES, mb, first_frame=1, row_offset=off, row_stride=stride)
    rows = len(range(off, h, stride))
    return r.get_state(rows, w)


@pytest.mark.parametrize("case", S.ORDINARY, ids=[c[0] for c in S.ORDINARY])
def test_sky_tiles_only_miss(cpu, case):
    _, make, w, h, off, stride, tw, sq = case
    scene = make()
    rng, acc = render_state(cpu, scene, w, h, off, stride)
    bits, mask, used = S.sky_pixels(cpu, w, h, off, stride, tw, sq)
    # not vacuous: a sky tile and a non-sky tile, both holding pixels
    assert bits[used].any() and not bits[used].all(), (int(bits[used].sum()), len(used))
    assert (acc[mask] == S.background_sum(S.FRAMES)).all()
    # the un-jittered camera ray of every such pixel misses too
    prim = cpu.render_aov(w, h, off, stride)["prim"]
    assert (prim[mask] == -1).all()
    empty = scenes.Scene(scene.camera, name="empty")
    rng0, acc0 = render_state(cpu, empty, w, h, off, stride)
    assert (acc0 == S.background_sum(S.FRAMES)).all()
    assert np.array_equal(rng[:, mask], rng0[:, mask]), "a sky tile's pixel drew more than its rejection loops"
    # (and the test can tell: outside the sky tiles streams did advance further)
    assert not np.array_equal(rng[:, ~mask], rng0[:, ~mask])


@pytest.mark.parametrize("name,make", S.EMPTY_TABLE, ids=[c[0] for c in S.EMPTY_TABLE])
def test_nothing_proven_outside_the_bounds(cpu, name, make):
    cpu.set_scene(make())
    for tw in (8, 32):
        bits, _ = cpu.sky_table(160, 90, tile_w=tw)
        assert len(bits) and not bits.any()


def test_linear_order_and_samples_per_pixel_have_no_table(cpu):
    cpu.set_scene(scenes.scene_07())
    bits, _ = cpu.sky_table(160, 90, tile_w=0)
    assert len(bits) == 0
    cpu.set_samples_per_pixel(2)
    try:
        bits, _ = cpu.sky_table(160, 90, tile_w=8)
        assert not bits.any()
    finally:
        cpu.set_samples_per_pixel(1)
    assert cpu.sky_table(160, 90, tile_w=8)[0].any()


@pytest.mark.parametrize("tw,sq", [(8, 0), (16, 0), (32, 0), (8, 1), (4, 1)])
def test_empty_scene_is_all_sky(cpu, tw, sq):
    cpu.set_scene(scenes.empty_scene())
    for w, h in ((100, 37), (64, 64), (3, 2)):
        bits, _, used = S.sky_pixels(cpu, w, h, 0, 1, tw, sq)
        assert bits[used].all()
        pad = np.ones(len(bits), bool)
        pad[used] = False
        assert not bits[pad].any()  # tiles without a pixel (tile_sq padding) stay clear


def test_one_pixel_frame_has_no_direction(cpu):
    """width 1: screen_z = -(1 / 2) / tan = -0, the pixel's direction is
    normalize(0, 0, -0) = NaN, and the reference accepts NaN distances: the
    tile is not sky, even in the empty scene."""
    cpu.set_scene(scenes.empty_scene())
    bits, _ = cpu.sky_table(1, 1, tile_w=8)
    assert len(bits) == 1 and not bits.any()


def test_table_is_cached_per_view(cpu):
    cpu.set_scene(scenes.scene_07())
    a, n0 = cpu.sky_table(160, 90, tile_w=8)
    b, n1 = cpu.sky_table(160, 90, tile_w=8)
    assert n1 == n0 and np.array_equal(a, b)  # reused
    # renders of the same view do not rebuild it either
    cpu.render(160, 90, 1, 1, first_frame=1)
    assert cpu.sky_table(160, 90, tile_w=8)[1] == n0
    cam = cpu.get_camera()
    cam.angle[0] = 0.6
    cpu.set_camera(cam)
    c, n2 = cpu.sky_table(160, 90, tile_w=8)
    assert n2 == n0 + 1 and not np.array_equal(a, c)
    cpu.set_scene(scenes.scene_04())
    d, n3 = cpu.sky_table(160, 90, tile_w=8)
    assert n3 == n2 + 1 and not np.array_equal(c, d)
    # every other part of the key: frame shape, shard, tile shape
    assert cpu.sky_table(160, 91, tile_w=8)[1] == n3 + 1
    assert cpu.sky_table(160, 91, 1, 3, tile_w=8)[1] == n3 + 2
    assert cpu.sky_table(160, 91, 1, 3, tile_w=16)[1] == n3 + 3
    assert cpu.sky_table(160, 91, 1, 3, tile_w=16, tile_sq=True)[1] == n3 + 4
    assert cpu.controls(["W"], 0.1) and cpu.sky_table(160, 91, 1, 3, tile_w=16, tile_sq=True)[1] == n3 + 5


def test_tile_of_pixel_matches_the_kernels_order(cpu):
    """sky_cases.tile_of_pixel against the launch order itself: in the empty
    scene exactly the tiles that hold a pixel are sky (the table walks the
    grid as item_to_pixel does), for ragged sizes and both tile orders."""
    cpu.set_scene(scenes.empty_scene())
    for w, h, tw, sq in ((100, 37, 8, 0), (100, 37, 8, 1), (33, 9, 16, 1), (65, 5, 32, 0)):
        bits, _ = cpu.sky_table(w, h, tile_w=tw, tile_sq=sq)
        t = S.tile_of_pixel(w, h, tw, sq)
        assert np.array_equal(np.flatnonzero(bits), np.unique(t))
