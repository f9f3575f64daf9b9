"""Cases and helpers shared by the sky-table tests (test_sky_table.py on the
CPU fallback, test_gpu_sky.py on the kernels)."""
import ctypes as C

import numpy as np

from bwrt import scenes
from bwrt.abi import Camera, Plane, Quad, Sphere, Triangle, Vec3

BG = (0.3, 0.5, 0.7)  # non-black, three different channels
FRAMES = 8


def with_camera(scene, yaw=0.0, pitch=0.0, pos=None, fov=None):
    c = scene.camera
    p = c.position if pos is None else Vec3(*map(float, pos))
    scene.set_camera(Camera(p, (C.c_float * 2)(float(yaw), float(pitch)), float(c.fov if fov is None else fov)))
    return scene


def random_sky_scene(seed):
    """Seeded scene of well-formed primitives (spheres, the floor, an oblique
    plane on odd seeds, triangles, a convex planar quad on some) under a yawed
    and pitched camera: silhouettes and the horizon cut tiles obliquely."""
    rng = np.random.default_rng(1000 + seed)
    U = rng.uniform
    v = lambda p: Vec3(*map(float, p))  # noqa: E731
    mat = lambda: scenes.material(tuple(U(0.1, 1, 3)), float(rng.choice([0, 0, U(1, 20)])),  # noqa: E731
                                  float(rng.choice([1.0, U(0, 1)])), float(U(1, 3)))
    cam = Camera(v(U(-1, 1, 3) + [0, 2, 0]), (C.c_float * 2)(float(U(-0.7, 0.7)), float(U(-0.2, 0.6))),
                 float(U(0.9, 1.9)))
    sph = [Sphere(v(U(-5, 5, 3) + [0, 3, -8]), float(U(0.3, 1.5)), mat()) for _ in range(int(rng.integers(1, 6)))]
    pln = [Plane(v([0, 0, 0]), (Vec3 * 2)(v([0, 0, float(U(0.5, 3))]), v([float(U(0.5, 3)), 0, 0])), mat())]
    if seed % 2:  # a ramp rising away from the camera (an oblique horizon), non-unit normal
        pln.append(Plane(v([0, 0, -20]), (Vec3 * 2)(v([2, float(U(-0.3, 0.3)), 0]), v([0, 1.5, float(U(-6, -3))])), mat()))
    tri = []
    for _ in range(int(rng.integers(0, 5))):
        a = U(-4, 4, 3) + [0, 3, -7]
        tri.append(Triangle((Vec3 * 3)(v(a), v(a + [float(U(0.5, 2)), 0, float(U(-1, 1))]),
                                       v(a + [float(U(-0.5, 0.5)), float(U(0.5, 2)), 0])), mat()))
    quads = []
    if seed % 3 == 0:  # a convex planar quad (a tilted rectangle)
        o, e0, e1 = U(-3, 3, 3) + [0, 4, -9], np.array([float(U(1, 3)), 0.0, float(U(-1, 1))]), np.array([0.0, float(U(1, 2)), 0.0])
        quads.append(Quad((Vec3 * 4)(v(o), v(o + e0), v(o + e0 + e1), v(o + e1)), mat()))
    return scenes.Scene(cam, sph, pln, tri, quads, name=f"sky_random{seed}")


def _box(yaw, pitch):
    return lambda: with_camera(scenes.scene_04_box(), yaw, pitch)


def _s07(yaw=0.0, pitch=0.0):
    return lambda: with_camera(scenes.scene_07(), yaw, pitch)


# a dozen seeds whose camera sees both sky and scene (seeds 1 and 11 look down
# at the ramp: no sky tile at all)
RANDOM_SEEDS = (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13)

# (id, scene factory, width, height, row_offset, row_stride, tile_w, tile_sq):
# every one classifies at least one tile as sky and at least one as not sky
ORDINARY = [
    ("07_160x90", _s07(), 160, 90, 0, 1, 8, 0),
    ("07_100x37", _s07(), 100, 37, 0, 1, 8, 0),
    ("07_shard", _s07(), 160, 90, 1, 3, 8, 0),
    ("07_jitter", _s07(), 1024, 40, 0, 1, 8, 0),          # width >= 1000: jitter 0.001
    ("07_yaw_pitch", _s07(0.5, 0.3), 160, 90, 0, 1, 8, 0),
    ("07_pitch_down", _s07(-0.8, -0.25), 100, 37, 0, 1, 8, 0),
    ("07_tile16", _s07(0.2, 0.1), 160, 90, 0, 1, 16, 0),
    ("07_tile32", _s07(), 160, 90, 0, 1, 32, 0),
    ("07_tile_sq", _s07(0.3, 0.2), 100, 37, 0, 1, 8, 1),
    ("04_box_yaw", _box(1.3, 0.2), 160, 90, 0, 1, 8, 0),
    ("04_box_yaw_neg", _box(-1.2, 0.15), 100, 37, 0, 1, 8, 0),
    ("04_box_shard", _box(0.9, 0.1), 160, 90, 1, 3, 16, 0),
] + [(f"random{s}", (lambda s=s: random_sky_scene(s)), 96, 54, 0, 1, 8, s % 2) for s in RANDOM_SEEDS]


def _scaled07():
    from scenegen import _scaled
    return _scaled(scenes.scene_07(), 1e10)


def _nan07():
    s = scenes.scene_07()
    s.spheres[2].position.y = float("nan")
    return s


def _inf07():
    s = scenes.scene_07()
    s.triangles[1].vertices[0].x = float("inf")
    return s


def _inside07():  # the camera inside the centre white sphere
    return with_camera(scenes.scene_07(), pos=(0.1, 0.75, -4.0))


EMPTY_TABLE = [("scaled_1e10", _scaled07), ("nan", _nan07), ("inf", _inf07), ("camera_inside", _inside07)]


def tile_of_pixel(width, rows, tile_w, tile_sq):
    """(rows, width) array: the launch-order wave tile of every shard pixel
    (the inverse of the kernels' item_to_pixel)."""
    th = 64 // tile_w
    tiles_x = -(-width // tile_w)
    tx = np.arange(width)[None, :] // tile_w
    ty = np.arange(rows)[:, None] // th
    if tile_sq:
        sx = (tiles_x + 1) >> 1
        return ((ty >> 1) * sx + (tx >> 1)) * 4 + (ty & 1) * 2 + (tx & 1)
    return ty * tiles_x + tx + 0 * tx


def sky_pixels(r, width, height, row_offset, row_stride, tile_w, tile_sq):
    """(bits per tile, (rows, width) bool mask of the pixels in sky tiles)."""
    bits, _ = r.sky_table(width, height, row_offset, row_stride, tile_w, tile_sq)
    rows = len(range(row_offset, height, row_stride))
    t = tile_of_pixel(width, rows, tile_w, tile_sq)
    assert t.max() < len(bits)
    return bits, bits[t], np.unique(t)


def background_sum(frames):
    """frameSum of a pixel whose every frame misses: reset, then one float32
    add of the background per frame."""
    acc = np.zeros(3, np.float32)
    for _ in range(frames):
        acc = acc + np.asarray(BG, np.float32)
    return acc
