"""The case matrix of the first-hit guide tests (tests/test_first_hit.py on the
CPU backend, tests/test_gpu_first_hit.py on the MI355X): scenes, frame sizes,
scene-compiler knobs, views and row shards, each compared bit for bit with
oracle.first_hit — the oracle's own closest-hit loop on the un-jittered
primary ray.  The oracle's result of a case is computed once and shared.
"""
import ctypes as C
import functools

import numpy as np

import denoise_ref as R
from bwrt import scenes
from bwrt.abi import Camera, Plane, Quad, Sphere, Triangle, Vec3
from scenegen import _random_scene, _scaled

KEYS = ("prim", "depth", "normal", "albedo")
BRUTE = {"BWRT_BVH_MIN": "100000000"}  # no BVH whatever the scene's size
BVH = {"BWRT_BVH_MIN": "1"}            # a BVH from the first bounded primitive on
PATHS = {"brute": BRUTE, "bvh": BVH}
MOVED = ((0.3, 1.2, 0.5), (0.35, -0.2))  # position, angles of the set_camera view


@functools.lru_cache(maxsize=None)
def stress(n_triangles=10000, n_spheres=256):
    """The stress scenes are never mutated by a case: built once."""
    return scenes.stress_scene(n_triangles=n_triangles, n_spheres=n_spheres)


class Case:
    """One frame: make() -> the scene, env = the scene-compiler knobs (read at
    set_scene), view = None, "set_camera" (MOVED) or "controls" (MOVED, then
    one controls() frame with W + LEFT + UP held), stats = a substring the
    BWRT_BVH_STATS line must hold (the node format, the octant mask)."""

    def __init__(self, name, make, w, h, env=None, off=0, stride=1, background=(0.0, 0.0, 0.0), view=None,
                 stats=None, extreme=False):
        self.name, self.make, self.w, self.h = name, make, w, h
        self.env = dict(BRUTE if env is None else env)
        self.off, self.stride, self.background, self.view, self.stats = off, stride, background, view, stats
        self.extreme = extreme
        # (only the stress scenes, far beyond the default threshold of 64, run without BWRT_BVH_MIN)
        self.bvh = self.env.get("BWRT_BVH_MIN", "1") == "1"

    def __repr__(self):
        return self.name


def _random(seed):
    s = _random_scene(seed)
    if seed % 4 == 2:
        s = _scaled(s, 1e3 if seed % 8 == 2 else 1e-3)
    return s


def _cases():
    out = []
    for name in ("01", "04", "04_box", "07"):
        for path, env in PATHS.items():
            out.append(Case(f"{name}-{path}", scenes.SCENES[name], 67, 45, env))
    out.append(Case("stress-bvh", stress, 99, 54, {}))
    # (the guide kernel and the CPU walk read the 32-byte nodes either way; the knob hides the
    # 16-byte ones from the render kernels, whose pins run in this configuration too)
    out.append(Case("stress-bvh-n16_0", stress, 99, 54, {"BWRT_BVH_N16": "0"}))
    for mask in (7, 1):
        out.append(Case(f"stress-bvh-mask{mask}", stress, 99, 54, {"BWRT_BVH_ORDER_MASK": str(mask)},
                        stats=f"octant mask {mask},"))
    out.append(Case("stress400-brute", functools.partial(stress, 400, 8), 48, 27, BRUTE))
    for seed in range(24):
        path = "bvh" if seed % 2 else "brute"
        out.append(Case(f"random{seed}-{path}", functools.partial(_random, seed), 40, 23, PATHS[path]))
    # The six listed scales give NaN depths (1e15, 1e19: every pixel) but no inf depth on a hit: a
    # NaN distance, once accepted, stays.  An inf depth needs a polygon whose plane test overflows to
    # t = inf (n.o ~ scale^3) with nothing finite accepted after it: 3e12 (a triangle) and 4e12 (a
    # quad), found by scanning the oracle, added for that.
    for seed, k in ((3, 1e6), (5, 1e10), (7, 1e-6), (9, 1e-10), (11, 1e15), (13, 1e19), (7, 3e12), (15, 4e12)):
        for path, env in PATHS.items():
            out.append(Case(f"random{seed}x{k:g}-{path}", lambda seed=seed, k=k: _scaled(_random_scene(seed), k),
                            32, 18, env, extreme=True))
    # Scales at which only some of a frame's rays fail bvh_safe (its bounds grow with max |d_i|, which
    # runs from 0.58 to 1 over a frame): lanes of one wave leave the wave-synchronous walk for the
    # brute-force loop while their neighbours stay in it (found with bvh_safe() below: 329, 351 and
    # 595 of 920 pixels, spread over nearly every wave).
    for seed, k in ((3, 3.1e4), (7, 3.3e4), (9, 3.5e4)):
        out.append(Case(f"random{seed}x{k:g}-bvh", lambda seed=seed, k=k: _scaled(_random_scene(seed), k), 40, 23, BVH))
    for path, env in PATHS.items():
        out.append(Case(f"07-moved-{path}", scenes.scene_07, 67, 45, env, view="set_camera"))
        out.append(Case(f"07-controls-{path}", scenes.scene_07, 67, 45, env, view="controls"))
        out.append(Case(f"07-background-{path}", scenes.scene_07, 67, 45, env, background=(0.125, 0.5, 0.75)))
    for off, stride in ((1, 3), (5, 8)):
        out.append(Case(f"07-shard{off}of{stride}-brute", scenes.scene_07, 67, 45, BRUTE, off, stride))
        out.append(Case(f"stress-shard{off}of{stride}-bvh", stress, 99, 54, {}, off, stride))
    return out


CASES = _cases()
# Frames whose last wave (64 lanes) and last block (256) of the guide kernel are partial or absent:
# on the BVH path the lanes past the end stay in the wave-synchronous walk with a clamped pixel.
# (At width 1 the screen distance -(W/2) / tan(fov/2) is -0 and the centre ray 0/0: a NaN
# direction, which the walk hands to the brute-force loop.)
SHAPES = ((1, 1), (63, 1), (65, 1), (255, 1), (257, 1), (5, 3), (99, 54))
SHAPE_CASES = [Case(f"stress-bvh-{w}x{h}", stress, w, h, {}) for w, h in SHAPES] + \
              [Case(f"07-brute-{w}x{h}", scenes.scene_07, w, h, BRUTE) for w, h in SHAPES]
BY_NAME = {c.name: c for c in CASES + SHAPE_CASES}
assert len(BY_NAME) == len(CASES + SHAPE_CASES)


def moved_camera(scene):
    """The scene's camera moved and turned (MOVED), its field of view kept."""
    pos, ang = MOVED
    return Camera(Vec3(*pos), (C.c_float * 2)(*ang), scene.camera.fov)


def run_case(r, case, monkeypatch, capfd):
    """The guides of `case` on renderer r and the scene as r sees it (its
    camera the one r ended up with).  The BWRT_BVH_STATS line on stderr shows
    that the scene took the path the case names.  The knobs are gone again
    afterwards; the background is put back."""
    scene = case.make()
    knobs = {**case.env, "BWRT_BVH_STATS": "1"}
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    r.set_background(*case.background)
    try:
        r.set_scene(scene)
        if case.view:
            r.set_camera(moved_camera(scene))
            if case.view == "controls":
                assert r.controls(["W", "LEFT", "UP"], 0.05) == 1
            scene.set_camera(r.get_camera())
        got = r.render_aov(case.w, case.h, case.off, case.stride)
    finally:
        r.set_background(0.0, 0.0, 0.0)
        for k in knobs:
            monkeypatch.delenv(k, raising=False)
    err = capfd.readouterr().err
    assert ("bvh:" in err) == case.bvh, (case, err)
    if case.stats:
        assert case.stats in err, (case.stats, err)
    return got, scene


_WANT = {}


def want(oracle, case, scene):
    """oracle.first_hit of the case (computed once per case; `scene` is the one
    run_case returned, or a fresh case.make() for a case without a view)."""
    if case.name not in _WANT:
        _WANT[case.name] = oracle.first_hit(scene, case.w, case.h, case.off, case.stride, background=case.background)
        for a in _WANT[case.name].values():
            a.setflags(write=False)
    return _WANT[case.name]


def differences(got, ref):
    """The guide arrays that are not bit for bit the oracle's (NaN == NaN)."""
    return [k for k in KEYS if not (got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k], equal_nan=True))]


def check_case(r, oracle, case, monkeypatch, capfd):
    got, scene = run_case(r, case, monkeypatch, capfd)
    ref = want(oracle, case, scene)
    assert differences(got, ref) == [], case
    return got, ref, scene


# ---- which pixels leave the BVH walk for the brute-force loop ------------------
def bvh_safe(scene, w, h, off=0, stride=1):
    """rt_path.h bvh_safe per shard pixel, restated for the tests' report of
    which cases reach the fall-back (not a bit-exact twin: float64 directions
    rounded to float32, which only matters exactly at a threshold).  The
    bounds are rt_scene.cpp's ovf_sc / ovf_nm / ovf_im."""
    f32 = np.float32
    ns, _, nt, nq = scene.counts
    sc = rmax = nm = im = 0.0

    def upd(b, x):
        a = np.abs(np.asarray(x, np.float64))
        return np.inf if np.isnan(a).any() else max(b, float(a.max()))
    for i in range(ns):
        s = scene.spheres[i]
        sc = upd(sc, [s.position.x, s.position.y, s.position.z])
        rmax = upd(rmax, s.radius)
    with np.errstate(all="ignore"):
        for arr, n, nv in ((scene.triangles, nt, 3), (scene.quads, nq, 4)):
            if n == 0:
                continue
            v = np.array([[[q.x, q.y, q.z] for q in arr[i].vertices] for i in range(n)], f32)  # (n, nv, 3)
            sc = upd(sc, v)
            e = np.roll(v, -1, 1) - v
            nrm = _cross32(e[:, 0], e[:, 1])
            nm = upd(nm, nrm)
            for k in range(nv):
                im = upd(im, _cross32(nrm, e[:, k]))
        S, N, I = (f32(min(x * (1.0 + 1e-6), 3e38)) for x in (sc + rmax, nm, im))
        cam = scene.camera
        om = f32(max(abs(cam.position.x), abs(cam.position.y), abs(cam.position.z)))
        ys = np.arange(off, h, stride)
        dm = np.abs(R.primary_dirs(cam, w, h, ys)).max(-1).astype(f32)
        ok = ((om + S < f32(1e18)) & (dm < f32(1e18)) & (dm > f32(1e-15)) & (dm * (om + S) < f32(1e18)) &
              (N * dm < f32(1e36)) & (N * (om + f32(3) * S) < f32(1e33)))
        pm = om + S + f32(6e4) * dm * (N * (om + f32(3) * S))
        return ok & (pm < f32(1e37)) & (I * pm < f32(3e36))


def _cross32(a, b):
    """Math.cuh:103-108 in float32 over (..., 3) arrays."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], -(a[..., 0] * b[..., 2] - a[..., 2] * b[..., 0]),
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def report(case, ref, scene):
    """One line per case: hits, NaN / inf depths among them, and (BVH cases)
    the pixels whose ray fails bvh_safe and takes the brute-force loop."""
    hit = ref["prim"] >= 0
    nan = int(np.isnan(ref["depth"][hit]).sum())
    inf = int(np.isinf(ref["depth"][hit]).sum())
    fb = int((~bvh_safe(scene, case.w, case.h, case.off, case.stride)).sum()) if case.bvh else 0
    print(f"{case.name}: {hit.size} pixels, {int(hit.sum())} hits, NaN depth {nan}, inf depth {inf}, "
          f"bvh_safe fall-back {fb if case.bvh else '-'}")
    return nan, inf, fb


# ---- the tie scene --------------------------------------------------------------
def tie_scene():
    """Every primitive twice at the same coordinates, the copy (with another
    albedo) after all the originals of its kind: one sphere, one plane (a wall
    behind everything, so every ray hits), one triangle, one quad and the 07
    pyramid with its shared edges.  The reference accepts an equal distance
    (Intersection.cuh: t > closest rejects), so the primitive tested later —
    the copy — must win every pixel.  Returns (scene, the set of the copies'
    prim ids)."""
    m = scenes.material
    first, second = (lambda i: m((0.25, 0.1 * i, 0.3))), (lambda i: m((0.75, 0.1 * i, 0.7), 0.0, 0.5))
    v = scenes.vec
    cam = Camera(v(0, 1, 0), (C.c_float * 2)(0.05, -0.1), 1.4)
    pyr = [t.vertices for t in scenes._pyramid()]
    tri_v = [(Vec3 * 3)(v(0.5, 0.2, -3), v(2.0, 0.3, -3.2), v(1.2, 1.8, -2.9))] + pyr
    sph, pln, tri, quad = [], [], [], []
    for mat in (first, second):
        sph.append(Sphere(v(0.2, 2.2, -5), 1.0, mat(0)))
        pln.append(Plane(v(0, 0, -12), (Vec3 * 2)(v(1.5, 0, 0), v(0, 2, 0)), mat(1)))
        tri += [Triangle(tv, mat(2 + k)) for k, tv in enumerate(tri_v)]
        quad.append(Quad((Vec3 * 4)(v(-4, 0.1, -6), v(-2.5, 0.2, -6.5), v(-2.4, 2.0, -6.4), v(-4.1, 1.9, -5.9)), mat(7)))
    scene = scenes.Scene(cam, sph, pln, tri, quad, name="ties")
    nt = len(tri_v)
    copies = {1, 2 + 1} | {4 + nt + k for k in range(nt)} | {4 + 2 * nt + 1}
    return scene, copies
