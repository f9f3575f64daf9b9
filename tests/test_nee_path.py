"""The next-event-estimation path loop against an independent replay of every
pixel's path — CPU only.

tests/nee_path_ref.py is a fourth text of the loop (beside the two placements
of the shadow ray in csrc/rt_kernel_lane.h and trace_path<NEE> of
csrc/rt_cpu.cpp), written from the specification and composed of pinned
blocks: the oracle's camera ray, closest hit and scattering, the host pass of
build/neeprobe_cpu for nee_normal_kind, nee_sample and light_suppressed, and a
float32 fold.  Here:

(a) the driver proves itself: with light sampling off, and with it on over an
    empty light table, it equals orc_render_rows bit for bit;
(b) no vacuous pass: on the driver's level records alone, every situation the
    loop has to get right occurs in the case matrix, each at least 16 times and
    in every scene built for it;
(c) the CPU twin (Renderer.cpu, set_light_sampling(True)) equals the driver:
    frameSum and RNG state bit for bit, every pixel, no tolerance — and the
    RGBA the oracle's tone mapping makes of the driver's frameSum.

tests/test_gpu_nee_path.py holds the HIP kernels to the same driver results.
`python tests/test_nee_path.py` prints the coverage table of
profiles/nee_path/coverage.txt.
"""
if __name__ == "__main__":
    import conftest  # noqa: F401  (the import paths of the suite)

import collections
import ctypes as C
import pathlib
import tempfile

import numpy as np
import pytest

import nee_cases as K
import nee_path_ref as D
import scenegen
import test_light_sampling as LS
import test_light_shapes as S
from bwrt import Renderer, scenes
from bwrt.abi import Camera, Plane, Quad, Sphere, Vec3
from bwrt.scenes import material, vec
from test_adaptive import DEFAULTS

W, H, FRAMES = 32, 18, 2
PICKS, SHAPES = ("uniform", "weighted"), ("spheres", "all")
MODES = [(p, s) for s in (0, 1) for p in (0, 1)]


# ---- scenes --------------------------------------------------------------------------------

def camera_inside_a_light():
    s = scenes.scene_07()
    cam = scenes.camera_07()
    cam.position = vec(-6, 3, -4)  # the centre of light 0
    s.set_camera(cam)
    return s


def light_touching_the_floor():
    s = scenes.scene_07()  # the green light: centre y 0.2, radius 0.2; the camera next to it
    cam = scenes.camera_07()
    cam.position = vec(-0.5, 0.3, -2.0)
    s.set_camera(cam)
    return s


def scaled_floor(z):
    """Scene 07 over a floor whose normal is cross((0, 0, z), (1, 0, 0)) = (0, z, 0)"""
    s = scenes.scene_07()
    n = s.counts
    floor = Plane(vec(0, 0, 0), (Vec3 * 2)(vec(0, 0, z), vec(1, 0, 0)), material((0.5, 0.5, 0.5)))
    return scenes.Scene(s.camera, list(s.spheres)[:n[0]], [floor], list(s.triangles)[:n[2]], [], name=f"floor_n{z:g}")


def far_wall():
    """Coordinates near 1e4 in x and z, where a float step is 1e-3 — ten times the
    reference's near-zero distance: an emissive wall (normal (10, 0, 28): both
    large coordinates reach its plane equation) fills the view, and a ray
    scattered off it can re-hit it at once: the level's own primitive, a table
    light that is not reachable.  Beside it a sphere light, a sphere light sunk
    into the floor (floor points inside a light) and a dark sphere."""
    x, z = 10000.0, -10000.0
    cam = Camera(vec(x, 1, z), (C.c_float * 2)(0.0, 0.0), float(scenes.PI / np.float32(2)))
    sph = [Sphere(vec(x - 2, 3, z - 2), 0.5, material((1, 0.6, 0.2), 20)),
           Sphere(vec(x + 1.5, 0.1, z - 2.5), 0.3, material((0.2, 0.8, 0.2), 10)),
           Sphere(vec(x, 0.75, z - 3), 0.75, material((1, 1, 1), 0, 1))]
    wall = Quad((Vec3 * 4)(vec(x - 4, 0, z - 4), vec(x + 3, 0, z - 6.5), vec(x + 3, 4, z - 6.5), vec(x - 4, 4, z - 4)),
                material((1, 0.9, 0.7), 2))
    return scenes.Scene(cam, sph, [scenes._floor()], [], [wall], name="far_wall")


SCENES = {
    "07": scenes.scene_07,
    "mixed": S.mixed,                                    # quad lights beside sphere lights; the pyramid's |n|^2 = 1.25
    "small_light0": lambda: K.small_light_scene(0),
    "small_light64": lambda: K.small_light_scene(64),    # a BVH scene on the GPU
    "occluder": lambda: LS.hidden_light_scene(50.0),     # a light in the middle of an opaque sphere
    "camera_in_light": camera_inside_a_light,
    "light_on_floor": light_touching_the_floor,
    "floor_n4": lambda: scaled_floor(2.0),               # |n|^2 = 4: kind 2
    "floor_n049": lambda: scaled_floor(0.7),             # |n|^2 = 0.49 <= 1/2: no level on the floor
    "far_wall": far_wall,
}

Case = collections.namedtuple("Case", "scene pick shapes w h mb spp off stride")


def _case(scene, pick, shapes, w=W, h=H, mb=4, spp=1, off=0, stride=1):
    return Case(scene, pick, shapes, w, h, mb, spp, off, stride)


CASES = [_case(s, p, sh) for s in SCENES for p, sh in MODES]
CASES += [_case("07", p, sh, mb=mb) for mb in (0, 1) for p, sh in ((0, 0), (1, 1))]
CASES += [_case("light_on_floor", 0, 0, spp=2), _case("light_on_floor", 1, 0, spp=2),   # the camera sees a sphere light
          _case("far_wall", 0, 1, spp=2), _case("far_wall", 1, 1, spp=2, mb=1)]         # ... a polygon light
CASES += [_case("07", 0, 0, off=1, stride=3), _case("mixed", 1, 1, w=37, h=11)]


def case_id(c):
    tail = "".join([f"-mb{c.mb}" if c.mb != 4 else "", f"-spp{c.spp}" if c.spp != 1 else "",
                    f"-rows{c.off}+{c.stride}" if c.stride != 1 else "", f"-{c.w}x{c.h}" if (c.w, c.h) != (W, H) else ""])
    return f"{c.scene}-{PICKS[c.pick]}-{SHAPES[c.shapes]}{tail}"


IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)

# ---- driver results, computed once per case and shared (tests/test_gpu_nee_path.py reads them too) ----

_TMP = []
_WORDS = {}
_RESULTS = {}


def tmp_dir():
    if not _TMP:
        _TMP.append(tempfile.TemporaryDirectory(prefix="nee_path"))
    return pathlib.Path(_TMP[0].name)


def table_of(name, make=None):
    if name not in _WORDS:
        _WORDS[name] = D.light_words((make or SCENES[name])(), tmp_dir(), name)
        _WORDS[name].setflags(write=False)
    return _WORDS[name]


def driver_result(c, frames=FRAMES, snapshots=()):
    """dict(sum, rng, rgba, levels) of the driver on case c, read-only; snapshots:
    frame counts at which (sum, rng, rgba) are kept besides (key "at")"""
    key = (c, frames, tuple(snapshots))
    if key not in _RESULTS:
        d = D.Driver(SCENES[c.scene](), c.w, c.h, table_of(c.scene), tmp_dir(), pick=c.pick, shapes=c.shapes,
                     samples_per_pixel=c.spp, row_offset=c.off, row_stride=c.stride)
        at = {}
        for f in range(1, frames + 1):
            d.render(1, c.mb)
            if f in snapshots:
                at[f] = (d.frame_sum(), d.rng_state(), D.tonemap(d.frame_sum(), f))
        res = dict(sum=d.frame_sum(), rng=d.rng_state(), rgba=D.tonemap(d.frame_sum(), frames), levels=d.levels, at=at,
                   n_lights=d.n_lights)
        for a in (res["sum"], res["rng"], res["rgba"], res["levels"]):
            a.setflags(write=False)
        _RESULTS[key] = res
    return _RESULTS[key]


def product_state(r, c, frames=FRAMES):
    """(frameSum, RNG state, RGBA) of renderer r on case c"""
    r.set_scene(SCENES[c.scene]())
    r.set_light_sampling(True)
    r.set_light_picking(PICKS[c.pick])
    r.set_light_shapes(SHAPES[c.shapes])
    r.set_samples_per_pixel(c.spp)
    img = r.render(c.w, c.h, frames, c.mb, first_frame=1, row_offset=c.off, row_stride=c.stride)
    rng, acc = r.get_state(img.shape[0], c.w)
    return acc, rng, img


def assert_equals_driver(got, want, what):
    acc, rng, img = got
    bad = np.nonzero(rng != want["rng"])
    assert len(bad[0]) == 0, (what, "RNG state", len(set(zip(bad[1], bad[2]))), "pixels, first", bad[1][:4], bad[2][:4])
    same = (acc.view(np.uint32) == want["sum"].view(np.uint32)) | (np.isnan(acc) & np.isnan(want["sum"]))
    bad = np.nonzero(~same.all(-1))
    assert len(bad[0]) == 0, (what, "frameSum", len(bad[0]), "pixels, first", bad[0][:4], bad[1][:4],
                              acc[bad][:2], want["sum"][bad][:2])
    assert np.array_equal(img, want["rgba"]), (what, "RGBA")


# ---- (a) the driver proves itself ------------------------------------------------------------

OFF_SCENES = dict(scenes.SCENES)
OFF_SCENES.update({"guard": scenegen.guard_scene, "random0": lambda: scenegen._random_scene(0),
                   "random1": lambda: scenegen._random_scene(1)})
assert "04_box" in OFF_SCENES and len(OFF_SCENES) == 9


def oracle_state(oracle, scene, w, h, mb, spp, off=0, stride=1):
    st = oracle.OracleState(w, h, off, stride)
    oracle.render(scene, st, FRAMES, mb, first_frame=1, samples_per_pixel=spp)
    return st


def assert_equals_oracle(d, st):
    assert np.array_equal(d.rng_state(), st.rng)
    assert D.same_bits(d.frame_sum(), st.accum)
    assert np.array_equal(D.tonemap(d.frame_sum(), FRAMES), st.rgba)


@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("mb", [0, 1, 4])
@pytest.mark.parametrize("name", list(OFF_SCENES))
def test_driver_equals_the_oracle_without_light_sampling(oracle, name, mb, spp):
    scene = OFF_SCENES[name]()
    d = D.Driver(scene, W, H, None, tmp_dir(), light_sampling=False, samples_per_pixel=spp)
    d.render(FRAMES, mb)
    assert_equals_oracle(d, oracle_state(oracle, scene, W, H, mb, spp))
    assert d.probe_runs == 0 and (len(d.levels) > 0 or name == "empty")


def test_driver_equals_the_oracle_on_a_row_shard(oracle):
    scene = scenes.scene_07()
    d = D.Driver(scene, 37, 11, None, tmp_dir(), light_sampling=False, row_offset=1, row_stride=3)
    d.render(FRAMES, 4)
    assert_equals_oracle(d, oracle_state(oracle, scene, 37, 11, 4, 1, 1, 3))


EMPTY = [("dark_07", LS.dark_07, p, sh) for p, sh in MODES] + [("empty", scenes.empty_scene, 0, 1)] + \
        [("triangle_light", LS.triangle_light_scene, p, 0) for p in (0, 1)]  # a polygon emitter, unseen in the spheres mode


@pytest.mark.parametrize("name,make,pick,shapes", EMPTY, ids=[f"{n}-{PICKS[p]}-{SHAPES[s]}" for n, _, p, s in EMPTY])
def test_driver_equals_the_oracle_over_an_empty_table(oracle, name, make, pick, shapes):
    scene = make()
    d = D.Driver(scene, W, H, table_of(name, make), tmp_dir(), pick=pick, shapes=shapes, samples_per_pixel=2)
    d.render(FRAMES, 4)
    assert d.n_lights == 0 and d.probe_runs == 0
    assert_equals_oracle(d, oracle_state(oracle, scene, W, H, 4, 2))


def test_tonemap_is_the_oracles(oracle):
    """the RGBA the driver's results carry: the oracle's own frame after 2 and after 3 frames"""
    scene = scenes.scene_07()
    st = oracle.OracleState(W, H)
    for frames in (2, 3):
        oracle.render(scene, st, 2 if frames == 2 else 1, 4, first_frame=1 if frames == 2 else None)
        assert np.array_equal(D.tonemap(st.accum, frames), st.rgba)


# ---- (b) no vacuous pass ----------------------------------------------------------------------

SITUATIONS = ["not traced", "traced, not visible", "traced, visible", "dropped emission", "unreachable light hit, emission kept",
              "level on a light", "kind 2", "diffuse at max_bounces", "inner path behind a level", "... whose camera ray hits a light"]
# the scenes built for a situation: each of their cases in a mode that can show it must
NAMED = {
    "not traced": ["camera_in_light", "far_wall", "floor_n4"],
    "traced, not visible": ["occluder", "07"],
    "traced, visible": ["07", "mixed", "small_light0", "small_light64", "light_on_floor", "floor_n4", "far_wall"],
    "dropped emission": ["07", "mixed", "light_on_floor"],
    "unreachable light hit, emission kept": ["far_wall"],   # (all shapes: the wall is a table light there)
    "level on a light": ["07", "light_on_floor", "far_wall"],
    "kind 2": ["mixed", "floor_n4", "far_wall", "07"],
    "diffuse at max_bounces": ["07", "mixed", "occluder"],
    "inner path behind a level": ["light_on_floor", "far_wall"],
    "... whose camera ray hits a light": ["light_on_floor", "far_wall"],
}
MINIMUM = 16


def situations(c, lv):
    """the count of every situation among the level records of case c"""
    aux = lv["aux"]
    level, visible, drop = (aux & D.LEVEL) != 0, (aux & D.VISIBLE) != 0, (aux & D.DROP) != 0
    return dict(zip(SITUATIONS, (int(x.sum()) for x in (
        level & ~lv["traced"], level & lv["traced"] & ~visible, level & visible, drop,
        lv["asked"] & lv["on_light"] & ~drop, level & lv["on_light"], level & (lv["kind"] == 2),
        ~lv["specular"] & (lv["depth"] == c.mb) & (c.mb > 0), lv["inherit"], lv["inherit"] & lv["on_light"]))))


def coverage():
    return [(case_id(c), situations(c, driver_result(c)["levels"]), len(driver_result(c)["levels"])) for c in CASES]


def coverage_table():
    rows = coverage()
    lines = ["situation columns: " + "; ".join(f"{i}: {s}" for i, s in enumerate(SITUATIONS)), "",
             f"{'case':40s} {'levels':>6s} " + " ".join(f"{i:>5d}" for i in range(len(SITUATIONS)))]
    for name, s, n in rows:
        lines.append(f"{name:40s} {n:6d} " + " ".join(f"{s[k]:5d}" for k in SITUATIONS))
    total = {k: sum(s[k] for _, s, _ in rows) for k in SITUATIONS}
    lines.append(f"{'total':40s} {sum(n for _, _, n in rows):6d} " + " ".join(f"{total[k]:5d}" for k in SITUATIONS))
    return "\n".join(lines)


def test_every_situation_occurs():
    """On the driver's level records alone, before the product is consulted."""
    rows = dict((name, s) for name, s, _ in coverage())
    print(coverage_table())
    for k in SITUATIONS:
        assert sum(s[k] for s in rows.values()) >= MINIMUM, k
    for k, names in NAMED.items():
        for c in CASES:
            if c.scene not in names or c.mb != 4:
                continue
            if k.startswith(("inner path", "...")) and c.spp == 1:
                continue
            if k == "unreachable light hit, emission kept" and c.shapes == 0:
                continue
            assert rows[case_id(c)][k] > 0, (k, case_id(c))
    # a level's tuple is what it says
    lv = driver_result(CASES[0])["levels"]
    assert (lv["frame"] >= 1).all() and (lv["frame"] <= FRAMES).all() and (lv["depth"] <= 4).all() and (lv["pixel"] < W * H).all()
    assert ((lv["aux"] & D.VISIBLE) == 0)[(lv["aux"] & D.LEVEL) == 0].all()


def test_the_draws_of_a_level_do_not_depend_on_the_pick():
    """The four modes of one scene: the same paths (levels, primitives, RNG
    state) wherever the tables agree — the pick changes k and the shadow ray only."""
    for name in ("07", "occluder", "small_light64"):  # no polygon emitter: the four tables are one
        res = [driver_result(_case(name, p, sh)) for p, sh in MODES]
        for r in res[1:]:
            assert np.array_equal(r["rng"], res[0]["rng"])
            for f in ("pixel", "frame", "depth", "prim", "specular", "kind"):
                assert np.array_equal(r["levels"][f], res[0]["levels"][f])
        assert not D.same_bits(res[0]["sum"], res[1]["sum"]) or name == "small_light64"  # (one light: the picks agree)
    for name in ("mixed", "far_wall"):  # both tables are non-empty: the same draws again, another frame per shapes mode
        res = [driver_result(_case(name, p, sh)) for p, sh in MODES]
        for r in res[1:]:
            assert np.array_equal(r["rng"], res[0]["rng"])
        assert not D.same_bits(res[0]["sum"], res[2]["sum"])


# ---- (c) the CPU twin against the driver -----------------------------------------------------

@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_cpu_twin_equals_the_driver(bwrt_lib, c):
    want = driver_result(c)
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        got = product_state(r, c)
    assert len(want["levels"]) > 0 and got[0].shape == want["sum"].shape
    assert_equals_driver(got, want, case_id(c))


# the same results through the BVH walk (BWRT_BVH_MIN=1: the scene's geometry does not change), and at 12 bounces
# (not the far wall: a shadow ray that starts 1e4 away from a sphere leaves the sphere test's discriminant to
# rounding alone, the reference's loop "hits" the sphere 4 radii off its centre, and the BVH walk, which prunes by
# the sphere's box, does not — DESIGN.md section 27, a finding about the walk and not about this loop)
FORCED_BVH = [_case("07", 0, 0), _case("07", 1, 0), _case("mixed", 0, 1), _case("mixed", 1, 1), _case("light_on_floor", 0, 0, spp=2)]
DEEP = [_case("07", 0, 0, mb=12), _case("07", 1, 1, mb=12)]
assert all(c in CASES for c in FORCED_BVH)


@pytest.mark.parametrize("c", FORCED_BVH + DEEP, ids=[case_id(c) for c in FORCED_BVH + DEEP])
def test_cpu_twin_bvh_and_deep_paths_equal_the_driver(bwrt_lib, monkeypatch, c):
    if c in FORCED_BVH:
        monkeypatch.setenv("BWRT_BVH_MIN", "1")
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        got = product_state(r, c)
    assert_equals_driver(got, driver_result(c), case_id(c))


def test_cpu_twin_continues_as_the_driver_does(bwrt_lib):
    """2 + 1 frames in two calls: the accumulation goes on, frame 1 alone resets it"""
    c = _case("07", 1, 1)
    want = driver_result(c, 3)
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        product_state(r, c)
        img = r.render(c.w, c.h, 1, c.mb)
        rng, acc = r.get_state(c.h, c.w)
    assert_equals_driver((acc, rng, img), want, "2 + 1 frames")


def adaptive_call(r, c, start=(2, 2), samples=2):
    """A uniform start, then one adaptive call: counts, state and image"""
    r.set_scene(SCENES[c.scene]())
    r.set_light_sampling(True)
    r.set_light_picking(PICKS[c.pick])
    r.set_light_shapes(SHAPES[c.shapes])
    r.init_rand(c.w, c.h)
    r.set_moments(True)
    for i, k in enumerate(start):
        r.render(c.w, c.h, k, c.mb, first_frame=1 if i == 0 else 0)
    img, col, st = r.render_adaptive(c.w, c.h, c.mb, want_color=True, samples=samples, **DEFAULTS)
    n = r.counts(c.h, c.w)[0]
    rng, acc = r.get_state(c.h, c.w)
    return dict(n=n, rng=rng, accum=acc, rgba=img, selected=st["selected"])


def assert_replays_the_driver(res, c, frames):
    want = driver_result(c, max(frames), snapshots=frames)["at"]
    n = res["n"]
    assert set(np.unique(n)) == set(frames) and 0 < res["selected"] < c.w * c.h
    for f in frames:
        m = n == f
        acc, rng, img = want[f]
        assert np.array_equal(res["rng"][:, m], rng[:, m]), f
        assert ((res["accum"][m].view(np.uint32) == acc[m].view(np.uint32)) | (np.isnan(res["accum"][m]) & np.isnan(acc[m]))).all(), f
        assert np.array_equal(res["rgba"][m], img[m]), f


LISTED = _case("07", 0, 0, w=67, h=45)



def test_cpu_list_form_replays_the_driver(bwrt_lib):
    """One adaptive call under NEE on 07 at 67 x 45 (4 uniform frames, then 2 more
    on the selected pixels): every pixel holds the driver's frameSum, RNG state
    and RGBA after its own number of frames."""
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        res = adaptive_call(r, LISTED)
    assert_replays_the_driver(res, LISTED, (4, 6))


if __name__ == "__main__":
    print(coverage_table())
