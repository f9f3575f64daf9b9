"""The light hierarchy of weighted light picking (rt_set_light_hierarchy,
csrc/rt_light.h) on the CPU backend — no GPU needed.  The
HIP kernels compute the same bits (tests/test_gpu_light_tree.py).

What is checked here: the interface; that the switch changes nothing where it
cannot act; that the path does not depend on it; the tree's invariants through
rt_get_light_tree; the pick probabilities of rt_light_pick_probabilities against
tests/light_tree_ref.py, a float64 restatement of the specification; that the
hierarchy has the default estimator's expectation (the z protocol of
tests/test_light_sampling.py) and where its variance stands; shards, adaptive
calls, toggling, the downstream passes and the CLI.
"""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import light_tree_ref as ref
from bwrt import Renderer, abi, scenes
from bwrt.abi import Sphere
from bwrt.scenes import material, vec
from light_tree_cases import TABLES, far_points, points_of, renderer, sixty_four_lights
from test_adaptive import adaptive_sequence, check_replay
from test_light_picking import (black_light_scene, block_means, eight_lights, runs as picking_runs, small_normal_scene)
from test_light_sampling import (CLI, assert_same_expectation, dark_07, hidden_light_scene, read_ppm, same_state, state,
                                 triangle_light_scene, z_scores)
from test_light_shapes import mixed


def cpu(lib, scene, pick="weighted", hierarchy=True, on=True, shapes="spheres", threads=0):
    r = Renderer.cpu(threads, lib=lib)
    r.set_scene(scene)
    r.set_light_sampling(on)
    r.set_light_picking(pick)
    r.set_light_shapes(shapes)
    r.set_light_hierarchy(hierarchy)
    return r


W0, H0 = 67, 45


# ---- interface, and where the switch cannot act ---------------------------------------

def test_abi_and_defaults(bwrt_lib):
    names = {"rt_set_light_hierarchy", "rt_get_light_hierarchy", "rt_get_light_tree", "rt_light_pick_probabilities"}
    assert names <= set(abi.declared_functions())
    for n in names:
        assert hasattr(bwrt_lib, n)
    assert abi.RT_LIGHT_NODE_FLOATS == 8
    with Renderer.cpu(1, lib=bwrt_lib) as r:
        assert r.light_hierarchy is False and bwrt_lib.rt_get_light_hierarchy(r.ctx) == 0
        assert bwrt_lib.rt_get_light_tree(r.ctx, None, 0) == abi.RT_ERR_NO_SCENE
        assert bwrt_lib.rt_light_pick_probabilities(r.ctx, None, None, 0, None) == abi.RT_ERR_NO_SCENE
        r.set_light_hierarchy(True)
        assert r.light_hierarchy is True and bwrt_lib.rt_get_light_hierarchy(r.ctx) == 1
        # stored independently of the other switches
        assert r.light_sampling is False and r.light_picking == "uniform" and r.light_shapes == "spheres"
        for bad in (2, -1, 7):
            assert bwrt_lib.rt_set_light_hierarchy(r.ctx, bad) == abi.RT_ERR_INVALID_ARGUMENT
            assert "rt_set_light_hierarchy" in bwrt_lib.rt_last_error(r.ctx).decode()
        assert r.light_hierarchy is True
        r.set_light_picking("weighted")
        r.set_light_picking("uniform")
        assert r.light_hierarchy is True
        # rt_set_light_picking keeps its two values
        assert bwrt_lib.rt_set_light_picking(r.ctx, 2) == abi.RT_ERR_INVALID_ARGUMENT
        r.set_light_hierarchy(False)
        assert r.light_hierarchy is False
    assert bwrt_lib.rt_set_light_hierarchy(None, 1) == bwrt_lib.rt_set_light_picking(None, 1) == abi.RT_ERR_INVALID_ARGUMENT
    assert bwrt_lib.rt_get_light_hierarchy(None) == 0
    assert bwrt_lib.rt_get_light_tree(None, None, 0) == abi.RT_ERR_INVALID_ARGUMENT
    assert bwrt_lib.rt_light_pick_probabilities(None, None, None, 0, None) == abi.RT_ERR_INVALID_ARGUMENT


def test_bad_arguments_of_the_readbacks(bwrt_lib):
    with cpu(bwrt_lib, scenes.scene_07()) as r:
        assert bwrt_lib.rt_get_light_tree(r.ctx, None, 1) == abi.RT_ERR_INVALID_ARGUMENT
        assert bwrt_lib.rt_get_light_tree(r.ctx, None, -1) == abi.RT_ERR_INVALID_ARGUMENT
        assert bwrt_lib.rt_light_pick_probabilities(r.ctx, None, None, 1, None) == abi.RT_ERR_INVALID_ARGUMENT
        assert bwrt_lib.rt_light_pick_probabilities(r.ctx, None, None, -1, None) == abi.RT_ERR_INVALID_ARGUMENT
        assert bwrt_lib.rt_light_pick_probabilities(r.ctx, None, None, 0, None) == 3
        # capacity clips the copy, not the count
        raw = np.full((2, 8), -1.0, np.float32)
        assert bwrt_lib.rt_get_light_tree(r.ctx, raw.ctypes.data_as(C.POINTER(C.c_float)), 1) == 5
        assert np.all(raw[1] == -1.0) and raw[0, 3] == r.light_tree()["r2"][0]
        with pytest.raises(ValueError):
            r.light_pick_probabilities(np.zeros((2, 6), np.float32), np.zeros(3, np.int32))


def test_reference_fast_stays_refused(bwrt_lib):
    """The switch needs no refusal of its own: NEE refuses that mode, a CPU context the mode itself."""
    with cpu(bwrt_lib, scenes.scene_07()) as r:
        assert bwrt_lib.rt_set_precision(r.ctx, abi.RT_PRECISION_REFERENCE_FAST) == abi.RT_ERR_UNSUPPORTED


def test_no_op_with_light_sampling_off(bwrt_lib):
    with cpu(bwrt_lib, scenes.scene_07(), "weighted", False, on=False) as a, cpu(bwrt_lib, scenes.scene_07(), on=False) as b:
        same_state(state(a, W0, H0, 3, 4), state(b, W0, H0, 3, 4))


def test_no_op_with_uniform_picking(bwrt_lib):
    with cpu(bwrt_lib, scenes.scene_07(), "uniform", False) as a, cpu(bwrt_lib, scenes.scene_07(), "uniform", True) as b:
        sa = state(a, W0, H0, 3, 4)
        same_state(sa, state(b, W0, H0, 3, 4))
    with cpu(bwrt_lib, scenes.scene_07(), "weighted", True) as c:
        assert not np.array_equal(sa[1], state(c, W0, H0, 3, 4)[1])  # and where it acts it does


@pytest.mark.parametrize("make,mb", [(dark_07, 4), (triangle_light_scene, 4), (scenes.scene_01, 4), (scenes.scene_07, 0)])
def test_identical_to_the_table_walk_where_it_cannot_act(bwrt_lib, make, mb):
    """An empty table (twice: no emitter, a polygon emitter under "spheres"), a
    one-record table, max_bounces 0"""
    with cpu(bwrt_lib, make(), "weighted", False) as a, cpu(bwrt_lib, make(), "weighted", True) as b:
        same_state(state(a, W0, H0, 3, mb), state(b, W0, H0, 3, mb))
        assert len(b.light_tree()) == 0 or make is scenes.scene_07


def test_one_polygon_record_is_the_table_walk(bwrt_lib):
    with cpu(bwrt_lib, triangle_light_scene(), "weighted", False, shapes="all") as a, \
            cpu(bwrt_lib, triangle_light_scene(), "weighted", True, shapes="all") as b:
        assert len(b.lights()) == 1 and len(b.light_tree()) == 0
        same_state(state(a, W0, H0, 3, 4), state(b, W0, H0, 3, 4))


@pytest.mark.parametrize("name,mb", [("07", 4), ("07", 1), ("stress", 4), ("04_box", 3)])
def test_the_path_does_not_depend_on_the_pick(bwrt_lib, name, mb):
    """Same draws, same rays: the RNG state after a hierarchy render is uniform
    NEE's; frameSum is neither uniform NEE's nor the table walk's."""
    make = scenes.SCENES[name]
    with cpu(bwrt_lib, make(), "uniform") as a, cpu(bwrt_lib, make(), "weighted", True) as b, \
            cpu(bwrt_lib, make(), "weighted", False) as c:
        sa, sb, sc = state(a, W0, H0, 3, mb), state(b, W0, H0, 3, mb), state(c, W0, H0, 3, mb)
    assert np.array_equal(sa[2], sb[2])
    if name == "07":
        assert not np.array_equal(sa[1], sb[1], equal_nan=True)
        assert not np.array_equal(sc[1], sb[1], equal_nan=True)


def test_toggling_inside_one_accumulation(bwrt_lib):
    """The switch resets nothing: walk, tree, uniform over one accumulation
    equals the same calls on contexts that were set once each."""
    w, h = 33, 17
    with cpu(bwrt_lib, scenes.scene_07(), "weighted", False) as r:
        r.render(w, h, 2, 4, first_frame=1)
        rng0, acc0 = r.get_state(h, w)
        r.set_light_hierarchy(True)
        assert r.frame_counter == 3
        same_state(list(r.get_state(h, w)), [rng0, acc0])
        r.render(w, h, 2, 4)
        rng1, acc1 = r.get_state(h, w)
        r.set_light_picking("uniform")
        r.render(w, h, 2, 4)
        assert r.frame_counter == 7
        mixed_state = r.get_state(h, w)
    with cpu(bwrt_lib, scenes.scene_07(), "weighted", True) as r:
        r.init_rand(w, h)
        r.set_state(rng0, acc0, 3)
        r.render(w, h, 2, 4)
        same_state(list(r.get_state(h, w)), [rng1, acc1])
    with cpu(bwrt_lib, scenes.scene_07(), "uniform", False) as r:
        r.init_rand(w, h)
        r.set_state(rng1, acc1, 5)
        r.render(w, h, 2, 4)
        same_state(list(r.get_state(h, w)), list(mixed_state))


# ---- the tree's invariants -------------------------------------------------------------

def leaves_below(tree, n, k):
    if k >= n - 1:
        return [k - (n - 1)]
    return leaves_below(tree, n, int(tree[k]["a"])) + leaves_below(tree, n, int(tree[k]["b"]))


def depth_of(tree, k):
    d = 0
    while tree[k]["parent"] >= 0:
        k = int(tree[k]["parent"])
        d += 1
    return d


@pytest.mark.parametrize("name", list(TABLES))
def test_tree_invariants(bwrt_lib, name):
    _, _, count = TABLES[name]
    with renderer(bwrt_lib, name, hierarchy=False) as r:  # built whether or not the switch is on
        lights, tree = r.lights(), r.light_tree()
        raw = tree.view(np.float32).tobytes()
    with renderer(bwrt_lib, name) as r:
        assert r.light_tree().view(np.float32).tobytes() == raw  # two builds give the same bytes
    n = len(lights)
    assert n == count and len(tree) == 2 * n - 1
    # every table index in exactly one leaf; parents in front of their children
    assert sorted(leaves_below(tree, n, 0)) == list(range(n))
    assert tree[0]["parent"] == -1
    for k in range(n - 1):
        for child in (int(tree[k]["a"]), int(tree[k]["b"])):
            assert k < child < 2 * n - 1 and tree[child]["parent"] == k
    for j in range(n):
        leaf = tree[n - 1 + j]
        assert (leaf["a"], leaf["b"]) == (j, -1)
        assert np.array_equal(leaf["centre"], lights["centre"][j]) and leaf["r2"] == lights["r2"][j]
    # the leaf power of a sphere light, in the float order of the specification
    e = np.abs(lights["emitted"])
    pw = (e[:, 0] + e[:, 1]) + e[:, 2]
    sph = lights["prim"] < renderer_counts(name)
    assert np.array_equal(tree["phi"][n - 1:][sph], (pw * lights["r2"])[sph])
    if name == "quads":  # unit quads: (pw * 1) / pi
        assert np.array_equal(tree["phi"][n - 1:], (pw * np.float32(1.0)) / np.float32(3.1415926535))
    for k in range(n - 1):
        a, b = tree[int(tree[k]["a"])], tree[int(tree[k]["b"])]
        # phi: one float addition of the children's
        assert tree[k]["phi"] == np.float32(a["phi"] + b["phi"])
        # containment, in float64 on the stored floats, no tolerance
        R = math.sqrt(float(tree[k]["r2"]))
        for ch in (a, b):
            d = math.sqrt(((tree[k]["centre"].astype(np.float64) - ch["centre"].astype(np.float64)) ** 2).sum())
            assert R >= d + math.sqrt(float(ch["r2"])), (k, R, d)
    depth = max(depth_of(tree, n - 1 + j) for j in range(n))
    assert depth <= math.ceil(math.log2(n)) + 1
    print(f"{name}: {n} lights, leaf depth at most {depth}")


def renderer_counts(name):
    return TABLES[name][0]().counts[0]


def test_zero_power_leaf_stays_in_the_tree(bwrt_lib):
    with cpu(bwrt_lib, black_light_scene(5.0)) as r:
        t = r.light_tree()
    assert len(t) == 3 and t["phi"][1] == 0.0 and t["phi"][2] > 0 and t["phi"][0] == t["phi"][2]


def test_tree_follows_the_shapes_mode(bwrt_lib):
    with cpu(bwrt_lib, mixed()) as r:
        assert len(r.light_tree()) == 5
        r.set_light_shapes("all")
        assert len(r.light_tree()) == 13


def test_the_tools_eight_lights_is_the_tests(bwrt_lib):
    """tools/light_tree_scenes.py keeps its own eight_lights (a tool imports no
    test): the same bytes as tests/test_light_picking.py's"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "light_tree_scenes.py")
    spec = importlib.util.spec_from_file_location("light_tree_scenes", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.eight_lights().digest() == eight_lights().digest()


# ---- the pick against the float64 reference -------------------------------------------

_POINTS = {}


def point_set(lib, name):
    """(lights, tree, points, prims, kinds, n_sphere_lights, scene sphere count) — once per table"""
    if name not in _POINTS:
        make = TABLES[name][0]
        with renderer(lib, name) as r:
            lights, tree = r.lights(), r.light_tree()
        scene = make()
        pts, prims, kinds = points_of(name, lights, tree, scene)
        nsl = int((lights["prim"] < scene.counts[0]).sum())
        _POINTS[name] = (lights, tree, pts, prims, kinds, nsl, scene.counts[0])
    return _POINTS[name]


@pytest.mark.parametrize("name", list(TABLES))
def test_pick_probabilities_against_the_reference(bwrt_lib, name):
    """Tolerance: tests/light_tree_ref.py derives a first-order relative bound
    per entry from the operations of the specification (u = 2^-24 per rounding,
    summed over the levels of the light's way down; its head has the table),
    doubled here for the second-order terms and the reference's own float64
    rounding.  Nothing in it comes from what the library returns.  The rows of
    the eight tables hold 4,800 points; measured, the largest error over the
    doubled bound is 0.045 (tables "3" and "mixed"), the largest bound 2.0e-3
    (the 40-quad panel: points on a quad see its neighbours edge-on, cb small)."""
    lights, tree, pts, prims, kinds, nsl, nss = point_set(bwrt_lib, name)
    assert set(kinds) == {"floor", "light", "inside", "kind2", "beside"} and len(pts) >= 500
    with renderer(bwrt_lib, name) as r:
        got = r.light_pick_probabilities(pts, prims).astype(np.float64)
        r.set_light_hierarchy(False)
        walk = r.light_pick_probabilities(pts, prims).astype(np.float64)
        r.set_light_picking("uniform")
        uni = r.light_pick_probabilities(pts, prims)
    p, bound, w, ew, least = ref.probabilities(tree, lights, nsl, pts, prims, nss)
    n = len(lights)
    tol = 2.0 * bound * p
    err = np.abs(got - p)
    worst = (err / np.where(tol > 0, tol, np.inf)).max()
    print(f"{name}: {len(pts)} points, largest error / bound {worst:.3f}, largest bound {bound.max():.2e}")
    assert (err <= tol).all()
    # probability 0 exactly where the linear weight is 0 (no underflow at this scale)
    assert np.array_equal(got == 0, w == 0)
    assert np.array_equal(p == 0, w == 0)
    # a row sums to 1, or is all 0 where the rule says no direct term: no light has a weight.  Between
    # the two, where the reference finds a dead end below the root (test_dead_end_below_a_node_is_the_
    # no_pick_rule), the row lacks exactly the reference's no-pick mass.
    none = (w == 0).all(1)
    sums = got.sum(1)
    assert (sums[none] == 0).all()
    mass = ref.no_pick_mass(tree, lights, nsl, pts, prims, nss)
    assert np.array_equal(mass == 1.0, none)
    rowtol = 2.0 * bound.max(1) + n * ref.U
    whole = mass == 0
    assert (np.abs(sums[whole] - 1.0) <= rowtol[whole]).all()
    assert (np.abs(sums + mass - 1.0) <= rowtol)[~none].all()
    print(f"{name}: rows without a direct term {int(none.sum())}, rows with a dead end below the root "
          f"{int((~whole & ~none).sum())} (largest no-pick mass there {mass[~none].max():.3f})")
    # the other two modes through the same call
    W = w.sum(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        pw = np.where(W > 0, w / W, 0.0)
    ewmax = ew.max(1, keepdims=True)
    assert (np.abs(walk - pw) <= 2.0 * (ew + ewmax + (n + 2) * ref.U) * pw).all()
    assert np.array_equal(uni, np.full_like(uni, np.float32(1.0) / np.float32(n)))


def test_dead_end_below_a_node_is_the_no_pick_rule(bwrt_lib):
    """A node has importance wherever its sphere can be seen, its leaves only
    where they are reachable: scene 07's orange and white lights and a
    zero-power light that the build pairs with the orange one.  From a point ON the orange light that pair is a
    dead end — both children 0, no direct term — whose share the row lacks.  The
    reference says the same, and the lights that can contribute keep p > 0."""
    s = scenes._spheres_07()
    sph = [s[0], Sphere(vec(-6, 3, -2.5), 0.3, material((0, 0, 0), 5.0)), s[1]] + s[3:]
    scene = scenes.Scene(scenes.camera_07(), sph, [scenes._floor()], scenes._pyramid(), [], name="dead_end")
    with cpu(bwrt_lib, scene) as r:
        lights, tree = r.lights(), r.light_tree()
        assert len(lights) == 3 and sorted(leaves_below(tree, 3, int(tree[2]["parent"]))) == [0, 1]
        pts = np.array([[-6, 4, -4, 0, 1, 0], [-5, 3, -4, 1, 0, 0]], np.float32)  # on the orange light (radius 1)
        prims = np.array([0, 0], np.int32)
        got = r.light_pick_probabilities(pts, prims).astype(np.float64)
    p, bound, w, _, _ = ref.probabilities(tree, lights, 3, pts, prims, scene.counts[0])
    mass = ref.no_pick_mass(tree, lights, 3, pts, prims, scene.counts[0])
    assert (np.abs(got - p) <= 2.0 * bound * p).all()
    assert np.array_equal(got == 0, w == 0) and (got[:, :2] == 0).all() and (got[:, 2:] > 0).all()
    assert (mass > 0.001).all() and (np.abs(got.sum(1) + mass - 1.0) <= 2.0 * bound.max(1) + 3 * ref.U).all()


def test_underflow_rule(bwrt_lib):
    """Far points: phi / d2 runs through the float32 denormals to 0.  A light
    with a positive linear weight (in float64) has probability 0 only under
    the written rule — some importance on its way down is at the underflow
    threshold, by the reference alone (least < 2^-125: a float32 denormal or
    0 once its factors are rounded) — and such a row is all 0 or sums to 1
    among the lights that are left, within the denormals' precision.  The
    bound on what is lost comes from the reference alone: the lights it puts at
    the threshold (`at_risk`: w_j > 0 in float64 and some importance on the way
    below 2^-125).  Every lost entry is one of them, so at every point the lost
    lights' share of the linear weight is at most the at-risk lights' share,
    and over the set the lost share of entries is at most the at-risk share
    (measured: 144 lost of 512 entries, 0.281, against 295 at risk, 0.576).
    Points whose d2 overflows give 0 everywhere, as the table walk."""
    lights, tree, _, _, _, nsl, nss = point_set(bwrt_lib, "8")
    pts, prims = far_points(lights, TABLES["8"][0]())
    with renderer(bwrt_lib, "8") as r:
        got = r.light_pick_probabilities(pts, prims).astype(np.float64)
    p, bound, w, _, least = ref.probabilities(tree, lights, nsl, pts, prims, nss)
    lost = (got == 0) & (w > 0)
    assert lost.any() and (got > 0).any()  # the set reaches both sides of the threshold
    assert (least[lost] < 2.0 ** -125).all()
    at_risk = (least < 2.0 ** -125) & (w > 0)
    share, bound_share = lost.sum() / lost.size, at_risk.sum() / at_risk.size
    print(f"underflow: {int(lost.sum())} of {lost.size} entries lost, share {share:.3f}; at risk by the reference alone: "
          f"{int(at_risk.sum())}, share {bound_share:.3f}")
    assert (lost <= at_risk).all()
    assert share <= bound_share < 1.0
    W = w.sum(1)
    lit = W > 0
    assert ((w * lost).sum(1)[lit] / W[lit] <= (w * at_risk).sum(1)[lit] / W[lit]).all()
    sums = got.sum(1)
    safe = (least > 2.0 ** -100).all(1)  # rows far from the threshold: the ordinary rule
    assert safe.any() and (np.abs(sums[safe] - 1.0) <= 2.0 * bound.max(1)[safe] + 8 * ref.U).all()
    assert ((sums == 0) | (np.abs(sums - 1.0) < 0.5)).all()
    with np.errstate(over="ignore"):
        d2_inf = ~np.isfinite((pts[:, :3].astype(np.float32) ** 2).sum(1, dtype=np.float32))
    assert d2_inf.any() and (got[d2_inf] == 0).all()


# ---- same expectation as the default estimator; where the variance stands ---------------

W, H, BATCHES, FRAMES = 80, 48, 32, 128
_TREE = {}


def tree_means(lib, case, make, mb, **kw):
    if case not in _TREE:
        out, whole = [], []
        w, h, frames, batches = kw.get("w", W), kw.get("h", H), kw.get("frames", FRAMES), kw.get("batches", BATCHES)
        rows = kw.get("rows", h)
        from test_light_sampling import LUM
        with cpu(lib, make()) as r:
            r.init_rand(w, h)
            for _ in range(batches):
                _, acc = r.render(w, h, frames, mb, first_frame=1, want_accum=True)
                lum = (acc.astype(np.float64) / frames) @ LUM
                whole.append(lum.mean())
                out.append(lum[:rows].reshape(rows // 8, 8, w // 8, 8).mean((1, 3)).ravel())
        _TREE[case] = (np.array(out), np.array(whole))
    return _TREE[case]


SHARED = {"07/4": (scenes.scene_07, 4), "07/1": (scenes.scene_07, 1), "eight/4": (eight_lights, 4)}
_SIXTY = {}


def all_runs(lib, case):
    """default, uniform NEE, weighted NEE, hierarchy — the first three are
    tests/test_light_picking.py's own runs where it has the case"""
    if case in SHARED:
        make, mb = SHARED[case]
        return (*picking_runs(lib, case), tree_means(lib, case, make, mb))
    if not _SIXTY:
        _SIXTY["runs"] = (block_means(lib, sixty_four_lights(), "uniform", False, 4),
                          block_means(lib, sixty_four_lights(), "uniform", True, 4),
                          block_means(lib, sixty_four_lights(), "weighted", True, 4))
    return (*_SIXTY["runs"], tree_means(lib, case, sixty_four_lights, 4))


CASES = ["07/4", "07/1", "eight/4", "sixty_four/4"]


@pytest.mark.parametrize("case", CASES)
def test_same_expectation(bwrt_lib, case):
    """The hierarchy against the default estimator.  Measured on the CPU backend
    (deterministic): 07 at 4 bounces 34 lit blocks, max |z| 2.10, rms z 0.97,
    frame z -0.24; 07 at 1 bounce 33 lit, 1.74, 0.83, -1.26; the 8-light scene 17
    lit, 3.06, 1.34, -1.11; the 64-light scene 18 lit, 2.42, 1.31, -1.90 (default
    relative standard error there at most 7.6 %)."""
    d, _, _, tree = all_runs(bwrt_lib, case)
    z, zf, lit, ma, sa, sb = z_scores(d, tree)
    print(f"{case}: default relative standard error at most {(sa[lit] / ma[lit]).max():.3f}")
    assert lit.sum() >= 15
    assert_same_expectation(d, tree, case)


def test_buried_light_keeps_the_expectation(bwrt_lib):
    """tests/test_light_picking.py's case: the hidden light takes picks, its
    shadow rays all end on the red sphere.  Measured: 7 lit blocks, max |z|
    0.74, rms z 0.34, frame z -0.57."""
    kw = dict(w=32, h=18, rows=16, batches=16, frames=128)
    a = tree_means(bwrt_lib, "buried0", lambda: hidden_light_scene(0.0), 4, **kw)
    b = tree_means(bwrt_lib, "buried50", lambda: hidden_light_scene(50.0), 4, **kw)
    assert_same_expectation(a, b, "buried light")


def test_non_unit_normals_keep_the_expectation(bwrt_lib):
    """Measured: 7 lit blocks, max |z| 1.23, rms z 0.84, frame z 1.29."""
    kw = dict(w=32, h=18, rows=16, batches=16, frames=512)
    a = block_means(bwrt_lib, small_normal_scene(), "uniform", False, 2, **kw)
    b = tree_means(bwrt_lib, "small_normal", small_normal_scene, 2, **kw)
    z, zf, lit, ma, sa, sb = z_scores(a, b)
    assert lit.sum() >= 2 and (sa[lit] / ma[lit]).max() <= 0.08
    assert_same_expectation(a, b, "small normal")


# measured ratios of the summed squared block standard errors over the default
# estimator's lit blocks (32 batches of 128 frames, 80x48),
# hierarchy over uniform NEE and hierarchy over the table walk.  Pinned at x 1.25,
# the project's margin for 32 batches (a variance estimate from them wobbles by
# about sqrt(2 / 31) = 25 %).  The second ratio is not asserted to be below 1:
# the tree approximates the walk.
VAR_OVER_UNIFORM = {"07/4": 0.692, "07/1": 0.465, "eight/4": 0.180, "sixty_four/4": 0.235}
VAR_OVER_WALK = {"07/4": 1.020, "07/1": 1.152, "eight/4": 1.224, "sixty_four/4": 5.818}


@pytest.mark.parametrize("case", CASES)
def test_variance(bwrt_lib, case):
    d, uni, wgt, tree = all_runs(bwrt_lib, case)
    _, _, lit, _, _, su = z_scores(d, uni)
    _, _, _, _, _, sw = z_scores(d, wgt)
    _, _, _, _, _, st = z_scores(d, tree)
    over_uniform = (st[lit] ** 2).sum() / (su[lit] ** 2).sum()
    over_walk = (st[lit] ** 2).sum() / (sw[lit] ** 2).sum()
    print(f"variance ratio {case}: hierarchy / uniform NEE {over_uniform:.4f}, hierarchy / table walk {over_walk:.4f}")
    if case in ("eight/4", "sixty_four/4"):
        assert over_uniform < 1.0
    assert over_uniform <= 1.25 * VAR_OVER_UNIFORM[case]
    assert over_walk <= 1.25 * VAR_OVER_WALK[case]


# ---- composition -----------------------------------------------------------------------

@pytest.mark.parametrize("make,shapes", [(scenes.scene_07, "spheres"), (mixed, "all")])
def test_row_shards_equal_the_full_frame(bwrt_lib, make, shapes):
    with cpu(bwrt_lib, make(), shapes=shapes) as r:
        full = state(r, W0, H0, 3, 4, calls=2)
    for off in (0, 1):
        with cpu(bwrt_lib, make(), shapes=shapes) as r:
            part = state(r, W0, H0, 3, 4, calls=2, row_offset=off, row_stride=2)
        for f, p in zip(full, part):
            assert np.array_equal(f[:, off::2] if f.shape[0] == 6 else f[off::2], p, equal_nan=True)


def tree_snapshots(lib, name, w, h, bounces, upto):
    have = {}
    with cpu(lib, scenes.SCENES[name]()) as u:
        for f in range(1, upto + 1):
            img = u.render(w, h, 1, bounces, first_frame=1 if f == 1 else 0)
            rng, acc = u.get_state(h, w)
            have[f] = (img, rng, acc)
    return have


@pytest.mark.parametrize("name,w,h,bounces", [("07", 67, 45, 4), ("stress", 48, 27, 4)])
def test_adaptive_replays_uniform_calls(bwrt_lib, name, w, h, bounces):
    """Every pixel after the adaptive calls holds the frameSum, RNG state and
    RGBA of a hierarchy uniform-call render stopped at its own frame count."""
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_light_sampling(True)
        r.set_light_picking("weighted")
        r.set_light_hierarchy(True)
        res = adaptive_sequence(r, scenes.SCENES[name](), w, h, bounces)
    assert len(np.unique(res["n"])) > 1
    check_replay(res, tree_snapshots(bwrt_lib, name, w, h, bounces, int(res["n"].max())))
    with Renderer.cpu(0, lib=bwrt_lib) as r:  # and the table walk's sequence is another one
        r.set_light_sampling(True)
        r.set_light_picking("weighted")
        walk = adaptive_sequence(r, scenes.SCENES[name](), w, h, bounces)
    assert not np.array_equal(walk["accum"], res["accum"], equal_nan=True)


def test_downstream_passes_run_on_hierarchy_frames(bwrt_lib):
    w, h = 64, 36
    with cpu(bwrt_lib, scenes.scene_07()) as r:
        r.set_moments(True)
        for i in range(3):
            r.render(w, h, 4, 4, first_frame=1 if i == 0 else 0)
        assert r.moments_batches == 3
        var = r.variance(h, w)
        assert np.isfinite(var).all() and (var > 0).any()
        img, col = r.denoise_var(w, h, want_color=True)
        assert img.shape == (h, w, 4) and np.isfinite(col).all()
        block, frames, batches = r.export_shard(h, w, planes=5)
        assert block.shape == (5, h, w) and (frames, batches) == (12, 3)
        assert np.array_equal(block[:3].transpose(1, 2, 0), r.get_state(h, w)[1])


def test_cli_flag_matches_python(bwrt_lib, tmp_path):
    def run(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)

    assert "--light-hierarchy" in run("--help").stdout
    for args in (("--light-hierarchy",), ("--light-sampling", "--light-hierarchy"),
                 ("--light-sampling", "--light-picking", "uniform", "--light-hierarchy"),
                 ("--light-picking", "weighted", "--light-hierarchy")):
        r = run(*args)
        assert r.returncode == 2, args
        assert "--light-picking weighted" in r.stderr or "--light-sampling" in r.stderr, args
    r = run("--light-sampling", "--light-hierarchy")
    assert "--light-picking weighted" in r.stderr
    w, h = 64, 36
    common = ("--cpu", "2", "--scene", "07", "--width", str(w), "--height", str(h), "--frames", "3", "--max-bounces", "4",
              "--light-sampling", "--light-picking", "weighted")
    imgs = {}
    for tree in (False, True):
        out = tmp_path / f"{tree}.ppm"
        r = run(*common, *(("--light-hierarchy",) if tree else ()), "--out", str(out))
        assert r.returncode == 0, r.stderr
        imgs[tree] = read_ppm(out)
        with cpu(bwrt_lib, scenes.scene_07(), hierarchy=tree, threads=2) as p:
            img = None
            for f in range(3):  # the CLI renders --frames-per-call 1
                img = p.render(w, h, 1, 4, first_frame=1 if f == 0 else 0)
        assert np.array_equal(imgs[tree], img[..., :3]), tree
    assert not np.array_equal(imgs[False], imgs[True])
