"""The first-hit guide buffers (rt_render_aov: prim, depth, normal, albedo)
pinned to the oracle on every hit path, on the CPU backend — no GPU needed
(tests/test_gpu_first_hit.py runs the same matrix on the HIP kernels).

The plain reference is oracle.first_hit: the oracle's own camera prelude and
closest-hit loop (the ones its renders use, Main.cu:214-234 / 287-290) on the
un-jittered primary ray.  Hit point o + t*d, sphere normal normalize(P - c),
plane / polygon normal cross(e0, e1) normalised once: the same float
operations on both sides, so every comparison is bit for bit
(np.array_equal, equal_nan=True).  The one tolerance in this file is the
float64 pin of the new oracle entry itself (1e-4, as test_denoise.py's).

The matrix is tests/first_hit_cases.py.  Of its six listed extreme scales,
random11 x 1e15 and random13 x 1e19 give NaN depths (all 576 pixels each) and
none gives an inf depth on a hit, so two scales were added that do:
random7 x 3e12 (498 inf and 68 NaN depths, a triangle) and random15 x 4e12
(458 inf depths, a quad).
"""
import numpy as np
import pytest

import denoise_ref as R
import first_hit_cases as F
from bwrt import Renderer
from test_denoise import feature_scene


@pytest.fixture(scope="module")
def cpu(bwrt_lib):
    r = Renderer.cpu(0, lib=bwrt_lib)
    yield r
    r.close()


# ---- the new oracle entry against float64 (no product involved) ------------------
def test_oracle_first_hit_against_float64(oracle):
    scene = feature_scene()
    w, h = 64, 36
    a = oracle.first_hit(scene, w, h)
    prim, depth, normal = R.first_hit(scene, w, h)
    ambiguous = np.zeros((h, w), bool)
    for dx, dy in ((0.05, 0.05), (-0.05, 0.05), (0.05, -0.05), (-0.05, -0.05)):
        ambiguous |= R.first_hit(scene, w, h, dx=dx, dy=dy)[0] != prim
    assert ambiguous.mean() <= 0.05
    assert len(np.unique(prim[~ambiguous])) == 5  # three spheres, the plane, the sky
    ok = ~ambiguous
    assert np.array_equal(a["prim"][ok], prim[ok])
    hit, miss = ok & (prim >= 0), ok & (prim < 0)
    assert np.all(a["depth"][miss] == np.inf) and not a["normal"][miss].any() and not a["albedo"][miss].any()
    assert np.max(np.abs(a["depth"][hit] - depth[hit]) / depth[hit]) <= 1e-4
    assert np.max(np.abs(a["normal"][hit] - normal[hit])) <= 1e-4
    albedo = np.array([[0.9, 0.2, 0.1], [0.1, 0.8, 0.3], [0.2, 0.3, 0.9], [0.5, 0.5, 0.5]], np.float32)
    assert np.array_equal(a["albedo"][hit], albedo[prim[hit]])
    # the oracle's own record: kind / index behind prim, P = o + t d, the plane's raw normal
    sph = ok & (prim >= 0) & (prim < 3)
    assert np.all(a["kind"][sph] == oracle.KIND_SPHERE) and np.array_equal(a["index"][sph], prim[sph])
    pl = ok & (prim == 3)
    assert np.all(a["kind"][pl] == oracle.KIND_PLANE) and np.all(a["index"][pl] == 0)
    assert np.all(a["kind"][miss] == oracle.KIND_MISS) and np.all(a["index"][miss] == -1)
    assert np.all(a["raw_normal"][pl] == np.float32([0.0, 3.0, 0.0]))  # cross((0,0,2), (1.5,0,0))
    assert np.array_equal(a["raw_normal"][sph], a["normal"][sph])
    P = R.hit_points(scene.camera, w, h, depth, prim)
    assert np.max(np.abs(a["point"][hit] - P[hit])) <= 1e-4 * np.max(np.abs(P[hit]))


def test_oracle_first_hit_shard_and_background(oracle):
    scene = F.BY_NAME["07-brute"].make()
    full = oracle.first_hit(scene, 67, 45, background=(0.25, 0.5, 1.0))
    part = oracle.first_hit(scene, 67, 45, 5, 8, background=(0.25, 0.5, 1.0))
    for k in full:
        assert np.array_equal(part[k], full[k][5::8], equal_nan=True), k
    miss = full["prim"] < 0
    assert miss.any() and np.all(full["albedo"][miss] == np.float32([0.25, 0.5, 1.0]))
    with pytest.raises(ValueError):
        oracle.first_hit(scene, 0, 45)


# ---- the CPU backend against the oracle, bit for bit ------------------------------
@pytest.mark.parametrize("case", F.CASES + F.SHAPE_CASES, ids=repr)
def test_guides_equal_oracle(cpu, oracle, monkeypatch, capfd, case):
    got, ref, scene = F.check_case(cpu, oracle, case, monkeypatch, capfd)
    if case.stride > 1:  # the shard's rows are the same rows of the full frame
        whole = F.Case(case.name + "-whole", lambda: scene, case.w, case.h, case.env)
        full, _ = F.run_case(cpu, whole, monkeypatch, capfd)
        for k in F.KEYS:
            assert np.array_equal(got[k], full[k][case.off::case.stride], equal_nan=True), k
    F.report(case, ref, scene)


def test_matrix_coverage(oracle):
    """Conditions on the inputs, checked on the oracle alone (the cases with a
    view of their own, which need a renderer's camera, are not needed for
    them): all four kinds of primitive and the miss are first hits somewhere
    in the matrix, the extreme scales give NaN and inf depths, and there are
    BVH cases whose every ray fails bvh_safe (the fall-back to the brute-force
    loop inside the walk), ones whose every ray takes the walk, and ones where
    only some do (lanes of one wave part ways)."""
    seen = {}
    for case in F.CASES:
        if not case.view:
            scene = case.make()
            ref = F.want(oracle, case, scene)
            seen[case.name] = (set(np.unique(ref["kind"]).tolist()),) + F.report(case, ref, scene)
    kinds = set().union(*(s[0] for s in seen.values()))
    assert kinds == {oracle.KIND_MISS, oracle.KIND_SPHERE, oracle.KIND_PLANE, oracle.KIND_TRIANGLE, oracle.KIND_QUAD}
    extreme = [c.name for c in F.CASES if c.extreme]
    assert any(seen[n][1] > 0 for n in extreme), "no NaN depth at the extreme scales"
    assert any(seen[n][2] > 0 for n in extreme), "no inf depth at the extreme scales"
    bvh = [c for c in F.CASES if c.bvh and not c.view]
    assert any(seen[c.name][3] == c.w * len(range(c.off, c.h, c.stride)) for c in bvh), "no all-fall-back case"
    assert any(seen[c.name][3] == 0 for c in bvh)
    assert any(0 < seen[c.name][3] < c.w * c.h for c in bvh if c.stride == 1), "no frame with a mixed fall-back"


# ---- exact distance ties: the primitive tested later wins --------------------------
@pytest.mark.parametrize("path", ["brute", "bvh"])
def test_ties_go_to_the_later_primitive(cpu, oracle, monkeypatch, capfd, path):
    scene, copies = F.tie_scene()
    case = F.Case(f"ties-{path}", lambda: scene, 64, 36, F.PATHS[path])
    got, ref, _ = F.check_case(cpu, oracle, case, monkeypatch, capfd)
    hit = got["prim"] >= 0
    assert hit.mean() >= 0.9
    # against the rule, not only against the oracle: every hit is a second copy ...
    seen = set(np.unique(got["prim"][hit]).tolist())
    assert seen <= copies, sorted(seen - copies)
    # ... of every kind, with the copy's albedo (red 0.75; the originals' is 0.25)
    assert set(np.unique(ref["kind"][hit]).tolist()) == {0, 1, 2, 3}
    assert np.all(got["albedo"][hit][:, 0] == np.float32(0.75))
    # the pyramid's shared edges: more than one of its faces is seen
    nt = scene.counts[2] // 2
    assert len(seen & set(range(4 + nt + 1, 4 + 2 * nt))) >= 2
