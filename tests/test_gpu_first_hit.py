"""The first-hit guide kernel (rt_aov_kernel, both instantiations) and its
cached twin (ensure_guides) on the MI355X, pinned to the oracle: the matrix of
tests/first_hit_cases.py directly against oracle.first_hit, bit for bit
(np.array_equal, equal_nan=True; no tolerance anywhere in this file), and
what only the kernel has — frames whose last wave and block are partial, each
output pointer alone, a reference-fast context, the guides the filters cache,
and repeated calls.  tests/test_first_hit.py has the same matrix on the CPU
backend and the float64 pin of the oracle entry.
"""
import numpy as np
import pytest

import first_hit_cases as F
from bwrt import Renderer, scenes

pytestmark = pytest.mark.gpu


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- the matrix and the partial waves / blocks, against the oracle -----------------
@pytest.mark.parametrize("case", F.CASES + F.SHAPE_CASES, ids=repr)
def test_guides_equal_oracle(gpu, oracle, monkeypatch, capfd, case):
    got, ref, scene = F.check_case(gpu, oracle, case, monkeypatch, capfd)
    if case.stride > 1:  # the shard's rows are the same rows of the full frame
        whole = F.Case(case.name + "-whole", lambda: scene, case.w, case.h, case.env)
        full, _ = F.run_case(gpu, whole, monkeypatch, capfd)
        for k in F.KEYS:
            assert same(got[k], full[k][case.off::case.stride]), k
    F.report(case, ref, scene)


@pytest.mark.parametrize("path", ["brute", "bvh"])
def test_ties_go_to_the_later_primitive(gpu, oracle, monkeypatch, capfd, path):
    scene, copies = F.tie_scene()
    case = F.Case(f"ties-{path}", lambda: scene, 64, 36, F.PATHS[path])
    got, _, _ = F.check_case(gpu, oracle, case, monkeypatch, capfd)
    hit = got["prim"] >= 0
    assert hit.mean() >= 0.9
    assert set(np.unique(got["prim"][hit]).tolist()) <= copies
    assert np.all(got["albedo"][hit][:, 0] == np.float32(0.75))  # the copies' red; the originals' is 0.25


# ---- each output pointer alone (the other three NULL) --------------------------------
@pytest.mark.parametrize("name", ["07-brute", "stress-bvh"])
def test_each_output_alone(gpu, oracle, monkeypatch, capfd, name):
    case = F.BY_NAME[name]
    every, _, _ = F.check_case(gpu, oracle, case, monkeypatch, capfd)  # leaves the case's scene set
    for k in F.KEYS:
        one = gpu.render_aov(case.w, case.h, only=k)
        assert list(one) == [k] and same(one[k], every[k]), k


# ---- a reference-fast context: the guides stay exact ----------------------------------
@pytest.mark.parametrize("name", ["stress-bvh", "07-bvh"])
def test_reference_fast_context_keeps_exact_guides(bwrt_lib, oracle, monkeypatch, capfd, name):
    with Renderer(0, lib=bwrt_lib) as r:
        r.set_precision("fast")
        F.check_case(r, oracle, F.BY_NAME[name], monkeypatch, capfd)
        assert r.precision == "fast"


# ---- the guides the filters cache (ensure_guides) on the BVH path ----------------------
def test_cached_guides_follow_the_view(bwrt_lib, monkeypatch):
    """denoise(iterations=1) reads the cached guides: after a render, after a
    camera change (the cache must be recomputed) and on a context that never
    called render_aov, each time the bits of a CPU context in the same state
    (whose guides tests/test_first_hit.py pins to the oracle)."""
    scene = scenes.scene_07()
    w, h = 64, 36
    cam = F.moved_camera(scene)
    monkeypatch.setenv("BWRT_BVH_MIN", "1")  # read at set_scene

    def cpu_result(state, frame, camera):
        with Renderer.cpu(0, lib=bwrt_lib) as c:
            c.set_scene(scene)
            if camera is not None:
                c.set_camera(camera)
            c.init_rand(w, h)
            c.set_state(*state, frame)
            return c.denoise(w, h, iterations=1, want_color=True)

    def equal(got, ref):
        return np.array_equal(got[0], ref[0]) and same(got[1], ref[1])

    with Renderer(0, lib=bwrt_lib) as r:
        r.set_scene(scene)
        r.render(w, h, 2, 4, first_frame=1)
        r.render_aov(w, h)
        first = r.denoise(w, h, iterations=1, want_color=True)
        state1 = r.get_state(h, w)
        want1 = cpu_result(state1, 3, None)
        assert equal(first, want1)
        r.set_camera(cam)
        assert r.frame_counter == 1
        r.render(w, h, 2, 4)
        second = r.denoise(w, h, iterations=1, want_color=True)
        state2 = r.get_state(h, w)
        want2 = cpu_result(state2, 3, cam)
        assert equal(second, want2)
        # with the first view's guides the second frame filters differently: the check above can tell
        assert not equal(want2, cpu_result(state2, 3, None))
    with Renderer(0, lib=bwrt_lib) as fresh:  # never calls render_aov
        fresh.set_scene(scene)
        fresh.set_camera(cam)
        fresh.init_rand(w, h)
        fresh.set_state(*state2, 3)
        assert equal(fresh.denoise(w, h, iterations=1, want_color=True), want2)


# ---- repeats --------------------------------------------------------------------------
def test_repeated_bvh_calls_are_identical(gpu, oracle, monkeypatch, capfd):
    case = F.BY_NAME["stress-bvh"]
    first, _, _ = F.check_case(gpu, oracle, case, monkeypatch, capfd)
    for _ in range(2):
        again = gpu.render_aov(case.w, case.h)
        for k in F.KEYS:
            assert same(again[k], first[k]), k
