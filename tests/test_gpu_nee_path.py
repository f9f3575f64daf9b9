"""The next-event-estimation kernels on the MI355X against the replay driver
(tests/nee_path_ref.py; the cases and the driver's results are those of
tests/test_nee_path.py, computed once per case and shared): frameSum, RNG state
and RGBA bit for bit, and the kernel's name per case, so that both placements
of the shadow ray in csrc/rt_kernel_lane.h are really taken —

* inline (brute force): the whole case matrix;
* deferred by one loop iteration (BVH): the small-light scene over 64 spheres,
  and scene 07 and the mixed scene with BWRT_BVH_MIN=1;
* 64-lane groups (max_bounces 12: the record stack of 256 lanes passes 48 KB);
* the list form: one adaptive call, whose pixels hold the driver's bits for
  their own frame counts.

No kernel text is mutated here; the sensitivity of the comparison is that of
the driver, measured on the CPU twin (tools/nee_path_sensitivity.py).
"""
import pytest

import nee_ref as R
import test_nee_path as T
from bwrt import Renderer

pytestmark = pytest.mark.gpu

BVH_BY_SIZE = {"small_light64"}


def kernel_name(c, bvh, block=256, listed=False):
    """what rt_last_kernel_name reports for case c (csrc/rt_kernel_nee.h)"""
    t, _ = R.table_from_words(T.table_of(c.scene))
    polygons = c.shapes == 1 and len(t["prim"]) > t["n_sphere_lights"]
    return "rt_render_nee_kernel<%d%s%s%s%s>" % (block, ",hit_global,bvh" if bvh else "", ",list" if listed else "",
                                                 ",weighted" if c.pick else "", ",polygons" if polygons else "")


def gpu_against_driver(lib, c, bvh, block=256):
    want = T.driver_result(c)
    with Renderer(0, lib=lib) as g:
        got = T.product_state(g, c)
        name = g.last_kernel_name()
    T.assert_equals_driver(got, want, T.case_id(c))
    if c.mb == 0:  # no level can act: the default launch policy's kernel
        assert not name.startswith("rt_render_nee_kernel"), name
    else:
        assert name == kernel_name(c, bvh, block), name


@pytest.mark.parametrize("c", T.CASES, ids=T.IDS)
def test_kernel_equals_the_driver(bwrt_lib, c):
    gpu_against_driver(bwrt_lib, c, c.scene in BVH_BY_SIZE)


@pytest.mark.parametrize("c", T.FORCED_BVH, ids=[T.case_id(c) for c in T.FORCED_BVH])
def test_deferred_shadow_ray_equals_the_driver(bwrt_lib, monkeypatch, c):
    """the same driver results through the BVH kernels (the scene's geometry does not change)"""
    assert c in T.CASES
    monkeypatch.setenv("BWRT_BVH_MIN", "1")
    gpu_against_driver(bwrt_lib, c, True)


@pytest.mark.parametrize("c", T.DEEP, ids=[T.case_id(c) for c in T.DEEP])
def test_small_groups_equal_the_driver(bwrt_lib, c):
    gpu_against_driver(bwrt_lib, c, False, block=64)


def test_list_form_replays_the_driver(bwrt_lib):
    """One adaptive call under NEE on 07 at 67 x 45 (4 uniform frames, then 2 more
    on the selected pixels): every pixel holds the driver's frameSum, RNG state
    and RGBA after its own number of frames."""
    with Renderer(0, lib=bwrt_lib) as g:
        res = T.adaptive_call(g, T.LISTED)
        assert g.last_kernel_name() == kernel_name(T.LISTED, False, listed=True)
    T.assert_replays_the_driver(res, T.LISTED, (4, 6))
