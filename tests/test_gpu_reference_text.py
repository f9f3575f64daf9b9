"""The HIP render against the reference's own source text built for the CPU,
with no restatement in between (tests/test_reference_text.py pins the oracle
and the CPU fallback to the same library; this is the short direct check).

The library (oracle/_ref/libreftext.so, recipe in oracle/ref/) is built where
the reference tree is and travels with the tree; this module never reads the
reference tree.  RNG states and RGBA8 bit for bit, frameSum value for value
with NaN equal to NaN.  Without the library: a failure where the reference
tree is present (a broken build), a skip where neither is.
"""
import os

import pytest

from bwrt import scenes
from reference_text_cases import (CASES, GPU_CASES, assert_same, nonfinite_pixels, reference_state,
                                  require_library, run_product)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _library():
    require_library()


@pytest.mark.parametrize("name", GPU_CASES)
def test_gpu_equals_reference_text(gpu, monkeypatch, name):
    try:
        img, rng, acc = run_product(gpu, CASES[name], monkeypatch)
        kernel = gpu.last_kernel_name()
    finally:
        gpu.set_scene(scenes.scene_07())  # the shared renderer goes back to its usual scene
    assert_same(img, rng, acc, reference_state(name), "HIP render")
    if name.startswith("guard"):
        assert nonfinite_pixels(acc) == 0
    if name == "stress" and not os.environ.get("BWRT_LIB"):
        assert kernel.startswith("rt_render_bvh_refill_kernel<"), kernel
