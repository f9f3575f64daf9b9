"""Cases and runners shared by tests/test_reference_text.py (CPU) and
tests/test_gpu_reference_text.py (GPU): renders compared with the reference's
own source text built for the CPU (oracle/_ref/libreftext.so through
oracle/reftext.py; recipe in oracle/ref/).

A case is a scene, a frame shape (with an optional row shard), a bounce limit
and a list of render calls (passes, first_frame); first_frame None continues,
1 restarts the accumulation (Main.cu:301).  Every backend (the library, the
oracle, the product's CPU fallback, the HIP renderer) runs the same calls; the
library's result is computed once per case and shared.

Comparison rule: RNG states and RGBA8 bit for bit; frameSum value for value
with NaN equal to NaN (the sign and payload of a NaN are not defined by the
reference's text, and do differ between compilers).
"""
import dataclasses

import numpy as np
import pytest

import oracle as O
import reftext as R
from bwrt import scenes
from scenegen import _random_scene, _scaled, guard_scene, guard_scene_inf


def require_library():
    """Skip only when there is nothing to pin against; a reference tree
    without the library built from it is a broken build, not a skip."""
    if R.available():
        return
    if R.reference_present():
        pytest.fail("the reference tree is present but oracle/_ref/libreftext.so is missing: "
                    "__graft_entry__.build() has not run oracle/ref's recipe")
    pytest.skip("no oracle/_ref/libreftext.so and no reference tree to build it from: "
                "the reference-text pin cannot run here")


@dataclasses.dataclass
class Case:
    scene: object              # a zero-argument callable giving a fresh Scene
    w: int
    h: int
    mb: int
    calls: tuple = ((2, 1),)   # (passes, first_frame or None)
    off: int = 0
    stride: int = 1
    background: tuple = (0.0, 0.0, 0.0)
    spp: int = 1               # samplesPerPixel, the in-frame loop
    bvh: bool = False          # product only: force the BVH (BWRT_BVH_MIN=1 at set_scene)


def _random_case(seed):
    """tests/test_gpu_parity.py test_random_scenes' scale and bounce pattern."""
    def make():
        s = _random_scene(seed)
        if seed % 4 == 2:
            s = _scaled(s, 1e3 if seed % 8 == 2 else 1e-3)
        return s
    return Case(make, 80, 45, [0, 1, 2, 4, 6, 9][seed % 6], ((3, 1),), bvh=bool(seed % 2))


def _stress(k):
    return (lambda: scenes.stress_scene()) if k == 1.0 else (lambda: _scaled(scenes.stress_scene(), k))


CASES = {
    "07_320x180_split": Case(scenes.scene_07, 320, 180, 4, ((3, 1), (1, None))),
    "04": Case(scenes.scene_04, 320, 180, 3, ((4, 1),)),
    "04_box": Case(scenes.scene_04_box, 320, 180, 5, ((4, 1),)),
    "01_256": Case(scenes.scene_01, 256, 256, 1, ((1, 1),)),
    "07_background_spp3": Case(scenes.scene_07, 96, 54, 4, ((2, 1), (1, None)), background=(0.25, 0.5, 1.0), spp=3),
    **{f"07_bounces{mb}": Case(scenes.scene_07, 80, 45, mb) for mb in (0, 1, 12, 32)},
    **{f"07_{w}x{h}": Case(scenes.scene_07, w, h, 4, ((3, 1),)) for w, h in ((100, 37), (1, 1), (63, 65))},
    "07_1080p_rows": Case(scenes.scene_07, 1920, 1080, 4, ((2, 1),), off=3, stride=135),
    "07_shard_1_of_3": Case(scenes.scene_07, 100, 37, 6, ((3, 1), (2, None)), off=1, stride=3),
    # progressive continuation, then a reset: accumulatedFrames == 1 again
    # restarts frameSum while the RNG streams go on (Controls.cuh:15)
    "07_continue_reset": Case(scenes.scene_07, 128, 72, 4, ((3, 1), (5, None), (2, 1), (1, None))),
    "stress": Case(_stress(1.0), 96, 54, 8, bvh=True),
    **{f"stress_x{k:g}": Case(_stress(k), 96, 54, mb, bvh=True)
       for k, mb in ((3e4, 6), (1e-4, 6), (100.0, 1), (1e3, 6), (1e10, 3))},
    **{f"random{seed}": _random_case(seed) for seed in range(40)},
    **{f"random{seed}_x{k:g}": Case(lambda seed=seed, k=k: _scaled(_random_scene(seed), k), 64, 36, 4, bvh=bool(seed % 4 == 1))
       for seed, k in ((3, 1e6), (5, 1e10), (7, 1e-6), (9, 1e-10), (11, 1e15), (13, 1e19))},
    "guard_1e20": Case(guard_scene, 160, 90, 4, ((3, 1),)),
    "guard_inf": Case(guard_scene_inf, 160, 90, 4, ((3, 1),)),
    "guard_07_1e20": Case(lambda: guard_scene(1e20, scenes.scene_07), 160, 90, 4, ((3, 1),)),
}

# the short direct GPU check (tests/test_gpu_reference_text.py)
GPU_CASES = ("07_320x180_split", "04_box", "stress", "random2", "random5", "random18",
             "07_background_spp3", "guard_1e20")


# mutant -> the case on which it must differ from the library
MUTANT_CASE = {
    1: "07_320x180_split",   # A.5 jitter scale: W / 1000 is 0 below 1000 pixels, W / 1000.0 is not
    2: "07_320x180_split",   # A.6 half-pixel offset
    3: "07_320x180_split",   # A.9 unit polygon normals (the pyramid)
    4: "07_320x180_split",   # A.10 tangent frame
    5: "07_320x180_split",   # A.11 tan^2 for tan^4
    6: "guard_1e20",         # A.11 no isnan(g) guard: only a scene that makes g NaN can tell
    7: "07_320x180_split",   # A.12 forward fold
    8: "random5_x1e+10",     # A.14/15 std::min / std::max: only non-finite pixels can tell
    9: "07_320x180_split",   # libm transcendentals
    10: "07_320x180_split",  # FMA contraction (built for an FMA target)
}


def run_state(render, case):
    """Run the case's calls through `render` (oracle.render or reftext.render)."""
    scene = case.scene()
    st = O.OracleState(case.w, case.h, case.off, case.stride)
    for passes, first in case.calls:
        render(scene, st, passes, case.mb, first_frame=first, background=case.background,
               samples_per_pixel=case.spp)
    return st


_reference = {}


def reference_state(name):
    """The library's result for CASES[name]: computed once, shared, read-only."""
    if name not in _reference:
        st = run_state(R.render, CASES[name])
        for a in (st.rng, st.accum, st.rgba):
            a.setflags(write=False)
        _reference[name] = st
    return _reference[name]


def run_product(r, case, monkeypatch):
    """The same calls on a bwrt Renderer (CPU fallback or GPU).  Returns
    (rgba, rng, accum) of the shard."""
    if case.bvh:
        monkeypatch.setenv("BWRT_BVH_MIN", "1")
    try:
        r.set_scene(case.scene())
    finally:
        monkeypatch.delenv("BWRT_BVH_MIN", raising=False)
    r.set_background(*case.background)
    r.set_samples_per_pixel(case.spp)
    try:
        r.init_rand(case.w, case.h, case.off, case.stride)
        for passes, first in case.calls:
            kw = {} if first is None else {"first_frame": first}
            img = r.render(case.w, case.h, passes, case.mb, row_offset=case.off, row_stride=case.stride, **kw)
        rng, acc = r.get_state(len(range(case.off, case.h, case.stride)), case.w)
    finally:
        r.set_background(0.0, 0.0, 0.0)
        r.set_samples_per_pixel(1)
    return img, rng, acc


def differing(got_rgba, got_rng, got_acc, ref):
    """Pixels that differ from the library's state `ref`, per output."""
    acc_same = (got_acc == ref.accum) | (np.isnan(got_acc) & np.isnan(ref.accum))
    return {"rng": int((got_rng != ref.rng).any(0).sum()), "rgba": int((got_rgba != ref.rgba).any(-1).sum()),
            "frameSum": int((~acc_same).any(-1).sum())}


def assert_same(got_rgba, got_rng, got_acc, ref, what):
    d = differing(got_rgba, got_rng, got_acc, ref)
    assert d == {"rng": 0, "rgba": 0, "frameSum": 0}, f"{what}: pixels differing from the reference text: {d}"


def nonfinite_pixels(accum):
    return int((~np.isfinite(accum)).any(-1).sum())
