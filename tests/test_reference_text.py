"""The oracle and the product's CPU fallback against the reference's own
source text built for the CPU — CPU only.

oracle/oracle.c is a hand restatement of the reference; every bit-exact test
of the HIP kernels rests on it.  oracle/_ref/libreftext.so is the reference's
Main.cu and headers themselves, compiled by the recipe in oracle/ref/ over
stand-in CUDA / GLFW headers (DESIGN.md section 2 lists their assumptions:
fminf / fmaxf for the float min / max, the project's sinf / cosf / atanf
sequence and its XORWOW restatement behind the device calls).  Here:

  - the oracle equals the library on every case of reference_text_cases.CASES;
  - so does the CPU fallback (csrc/rt_cpu.cpp over csrc/rt_path.h, the
    arithmetic the HIP kernels share);
  - rt_apply_controls equals the reference's controls() for all 1,024 key
    masks at three frame times from a turned camera;
  - every oracle mutant (oracle.c ORC_MUTANT 1-10: one reference quirk each
    replaced by its "natural" formula) DIFFERS from the library on a named
    case on which the unmutated oracle does not: the comparison can see each
    quirk;
  - the isnan(g) guard scene (scenegen.guard_scene) stays finite everywhere.

RNG states and RGBA8 are compared bit for bit, frameSum value for value with
NaN equal to NaN.  Without the library the tests fail when the reference tree
is present (a broken build) and skip when it is absent too.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reftext as R
from bwrt import abi
from reference_text_cases import (CASES, MUTANT_CASE, assert_same, differing, nonfinite_pixels, reference_state,
                                  require_library, run_product, run_state)


@pytest.fixture(scope="module", autouse=True)
def _library():
    require_library()


@pytest.fixture(scope="module")
def cpu(bwrt_lib):
    from bwrt import Renderer
    r = Renderer.cpu(0, lib=bwrt_lib)
    yield r
    r.close()


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_reference_text(oracle, name):
    st = run_state(oracle.render, CASES[name])
    assert_same(st.rgba, st.rng, st.accum, reference_state(name), "oracle")


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_fallback_equals_reference_text(cpu, monkeypatch, name):
    img, rng, acc = run_product(cpu, CASES[name], monkeypatch)
    assert_same(img, rng, acc, reference_state(name), "CPU fallback")


def test_cases_are_live():
    """The matrix holds what it claims: non-finite pixels where the scales
    overflow (the cases that separate value from bit comparison and feed
    mutant 8), a reset that really restarts, a shard that is one."""
    assert nonfinite_pixels(reference_state("random5_x1e+10").accum) > 100
    assert nonfinite_pixels(reference_state("07_320x180_split").accum) == 0
    assert reference_state("07_1080p_rows").rgba.shape == (8, 1920, 4)
    assert reference_state("07_shard_1_of_3").rgba.shape == (12, 100, 4)
    assert reference_state("07_continue_reset").frame == 4  # 2 frames after the reset, then 1 more


# ---- the isnan(g) guard (Main.cu:139) -----------------------------------------

@pytest.mark.parametrize("name", ["guard_1e20", "guard_inf", "guard_07_1e20"])
def test_guard_scene_is_finite(oracle, cpu, monkeypatch, name):
    """Reference text, oracle and CPU fallback agree (the tests above) and no
    pixel is non-finite: the guard turned every NaN geometry term into 1."""
    assert nonfinite_pixels(reference_state(name).accum) == 0
    assert nonfinite_pixels(run_state(oracle.render, CASES[name]).accum) == 0
    assert nonfinite_pixels(run_product(cpu, CASES[name], monkeypatch)[2]) == 0


# ---- sensitivity: every oracle mutant is rejected --------------------------------

_MUT_FLAGS = ["-O2", "-std=c11", "-fPIC", "-fopenmp", "-fno-fast-math", "-w", "-shared"]


def _host_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma " in line + " " for line in f)
    except OSError:
        return False


def _build_mutant(k):
    out = os.path.join(R.HERE, "_mut", f"liboracle_m{k}.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    flags = _MUT_FLAGS + (["-ffp-contract=fast", "-march=x86-64-v3"] if k == 10 else
                          ["-ffp-contract=off", f"-DORC_MUTANT={k}"])
    subprocess.run(["gcc", *flags, "-o", out, os.path.join(R.HERE, "oracle.c"), "-lm"], check=True)
    return out


@pytest.mark.parametrize("k", sorted(MUTANT_CASE))
def test_mutant_differs_from_reference_text(oracle, k):
    if k == 10 and not _host_has_fma():
        pytest.skip("mutant 10 is FMA contraction: this host has no FMA unit to run it on")
    name = MUTANT_CASE[k]
    ref = reference_state(name)
    st = run_state(oracle.render, CASES[name])
    assert differing(st.rgba, st.rng, st.accum, ref) == {"rng": 0, "rgba": 0, "frameSum": 0}
    try:
        oracle.use_library(_build_mutant(k))
        mut = run_state(oracle.render, CASES[name])
    finally:
        oracle.use_library(oracle.LIB_PATH)
    d = differing(mut.rgba, mut.rng, mut.accum, ref)
    print(f"mutant {k} on {name}: {d}")
    assert d["frameSum"] > 0 or d["rgba"] > 0, f"mutant {k} is not told from the reference text on {name}"
    if k == 6:  # the guard's absence shows as NaN pixels, thousands of them
        assert nonfinite_pixels(mut.accum) > 1000 and nonfinite_pixels(ref.accum) == 0


# ---- controls() --------------------------------------------------------------------

def test_controls_equal_reference_controls(bwrt_lib):
    """rt_apply_controls against the reference's controls() (Controls.cuh),
    bit for bit: every combination of the ten movement keys, with and without
    escape on one of them, at three frame times, from a turned camera."""
    start = (abi.Vec3(1.25, 0.75, -3.5), (0.7, -0.4), 1.3)
    checked = 0
    for dt in (1 / 60, 1 / 144, 0.25):
        for keys in list(range(1024)) + [1 << 10, (1 << 10) | 0x155]:
            cams = [abi.Camera(abi.Vec3(start[0].x, start[0].y, start[0].z), (C.c_float * 2)(*start[1]), start[2])
                    for _ in range(2)]
            got = bwrt_lib.rt_apply_controls(C.byref(cams[0]), keys, dt)
            want = R.controls(cams[1], keys, dt)
            assert got == want, (keys, dt)
            assert bytes(cams[0]) == bytes(cams[1]), (keys, dt)
            checked += 1
    assert checked == 3 * 1026
