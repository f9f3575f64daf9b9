"""The precision mode's interface off the GPU: rt_set_precision /
rt_get_precision on a CPU context (EXACT only: the CPU fallback exists to be
bit-identical to the exact kernels), Renderer.precision, and the host CLI's
--precision — CPU only.  tests/test_gpu_precision.py checks what
RT_PRECISION_REFERENCE_FAST computes.
"""
import os
import subprocess

import numpy as np
import pytest

from bwrt import Renderer, abi, scenes

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd", "bin",
                   "bwrt_render")


def test_abi_declares_the_mode(bwrt_lib):
    assert {"rt_set_precision", "rt_get_precision"} <= set(abi.declared_functions())
    assert (abi.RT_PRECISION_EXACT, abi.RT_PRECISION_REFERENCE_FAST) == (0, 1)
    major, minor, _ = (int(x) for x in bwrt_lib.rt_version().decode().split("."))
    assert (major, minor) >= (0, 2)


def test_cpu_context_is_exact_only(bwrt_lib, oracle):
    with Renderer.cpu(2, lib=bwrt_lib) as r:
        lib, ctx = r.lib, r.ctx
        assert lib.rt_get_precision(ctx) == abi.RT_PRECISION_EXACT
        assert lib.rt_set_precision(ctx, abi.RT_PRECISION_EXACT) == abi.RT_OK
        assert lib.rt_set_precision(ctx, abi.RT_PRECISION_REFERENCE_FAST) == abi.RT_ERR_UNSUPPORTED
        text = lib.rt_last_error(ctx).decode()
        assert "REFERENCE_FAST" in text and "CPU" in text and "not supported" in text, text
        assert lib.rt_set_precision(ctx, 7) == abi.RT_ERR_INVALID_ARGUMENT
        assert lib.rt_get_precision(ctx) == abi.RT_PRECISION_EXACT
        with pytest.raises(abi.RTError, match="unsupported"):
            r.set_precision("fast")
        # after the refusals the context still renders bit-exactly
        scene = scenes.scene_01()
        r.set_scene(scene)
        r.init_rand(64, 64)
        img, acc = r.render(64, 64, 1, 1, first_frame=1, want_accum=True)
        st = oracle.render_image(scene, 64, 64, 1, 1)
        assert np.array_equal(img, st.rgba)
        assert np.array_equal(acc, st.accum, equal_nan=True)
        rng, _ = r.get_state(64, 64)
        assert np.array_equal(rng, st.rng)
    assert bwrt_lib.rt_set_precision(None, abi.RT_PRECISION_EXACT) == abi.RT_ERR_INVALID_ARGUMENT
    assert bwrt_lib.rt_get_precision(None) == abi.RT_PRECISION_EXACT


def test_renderer_precision_round_trips(bwrt_lib):
    with Renderer.cpu(1, lib=bwrt_lib) as r:
        assert r.precision == "exact"
        r.set_precision("exact")
        assert r.precision == "exact"
        with pytest.raises(ValueError):
            r.set_precision("bogus")
        assert r.precision == "exact"


def test_cli_precision_option(tmp_path):
    def run(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)

    r = run("--help")
    assert r.returncode == 0 and "--precision exact|fast" in r.stdout
    r = run("--precision", "bogus")
    assert r.returncode == 2 and "usage:" in r.stderr, (r.returncode, r.stderr)
    small = ("--scene", "01", "--width", "64", "--height", "64", "--frames", "1", "--max-bounces", "1")
    r = run("--cpu", "2", "--precision", "fast", *small)
    assert r.returncode not in (0, 2), (r.returncode, r.stderr)
    assert "rt_set_precision failed" in r.stderr and "not supported on a CPU context" in r.stderr, r.stderr
    out = tmp_path / "exact.ppm"
    r = run("--cpu", "2", "--precision", "exact", *small, "--out", str(out))
    assert r.returncode == 0, r.stderr
    assert out.stat().st_size > 64 * 64 * 3
