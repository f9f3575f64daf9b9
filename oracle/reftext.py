"""ctypes wrapper of oracle/_ref/libreftext.so — TEST INFRASTRUCTURE ONLY.

The library is the reference's own source text (Main.cu and its four headers)
compiled for the CPU by the recipe in oracle/ref/ (stand-in CUDA / GLFW
headers, see oracle/ref/README.md and DESIGN.md section 2).  It is what the
oracle (oracle.c, a restatement) and through it the product are pinned to.
Only tests import this module; smoke() and bench.py never do.

The library exists only where __graft_entry__.build() found the reference
tree (or where a build travelled to): `available()` says whether it is there,
`reference_present()` whether it could be built.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RECIPE = os.path.join(HERE, "ref")
LIB_PATH = os.path.join(HERE, "_ref", "libreftext.so")
REFERENCE_ENV = "RAYTRACER_REFERENCE_DIR"

_lib = None


def reference_dir() -> str:
    """Where the reference tree is looked for (it is never read by a test)."""
    return os.environ.get(REFERENCE_ENV, "/root/reference")


def reference_present() -> bool:
    return os.path.isfile(os.path.join(reference_dir(), "bwidman-raytracer", "src", "Main.cu"))


def available() -> bool:
    return os.path.isfile(LIB_PATH)


def build() -> str | None:
    """Run the recipe when the reference tree is present; otherwise leave an
    existing oracle/_ref/ alone.  Returns the library's path, or None."""
    if reference_present():
        subprocess.run(["make", "-s", "-C", RECIPE, f"REF={reference_dir()}"], check=True)
    return LIB_PATH if available() else None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(LIB_PATH)
        L.ref_render_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_uint, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_int]
        L.ref_render_rows.restype = C.c_int
        L.ref_set_window.argtypes = [C.c_int, C.c_int]
        L.ref_set_window.restype = None
        for f in ("ref_set_max_bounces", "ref_set_samples_per_pixel"):
            getattr(L, f).argtypes = [C.c_int]
            getattr(L, f).restype = None
        L.ref_set_background.argtypes = [C.c_float, C.c_float, C.c_float]
        L.ref_set_background.restype = None
        L.ref_controls.argtypes = [C.c_void_p, C.c_uint, C.c_float]
        L.ref_controls.restype = C.c_int
        _lib = L
    return _lib


def render(scene, state, passes: int, max_bounces: int, first_frame: int | None = None, threads: int = 0,
           background=(0.0, 0.0, 0.0), samples_per_pixel: int = 1) -> np.ndarray:
    """oracle.render's twin: the same arguments and the same oracle.OracleState,
    rendered by the reference's own render() / launchRaytracer / tracePath."""
    ff = state.frame if first_frame is None else first_frame
    lib().ref_set_background(*[float(c) for c in background])
    lib().ref_set_samples_per_pixel(int(samples_per_pixel))
    rc = lib().ref_render_rows(C.cast(scene.ptr(), C.c_void_p), state.width, state.height,
                               state.row_offset, state.row_stride, state.rows, ff, passes,
                               max_bounces, state.rng.ctypes.data, state.accum.ctypes.data,
                               state.rgba.ctypes.data, 0 if state.seeded else 1, threads)
    if rc != 0:
        raise ValueError("ref_render_rows: bad arguments")
    state.seeded = True
    state.frame = ff + passes
    return state.rgba


def controls(camera, keys: int, dt: float) -> int:
    """The reference's controls() on a bwrt.abi.Camera (changed in place) with
    the RT_KEY_* mask `keys` held for `dt` seconds; rt_apply_controls' flags."""
    rc = lib().ref_controls(C.cast(C.byref(camera), C.c_void_p), keys, float(dt))
    if rc < 0:
        raise ValueError("ref_controls: bad arguments")
    return rc
