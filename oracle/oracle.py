"""ctypes wrapper of liboracle.so — TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import
this module, as the checker / the CPU baseline.  The product (libbwrt.so,
bwrt package) never imports it.  See oracle.h for what the oracle restates
and how its parity is pinned.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liboracle.so")

_lib = None


def build(force: bool = False) -> str:
    if force or not os.path.exists(LIB_PATH) or \
            os.path.getmtime(LIB_PATH) < max(os.path.getmtime(os.path.join(HERE, f))
                                             for f in ("oracle.c", "oracle.h")):
        subprocess.run(["make", "-B" if force else "-s", "-C", HERE], check=True)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if LIB_PATH_IN_USE == LIB_PATH and not os.path.exists(LIB_PATH):
            build()
        L = C.CDLL(LIB_PATH_IN_USE)
        L.orc_curand_init.argtypes = [C.c_ulonglong, C.POINTER(C.c_uint32)]
        L.orc_curand_init.restype = None
        L.orc_curand.argtypes = [C.POINTER(C.c_uint32)]
        L.orc_curand.restype = C.c_uint32
        for f in ("orc_atanf", "orc_sinf", "orc_cosf"):
            getattr(L, f).argtypes = [C.c_float]
            getattr(L, f).restype = C.c_float
        L.orc_render_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_uint, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_int]
        L.orc_render_rows.restype = C.c_int
        L.orc_first_hit_rows.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 7
        L.orc_first_hit_rows.restype = C.c_int
        L.orc_camera_rays.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 5
        L.orc_camera_rays.restype = C.c_int
        L.orc_closest_hits.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
        L.orc_closest_hits.restype = C.c_int
        L.orc_scatter.argtypes = [C.c_int] + [C.c_void_p] * 7
        L.orc_scatter.restype = C.c_int
        L.orc_set_background.argtypes = [C.c_float, C.c_float, C.c_float]
        L.orc_set_background.restype = None
        L.orc_set_samples_per_pixel.argtypes = [C.c_int]
        L.orc_set_samples_per_pixel.restype = None
        L.orc_last_counters.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
        L.orc_last_counters.restype = None
        _lib = L
    return _lib


def use_library(path: str):
    """Switch to another build of the oracle (the pin-sensitivity mutants,
    tests/golden/make_pin_sensitivity.py); use_library(LIB_PATH) goes back."""
    global _lib, LIB_PATH_IN_USE
    _lib = None
    LIB_PATH_IN_USE = path
    return lib()


LIB_PATH_IN_USE = LIB_PATH


def curand_stream(seed: int, n: int) -> np.ndarray:
    st = (C.c_uint32 * 6)()
    lib().orc_curand_init(seed, st)
    return np.array([lib().orc_curand(st) for _ in range(n)], dtype=np.uint32)


def curand_init(seed: int) -> np.ndarray:
    st = (C.c_uint32 * 6)()
    lib().orc_curand_init(seed, st)
    return np.array(list(st), dtype=np.uint32)


class OracleState:
    """Progressive state of one shard: rng planes (6,rows,W), accum (rows,W,3)."""

    def __init__(self, width, height, row_offset=0, row_stride=1):
        self.width, self.height = width, height
        self.row_offset, self.row_stride = row_offset, row_stride
        self.rows = len(range(row_offset, height, row_stride))
        self.rng = np.zeros((6, self.rows, width), dtype=np.uint32)
        self.accum = np.zeros((self.rows, width, 3), dtype=np.float32)
        self.rgba = np.zeros((self.rows, width, 4), dtype=np.uint8)
        self.seeded = False
        self.frame = 1


def render(scene, state: OracleState, passes: int, max_bounces: int,
           first_frame: int | None = None, threads: int = 0, background=(0.0, 0.0, 0.0),
           samples_per_pixel: int = 1) -> np.ndarray:
    """Render `passes` progressive frames; returns the RGBA8 rows (row 0 = bottom).
    samples_per_pixel: the reference's in-frame loop (Main.cu:27, 296-299)."""
    ff = state.frame if first_frame is None else first_frame
    lib().orc_set_background(*[float(c) for c in background])
    lib().orc_set_samples_per_pixel(int(samples_per_pixel))
    rc = lib().orc_render_rows(C.cast(scene.ptr(), C.c_void_p), state.width, state.height,
                               state.row_offset, state.row_stride, state.rows, ff, passes,
                               max_bounces, state.rng.ctypes.data, state.accum.ctypes.data,
                               state.rgba.ctypes.data, 0 if state.seeded else 1, threads)
    if rc != 0:
        raise ValueError("orc_render_rows: bad arguments")
    state.seeded = True
    state.frame = ff + passes
    return state.rgba


def render_image(scene, width, height, passes, max_bounces, row_offset=0, row_stride=1,
                 threads=0):
    st = OracleState(width, height, row_offset, row_stride)
    render(scene, st, passes, max_bounces, first_frame=1, threads=threads)
    return st


KIND_MISS, KIND_SPHERE, KIND_PLANE, KIND_TRIANGLE, KIND_QUAD = -1, 0, 1, 2, 3


def first_hit(scene, width, height, row_offset=0, row_stride=1, background=(0.0, 0.0, 0.0)):
    """orc_first_hit_rows: the first hit of every shard pixel's un-jittered
    primary ray, as a dict of arrays shaped like Renderer.render_aov's —
    "albedo", "normal" (the unit normal) (rows, width, 3) float32, "depth"
    (rows, width) float32, "prim" (rows, width) int32 in the product's
    numbering: spheres first, then planes, triangles and quads.  A miss gives
    prim -1, depth +inf, normal 0 and albedo = `background`.  Beside them the
    oracle's own record: "kind" (KIND_*), "index" (in the primitive's own
    array), "point" (the intersection) and "raw_normal"."""
    rows = len(range(row_offset, height, row_stride))
    kind = np.empty((rows, width), np.int32)
    index = np.empty((rows, width), np.int32)
    depth = np.empty((rows, width), np.float32)
    point, raw, unit, albedo = (np.empty((rows, width, 3), np.float32) for _ in range(4))
    lib().orc_set_background(*[float(c) for c in background])
    rc = lib().orc_first_hit_rows(C.cast(scene.ptr(), C.c_void_p), width, height, row_offset, row_stride, rows,
                                  *[a.ctypes.data for a in (kind, index, depth, point, raw, unit, albedo)])
    if rc != 0:
        raise ValueError("orc_first_hit_rows: bad arguments")
    ns, npl, nt, _ = scene.counts
    base = np.array([0, ns, ns + npl, ns + npl + nt], np.int32)
    prim = np.where(kind < 0, np.int32(-1), base[np.maximum(kind, 0)] + index).astype(np.int32)
    return {"albedo": albedo, "normal": unit, "depth": depth, "prim": prim,
            "kind": kind, "index": index, "point": point, "raw_normal": raw}


# ---- per-step entry points (tests/nee_path_ref.py) ---------------------------------------

def _in(a, dtype, shape):
    a = np.ascontiguousarray(a, dtype)
    if a.shape != shape:
        raise ValueError(f"expected an array of shape {shape}, got {a.shape}")
    return a


def camera_rays(scene, width, height, x, y, states):
    """orc_camera_rays: the jittered camera rays of pixels (x[i], y[i]) with RNG
    states (n, 6) {d, v0 .. v4}: (origin (n, 3), direction (n, 3), the states after)."""
    n = len(x)
    x, y = _in(x, np.int32, (n,)), _in(y, np.int32, (n,))
    st = _in(states, np.uint32, (n, 6)).copy()
    o, d = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    rc = lib().orc_camera_rays(C.cast(scene.ptr(), C.c_void_p), width, height, n,
                               *[a.ctypes.data for a in (x, y, st, o, d)])
    if rc != 0:
        raise ValueError("orc_camera_rays: bad arguments")
    return o, d, st


def closest_hits(scene, origin, direction):
    """orc_closest_hits for n rays: a dict of "kind", "index", "prim" (the
    product's numbering, -1 on a miss) (n,) int32, "distance" (n,), "point",
    "normal" (unit for a sphere, raw otherwise) (n, 3) and "material" (n, 6:
    albedo, emittance, roughness, refractive index) float32."""
    n = len(origin)
    o, d = _in(origin, np.float32, (n, 3)), _in(direction, np.float32, (n, 3))
    kind, index = np.empty(n, np.int32), np.empty(n, np.int32)
    dist, point, normal = np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    mat = np.empty((n, 6), np.float32)
    rc = lib().orc_closest_hits(C.cast(scene.ptr(), C.c_void_p), n,
                                *[a.ctypes.data for a in (o, d, kind, index, dist, point, normal, mat)])
    if rc != 0:
        raise ValueError("orc_closest_hits: bad arguments")
    ns, npl, nt, _ = scene.counts
    base = np.array([0, ns, ns + npl, ns + npl + nt], np.int32)
    prim = np.where(kind < 0, np.int32(-1), base[np.maximum(kind, 0)] + index).astype(np.int32)
    return {"kind": kind, "index": index, "prim": prim, "distance": dist, "point": point, "normal": normal,
            "material": mat}


def scatter(states, incoming, normal, material):
    """orc_scatter for n hits: (specular (n,) bool, scattered direction (n, 3),
    brdf (n, 3), the states after)."""
    n = len(incoming)
    st = _in(states, np.uint32, (n, 6)).copy()
    i, nr, m = _in(incoming, np.float32, (n, 3)), _in(normal, np.float32, (n, 3)), _in(material, np.float32, (n, 6))
    spec = np.empty(n, np.int32)
    s, b = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    rc = lib().orc_scatter(n, *[a.ctypes.data for a in (st, i, nr, m, spec, s, b)])
    if rc != 0:
        raise ValueError("orc_scatter: bad arguments")
    return spec != 0, s, b, st


def last_counters():
    q, p = C.c_ulonglong(), C.c_ulonglong()
    lib().orc_last_counters(C.byref(q), C.byref(p))
    return q.value, p.value
