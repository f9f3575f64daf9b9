"""Python host mirror of the reference's render driver over the C ABI.

Mirrors /root/reference/bwidman-raytracer/src/Main.cu: allocateScene()
(:38-109) -> Renderer.set_scene(); the frame loop's render() +
accumulatedFrames++ (:467-480) -> Renderer.render(); controls()' reset
(Controls.cuh:15..69) -> Renderer.reset_accumulation() / set_camera().
Every call goes to libbwrt.so: Renderer(device) renders with the HIP
kernels; Renderer.cpu(threads) makes a context of the library's scalar C++
CPU fallback (rt_create_cpu, the same per-ray arithmetic, bit-identical
results).  A GPU renderer never falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi


class Renderer:
    def __init__(self, device: int = 0, lib=None, _cpu_threads=None):
        self.lib = lib or abi.load()
        self.ctx = C.c_void_p()
        if _cpu_threads is None:
            abi.check(self.lib, self.lib.rt_create(device, C.byref(self.ctx)))
        else:
            abi.check(self.lib, self.lib.rt_create_cpu(_cpu_threads, C.byref(self.ctx)))
        self.device = device if _cpu_threads is None else -1
        self.scene = None

    @classmethod
    def cpu(cls, threads: int = 0, lib=None) -> "Renderer":
        """A context of the scalar C++ CPU fallback on `threads` host threads
        (0 = every CPU this process may run on)."""
        return cls(-1, lib=lib, _cpu_threads=threads)

    @property
    def is_cpu(self) -> bool:
        return self.device < 0

    @property
    def threads(self) -> int:
        """Host threads of a CPU renderer (0 for a GPU one)."""
        return self.lib.rt_context_threads(self.ctx)

    # -- context lifetime -------------------------------------------------
    def close(self):
        if self.ctx:
            self.lib.rt_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, status):
        return abi.check(self.lib, status, self.ctx)

    # -- scene / camera / accumulation -----------------------------------
    def set_scene(self, scene):
        self.scene = scene
        self._check(self.lib.rt_set_scene(self.ctx, C.byref(scene.struct)))

    def set_camera(self, camera):
        self._check(self.lib.rt_set_camera(self.ctx, C.byref(camera)))

    def reset_accumulation(self):
        self._check(self.lib.rt_reset_accumulation(self.ctx))

    @property
    def frame_counter(self) -> int:
        return self.lib.rt_frame_counter(self.ctx)

    def set_max_bounces(self, mb: int):
        self._check(self.lib.rt_set_max_bounces(self.ctx, mb))

    def set_background(self, r: float, g: float, b: float):
        """backgroundColor (Main.cu:27): radiance of misses and the depth cut-off."""
        self._check(self.lib.rt_set_background(self.ctx, r, g, b))

    _PRECISIONS = {"exact": abi.RT_PRECISION_EXACT, "fast": abi.RT_PRECISION_REFERENCE_FAST}

    def set_precision(self, mode: str):
        """rt_set_precision: "exact" (the default: bit-identical to the oracle)
        or "fast" (the reference's fast-math trade-off: hardware rcp / sqrt /
        sin / cos and FMAs; GPU renderers only).  Takes effect at the next
        render; accumulation, frame counter and RNG streams stay."""
        if mode not in self._PRECISIONS:
            raise ValueError(f"precision {mode!r}: expected 'exact' or 'fast'")
        self._check(self.lib.rt_set_precision(self.ctx, self._PRECISIONS[mode]))

    @property
    def precision(self) -> str:
        return "fast" if self.lib.rt_get_precision(self.ctx) == abi.RT_PRECISION_REFERENCE_FAST else "exact"

    def set_light_sampling(self, on):
        """rt_set_light_sampling: next-event estimation (sample the emissive
        spheres at diffuse bounces) for the following render calls.  Another
        estimator of the same expectation; accumulation, frame counter and RNG
        streams stay.  Not with precision "fast" (the renders then refuse)."""
        self._check(self.lib.rt_set_light_sampling(self.ctx, int(on)))

    @property
    def light_sampling(self) -> bool:
        return bool(self.lib.rt_get_light_sampling(self.ctx))

    _LIGHT_PICKS = {"uniform": abi.RT_LIGHT_PICK_UNIFORM, "weighted": abi.RT_LIGHT_PICK_WEIGHTED}

    def set_light_picking(self, mode: str):
        """rt_set_light_picking: how light sampling picks the light of a bounce,
        "uniform" (default) or "weighted" (by emitted power, solid angle and a
        cosine bound at the shading point: less noise where the lights' shares
        differ, two passes over the light table per bounce).  Acts only while
        light sampling is on; accumulation, frame counter and RNG streams stay."""
        if mode not in self._LIGHT_PICKS:
            raise ValueError(f"light picking {mode!r}: expected 'uniform' or 'weighted'")
        self._check(self.lib.rt_set_light_picking(self.ctx, self._LIGHT_PICKS[mode]))

    @property
    def light_picking(self) -> str:
        return "weighted" if self.lib.rt_get_light_picking(self.ctx) == abi.RT_LIGHT_PICK_WEIGHTED else "uniform"

    _LIGHT_SHAPES = {"spheres": abi.RT_LIGHT_SHAPES_SPHERES, "all": abi.RT_LIGHT_SHAPES_ALL}

    def set_light_shapes(self, mode: str):
        """rt_set_light_shapes: which emitters light sampling samples, "spheres"
        (default) or "all" (emissive triangles and convex quads as well, by
        area).  Acts only while light sampling is on; accumulation, frame
        counter and RNG streams stay.  lights() returns the table of the
        current mode."""
        if mode not in self._LIGHT_SHAPES:
            raise ValueError(f"light shapes {mode!r}: expected 'spheres' or 'all'")
        self._check(self.lib.rt_set_light_shapes(self.ctx, self._LIGHT_SHAPES[mode]))

    @property
    def light_shapes(self) -> str:
        return "all" if self.lib.rt_get_light_shapes(self.ctx) == abi.RT_LIGHT_SHAPES_ALL else "spheres"

    def lights(self):
        """rt_get_lights: the scene's light table as a structured array with
        fields centre (3 float32), r2, emitted (3 float32) and prim (int32)."""
        dt = np.dtype([("centre", np.float32, 3), ("r2", np.float32), ("emitted", np.float32, 3), ("prim", np.int32)])
        n = self.lib.rt_get_lights(self.ctx, None, 0)
        if n < 0:
            self._check(n)
        raw = np.zeros((max(n, 1), abi.RT_LIGHT_RECORD_FLOATS), np.float32)
        got = self.lib.rt_get_lights(self.ctx, raw.ctypes.data_as(C.POINTER(C.c_float)), n)
        if got < 0:
            self._check(got)
        return raw[:n].view(dt).reshape(n)

    def set_light_hierarchy(self, on):
        """rt_set_light_hierarchy: weighted picking descends a binary tree over
        the light table (at most ceil(log2 n) + 1 levels per bounce) instead of
        walking the table twice.  Acts only while light sampling is on, picking
        is "weighted" and the table holds at least 2 lights; accumulation, frame
        counter and RNG streams stay."""
        self._check(self.lib.rt_set_light_hierarchy(self.ctx, int(on)))

    @property
    def light_hierarchy(self) -> bool:
        return bool(self.lib.rt_get_light_hierarchy(self.ctx))

    def light_tree(self):
        """rt_get_light_tree: the light tree of the current shapes mode's table
        as a structured array with fields centre (3 float32), r2, phi and a, b,
        parent (int32); 2 n - 1 nodes for n >= 2 lights (the internal ones
        first, node n - 1 + j the leaf of light j), none below that."""
        dt = np.dtype([("centre", np.float32, 3), ("r2", np.float32), ("phi", np.float32), ("a", np.int32),
                       ("b", np.int32), ("parent", np.int32)])
        n = self.lib.rt_get_light_tree(self.ctx, None, 0)
        if n < 0:
            self._check(n)
        raw = np.zeros((max(n, 1), abi.RT_LIGHT_NODE_FLOATS), np.float32)
        got = self.lib.rt_get_light_tree(self.ctx, raw.ctypes.data_as(C.POINTER(C.c_float)), n)
        if got < 0:
            self._check(got)
        return raw[:n].view(dt).reshape(n)

    def light_pick_probabilities(self, points, prims) -> np.ndarray:
        """rt_light_pick_probabilities: where the shadow rays go.  points:
        (count, 6) float32 {P.xyz, n.xyz} (n the shading normal as the path has
        it), prims: (count,) int32, the primitive each point lies on (-1: none).
        Returns (count, n_lights) float32: the probability with which the
        current pick mode (uniform, weighted, or weighted through the light
        hierarchy) picks each table light there."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 6)
        ids = np.ascontiguousarray(prims, np.int32).reshape(-1)
        if len(ids) != len(pts):
            raise ValueError(f"{len(pts)} points but {len(ids)} primitive ids")
        n = self.lib.rt_get_lights(self.ctx, None, 0)
        if n < 0:
            self._check(n)
        out = np.zeros((len(pts), n), np.float32)
        got = self.lib.rt_light_pick_probabilities(self.ctx, pts.ctypes.data_as(C.POINTER(C.c_float)),
                                                   ids.ctypes.data_as(C.POINTER(C.c_int)), len(pts),
                                                   out.ctypes.data_as(C.POINTER(C.c_float)))
        if got < 0:
            self._check(got)
        return out

    def set_samples_per_pixel(self, n: int):
        """samplesPerPixel (Main.cu:27, 296-299): n paths per frame from one
        jittered camera ray, the last one kept and scaled by 1/n (default 1)."""
        self._check(self.lib.rt_set_samples_per_pixel(self.ctx, n))

    def get_camera(self):
        from .abi import Camera
        cam = Camera()
        self._check(self.lib.rt_get_camera(self.ctx, C.byref(cam)))
        return cam

    def controls(self, keys, delta_time: float) -> int:
        """controls() (Controls.cuh:5-75) for one frame: `keys` is an int mask
        or an iterable of key names ("W", "LEFT", ...).  Returns the
        RT_CONTROLS_* flags; movement restarts accumulation."""
        from .abi import KEYS
        if not isinstance(keys, int):
            keys = sum(KEYS[k] for k in keys)
        flags = self.lib.rt_controls(self.ctx, keys, delta_time)
        if flags < 0:
            self._check(flags)
        return flags

    def init_rand(self, width, height, row_offset=0, row_stride=1):
        self._check(self.lib.rt_init_rand(self.ctx, width, height, row_offset, row_stride))

    # -- rendering ----------------------------------------------------------
    @staticmethod
    def params(width, height, samples, max_bounces, first_frame=0, row_offset=0, row_stride=1):
        return abi.RenderParams(width, height, samples, max_bounces, first_frame, row_offset,
                                row_stride)

    def render_simple(self, width: int, height: int, samples: int) -> np.ndarray:
        """Drop-in render(width, height, samples): continue accumulation."""
        out = np.empty((height, width, 4), dtype=np.uint8)
        self._check(self.lib.rt_render(self.ctx, width, height, samples, out.ctypes.data))
        return out

    def render(self, width, height, samples, max_bounces=abi.RT_DEFAULT_MAX_BOUNCES, first_frame=0,
               row_offset=0, row_stride=1, want_accum=False):
        rows = self.lib.rt_shard_rows(height, row_offset, row_stride)
        out = np.empty((rows, width, 4), dtype=np.uint8)
        acc = np.empty((rows, width, 3), dtype=np.float32) if want_accum else None
        p = self.params(width, height, samples, max_bounces, first_frame, row_offset, row_stride)
        self._check(self.lib.rt_render_ex(self.ctx, C.byref(p), out.ctypes.data,
                                          acc.ctypes.data if acc is not None else None))
        return (out, acc) if want_accum else out

    def render_cpu(self, width, height, samples, max_bounces=abi.RT_DEFAULT_MAX_BOUNCES, first_frame=0,
                   row_offset=0, row_stride=1, threads=0, want_accum=False):
        """rt_render_cpu: render() on a CPU renderer with this call's thread count."""
        rows = self.lib.rt_shard_rows(height, row_offset, row_stride)
        out = np.empty((rows, width, 4), dtype=np.uint8)
        acc = np.empty((rows, width, 3), dtype=np.float32) if want_accum else None
        p = self.params(width, height, samples, max_bounces, first_frame, row_offset, row_stride)
        self._check(self.lib.rt_render_cpu(self.ctx, C.byref(p), threads, out.ctypes.data,
                                           acc.ctypes.data if acc is not None else None))
        return (out, acc) if want_accum else out

    def render_device(self, params: abi.RenderParams, rgba_ptr: int, stream_ptr: int | None = None):
        self._check(self.lib.rt_render_device(self.ctx, C.byref(params), rgba_ptr, stream_ptr))

    def synchronize(self):
        self._check(self.lib.rt_synchronize(self.ctx))

    def stream_handle(self) -> int:
        """The context's own hipStream_t (rt_get_stream): renders on it defer
        their end event (no marker packet between back-to-back renders)."""
        return self.lib.rt_get_stream(self.ctx) or 0

    def sky_table(self, width, height, row_offset=0, row_stride=1, tile_w=-1, tile_sq=False):
        """rt_sky_table: (bits, builds) for a view.  bits: one bool per wave
        tile of the launch order (tile_w x 64 / tile_w pixels; tile_w -1 = the
        launch policy's), True where every camera ray provably misses; builds:
        the tables this context has built so far (a cache-key diagnostic)."""
        p = self.params(width, height, 1, 0, 0, row_offset, row_stride)
        tiles, builds = C.c_longlong(), C.c_ulonglong()
        self._check(self.lib.rt_sky_table(self.ctx, C.byref(p), tile_w, int(bool(tile_sq)), None, 0,
                                          C.byref(tiles), C.byref(builds)))
        words = np.zeros(tiles.value // 32 + 1, np.uint32)
        self._check(self.lib.rt_sky_table(self.ctx, C.byref(p), tile_w, int(bool(tile_sq)), words.ctypes.data,
                                          words.size, C.byref(tiles), C.byref(builds)))
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:tiles.value].astype(bool)
        return bits, builds.value

    def last_kernel_ms(self) -> float:
        return self.lib.rt_last_kernel_ms(self.ctx)

    def last_kernel_name(self) -> str:
        """The render kernel the last GPU render launched (rt_last_kernel_name)."""
        return self.lib.rt_last_kernel_name(self.ctx).decode()

    def set_kernel_timing(self, enable: bool):
        """Per-launch timing events for last_kernel_ms (rt_set_kernel_timing)."""
        self._check(self.lib.rt_set_kernel_timing(self.ctx, int(bool(enable))))

    def deinterleave_device(self, gathered_ptr, image_ptr, width, height, shards, rows_per_shard,
                            stream_ptr=None):
        self._check(self.lib.rt_deinterleave_rows_device(self.ctx, gathered_ptr, image_ptr, width,
                                                         height, shards, rows_per_shard,
                                                         stream_ptr))

    # -- first-hit features and the denoiser --------------------------------
    def render_aov(self, width, height, row_offset=0, row_stride=1, only=None):
        """rt_render_aov: the first-hit feature buffers of a shard as a dict of
        arrays: "albedo", "normal" (rows, width, 3) float32, "depth" (rows,
        width) float32 (+inf on a miss), "prim" (rows, width) int32 (-1).
        `only`: the names to compute; the call gets NULL for the others."""
        rows = self.lib.rt_shard_rows(height, row_offset, row_stride)
        shapes = {"albedo": ((rows, width, 3), np.float32), "normal": ((rows, width, 3), np.float32),
                  "depth": ((rows, width), np.float32), "prim": ((rows, width), np.int32)}
        names = list(shapes) if only is None else [only] if isinstance(only, str) else list(only)
        if not names or set(names) - set(shapes):
            raise ValueError(f"only={only!r}: expected names out of {list(shapes)}")
        out = {k: np.empty(*shapes[k]) for k in shapes if k in names}
        ptr = [out[k].ctypes.data if k in out else None for k in ("albedo", "normal", "depth", "prim")]
        p = self.params(width, height, 1, 0, 0, row_offset, row_stride)
        self._check(self.lib.rt_render_aov(self.ctx, C.byref(p), *ptr))
        return out

    def denoise_params(self, iterations=None, sigma_color=None, sigma_normal=None, sigma_plane=None):
        """rt_denoise_params_default() with the given fields replaced."""
        d = self.lib.rt_denoise_params_default()
        for name, v in (("iterations", iterations), ("sigma_color", sigma_color),
                        ("sigma_normal", sigma_normal), ("sigma_plane", sigma_plane)):
            if v is not None:
                setattr(d, name, v)
        return d

    def denoise(self, width, height, iterations=None, sigma_color=None, sigma_normal=None, sigma_plane=None,
                want_color=False):
        """rt_denoise: the a-trous filter over the accumulated full frame
        (width x height: the shape of the last render).  Returns the RGBA8
        image, with want_color also the filtered linear colour (H, W, 3)."""
        d = self.denoise_params(iterations, sigma_color, sigma_normal, sigma_plane)
        out = np.empty((height, width, 4), np.uint8)
        col = np.empty((height, width, 3), np.float32) if want_color else None
        self._check(self.lib.rt_denoise(self.ctx, C.byref(d), out.ctypes.data,
                                        col.ctypes.data if col is not None else None))
        return (out, col) if want_color else out

    def denoise_device(self, rgba_ptr: int, stream_ptr: int | None = None, iterations=None, sigma_color=None,
                       sigma_normal=None, sigma_plane=None):
        """rt_denoise_device: the filtered RGBA8 into device memory on a stream
        (asynchronous; ordered after the last render on the device)."""
        d = self.denoise_params(iterations, sigma_color, sigma_normal, sigma_plane)
        self._check(self.lib.rt_denoise_device(self.ctx, C.byref(d), rgba_ptr, stream_ptr))

    def last_denoise_ms(self) -> float:
        return self.lib.rt_last_denoise_ms(self.ctx)

    # -- variance-guided filter -------------------------------------------------
    def denoise_var_params(self, iterations=None, sigma_lum=None, sigma_normal=None, sigma_plane=None,
                           min_batches=None):
        """rt_denoise_var_params_default() with the given fields replaced."""
        d = self.lib.rt_denoise_var_params_default()
        for name, v in (("iterations", iterations), ("sigma_lum", sigma_lum), ("sigma_normal", sigma_normal),
                        ("sigma_plane", sigma_plane), ("min_batches", min_batches)):
            if v is not None:
                setattr(d, name, v)
        return d

    def denoise_var(self, width, height, want_color=False, want_var=False, **params):
        """rt_denoise_var: the variance-guided a-trous filter over the
        accumulated full frame (width x height: the shape of the last render);
        `params` are denoise_var_params() fields.  Returns the RGBA8 image,
        with want_color / want_var also the filtered linear colour (H, W, 3)
        and the filtered variance of the mean luminance (H, W), in that order."""
        d = self.denoise_var_params(**params)
        out = np.empty((height, width, 4), np.uint8)
        col = np.empty((height, width, 3), np.float32) if want_color else None
        var = np.empty((height, width), np.float32) if want_var else None
        self._check(self.lib.rt_denoise_var(self.ctx, C.byref(d), out.ctypes.data,
                                            col.ctypes.data if col is not None else None,
                                            var.ctypes.data if var is not None else None))
        res = (out,) + ((col,) if want_color else ()) + ((var,) if want_var else ())
        return res if len(res) > 1 else out

    def denoise_var_device(self, rgba_ptr: int, stream_ptr: int | None = None, **params):
        """rt_denoise_var_device: the filtered RGBA8 into device memory on a
        stream (asynchronous; ordered after the last render on the device)."""
        d = self.denoise_var_params(**params)
        self._check(self.lib.rt_denoise_var_device(self.ctx, C.byref(d), rgba_ptr, stream_ptr))

    def last_denoise_var_ms(self) -> float:
        return self.lib.rt_last_denoise_var_ms(self.ctx)

    # -- temporal reprojection ------------------------------------------------
    def temporal_params(self, max_history=None, normal_cos_min=None, plane_tol=None):
        """rt_temporal_params_default() with the given fields replaced."""
        t = self.lib.rt_temporal_params_default()
        for name, v in (("max_history", max_history), ("normal_cos_min", normal_cos_min), ("plane_tol", plane_tol)):
            if v is not None:
                setattr(t, name, v)
        return t

    def _dn(self, denoise):
        """None, or a dict of denoise_params() fields -> a pointer argument."""
        return None if denoise is None else C.byref(self.denoise_params(**denoise))

    def temporal(self, width, height, max_history=None, normal_cos_min=None, plane_tol=None, denoise=None,
                 want_color=False, want_length=False):
        """rt_temporal: reproject the previous view's accumulated colour into
        the accumulated full frame (width x height: the shape of the last
        render) and blend; `denoise` (a dict of denoise_params() fields, {} =
        the defaults) runs the a-trous filter over the result.  Returns the
        RGBA8 image, with want_color / want_length also the linear colour (H,
        W, 3) and the effective sample count (H, W), in that order."""
        t = self.temporal_params(max_history, normal_cos_min, plane_tol)
        out = np.empty((height, width, 4), np.uint8)
        col = np.empty((height, width, 3), np.float32) if want_color else None
        ln = np.empty((height, width), np.float32) if want_length else None
        self._check(self.lib.rt_temporal(self.ctx, C.byref(t), self._dn(denoise), out.ctypes.data,
                                         col.ctypes.data if col is not None else None,
                                         ln.ctypes.data if ln is not None else None))
        res = (out,) + ((col,) if want_color else ()) + ((ln,) if want_length else ())
        return res if len(res) > 1 else out

    def temporal_device(self, rgba_ptr: int, stream_ptr: int | None = None, max_history=None, normal_cos_min=None,
                        plane_tol=None, denoise=None):
        """rt_temporal_device: the temporal (and, with `denoise`, filtered)
        RGBA8 into device memory on a stream (asynchronous; ordered after the
        last render, denoise and temporal call on the device)."""
        t = self.temporal_params(max_history, normal_cos_min, plane_tol)
        self._check(self.lib.rt_temporal_device(self.ctx, C.byref(t), self._dn(denoise), rgba_ptr, stream_ptr))

    def temporal_reset(self):
        """rt_temporal_reset: drop the history and the pending result."""
        self._check(self.lib.rt_temporal_reset(self.ctx))

    def last_temporal_ms(self) -> float:
        return self.lib.rt_last_temporal_ms(self.ctx)

    # -- temporal reprojection of the luminance moments --------------------------
    def _dv(self, denoise_var):
        """None, or a dict of denoise_var_params() fields -> a pointer argument."""
        return None if denoise_var is None else C.byref(self.denoise_var_params(**denoise_var))

    def temporal_var(self, width, height, denoise_var=None, want_color=False, want_length=False,
                     want_moments=False, **tp):
        """rt_temporal_var: rt_temporal that also carries a per-pixel variance
        estimate across camera moves; `tp` are temporal_params() fields,
        `denoise_var` (a dict of denoise_var_params() fields, {} = the
        defaults) runs the variance-guided levels over the result.  Returns the
        RGBA8 image, with want_color / want_length / want_moments also the
        linear colour (H, W, 3), the effective sample count (H, W) and {variance
        of the mean luminance, degrees of freedom} (H, W, 2), in that order."""
        return self._temporal_var(self.lib.rt_temporal_var, width, height, denoise_var, want_color, want_length,
                                  want_moments, tp)

    def _temporal_var(self, fn, width, height, denoise_var, want_color, want_length, want_moments, tp):
        t = self.temporal_params(**tp)
        out = np.empty((height, width, 4), np.uint8)
        col = np.empty((height, width, 3), np.float32) if want_color else None
        ln = np.empty((height, width), np.float32) if want_length else None
        mom = np.empty((height, width, 2), np.float32) if want_moments else None
        self._check(fn(self.ctx, C.byref(t), self._dv(denoise_var), out.ctypes.data,
                       col.ctypes.data if col is not None else None,
                       ln.ctypes.data if ln is not None else None,
                       mom.ctypes.data if mom is not None else None))
        res = ((out,) + ((col,) if want_color else ()) + ((ln,) if want_length else ())
               + ((mom,) if want_moments else ()))
        return res if len(res) > 1 else out

    def temporal_var_counted(self, width, height, denoise_var=None, want_color=False, want_length=False,
                             want_moments=False, **tp):
        """rt_temporal_var_counted: temporal_var on a non-uniform frame (after an
        adaptive call, or a counted assembled frame; set_adaptive_filters on):
        every pixel merges with its own frame and batch counts.  Arguments and
        results as temporal_var, which it equals on a uniform frame."""
        return self._temporal_var(self.lib.rt_temporal_var_counted, width, height, denoise_var, want_color,
                                  want_length, want_moments, tp)

    def temporal_var_counted_device(self, rgba_ptr: int, stream_ptr: int | None = None, denoise_var=None, **tp):
        """rt_temporal_var_counted_device: as temporal_var_device."""
        t = self.temporal_params(**tp)
        self._check(self.lib.rt_temporal_var_counted_device(self.ctx, C.byref(t), self._dv(denoise_var), rgba_ptr,
                                                            stream_ptr))

    def temporal_var_device(self, rgba_ptr: int, stream_ptr: int | None = None, denoise_var=None, **tp):
        """rt_temporal_var_device: the reprojected (and, with `denoise_var`,
        filtered) RGBA8 into device memory on a stream (asynchronous; ordered as
        temporal_device)."""
        t = self.temporal_params(**tp)
        self._check(self.lib.rt_temporal_var_device(self.ctx, C.byref(t), self._dv(denoise_var), rgba_ptr,
                                                    stream_ptr))

    def last_temporal_var_ms(self) -> float:
        return self.lib.rt_last_temporal_var_ms(self.ctx)

    # -- luminance moment tracking ---------------------------------------------
    def set_moments(self, enable: bool = True):
        """rt_set_moments: track per-pixel luminance moments behind every render
        call (one batch per call); live from the next render of frame 1."""
        self._check(self.lib.rt_set_moments(self.ctx, int(bool(enable))))

    @property
    def moments(self) -> bool:
        return bool(self.lib.rt_get_moments(self.ctx))

    @property
    def moments_batches(self) -> int:
        """Tracked render calls J of the current accumulation (0: not live)."""
        return self.lib.rt_moments_batches(self.ctx)

    def variance(self, rows, width, want_lum=False):
        """rt_get_variance: the (rows, width) unbiased estimate of the variance
        of each pixel's mean luminance after the accumulated frames (needs two
        tracked render calls); with want_lum also that mean luminance."""
        var = np.empty((rows, width), np.float32)
        lum = np.empty((rows, width), np.float32) if want_lum else None
        self._check(self.lib.rt_get_variance(self.ctx, var.ctypes.data, lum.ctypes.data if want_lum else None))
        return (var, lum) if want_lum else var

    # -- adaptive sampling ------------------------------------------------------
    def adaptive_params(self, samples=None, tolerance=None, lum_floor=None, radius=None, min_frames=None,
                        max_frames=None):
        """rt_adaptive_params_default() with the given fields replaced."""
        d = self.lib.rt_adaptive_params_default()
        for name, v in (("samples", samples), ("tolerance", tolerance), ("lum_floor", lum_floor), ("radius", radius),
                        ("min_frames", min_frames), ("max_frames", max_frames)):
            if v is not None:
                setattr(d, name, v)
        return d

    @staticmethod
    def _stats(st):
        return {"selected": st.selected, "frames_total": st.frames_total, "select_ms": st.select_ms,
                "render_ms": st.render_ms, "resolve_ms": st.resolve_ms}

    def render_adaptive(self, width, height, max_bounces=-1, want_color=False, **params):
        """rt_render_adaptive: `samples` more frames for the pixels the tracked
        moments select (width x height: the shape of the accumulated full
        frame; max_bounces < 0: the context's); `params` are adaptive_params()
        fields.  Returns (RGBA8 image, stats dict), with want_color (image,
        frameSum / n_p as (H, W, 3) float32, stats)."""
        d = self.adaptive_params(**params)
        out = np.empty((height, width, 4), np.uint8)
        col = np.empty((height, width, 3), np.float32) if want_color else None
        st = abi.AdaptiveStats()
        self._check(self.lib.rt_render_adaptive(self.ctx, C.byref(d), max_bounces, out.ctypes.data,
                                                col.ctypes.data if col is not None else None, C.byref(st)))
        return (out, col, self._stats(st)) if want_color else (out, self._stats(st))

    def render_adaptive_device(self, rgba_ptr: int, stream_ptr: int | None = None, max_bounces=-1, **params):
        """rt_render_adaptive_device: the adaptive call with its RGBA8 into
        device memory on a stream (asynchronous, ordered like render_device)."""
        d = self.adaptive_params(**params)
        self._check(self.lib.rt_render_adaptive_device(self.ctx, C.byref(d), max_bounces, rgba_ptr, stream_ptr))

    def adaptive_reprojected_params(self, min_dof=None, **params):
        """rt_adaptive_reprojected_params_default() with the given fields
        replaced (adaptive_params()'s and min_dof)."""
        d = self.lib.rt_adaptive_reprojected_params_default()
        for name, v in dict(params, min_dof=min_dof).items():
            if name not in dict(abi.AdaptiveReprojectedParams._fields_):
                raise TypeError(f"unknown adaptive parameter {name!r}")
            if v is not None:
                setattr(d, name, v)
        return d

    def render_adaptive_reprojected(self, width, height, max_bounces=-1, want_color=False, **params):
        """rt_render_adaptive_reprojected: `samples` more frames for the pixels
        that the pending planes of the current view select (temporal_var's
        {colour, length, s2, dof}: a moving camera needs one render call per
        view, not two); `params` are adaptive_reprojected_params() fields.
        Returns what render_adaptive returns."""
        d = self.adaptive_reprojected_params(**params)
        out = np.empty((height, width, 4), np.uint8)
        col = np.empty((height, width, 3), np.float32) if want_color else None
        st = abi.AdaptiveStats()
        self._check(self.lib.rt_render_adaptive_reprojected(self.ctx, C.byref(d), max_bounces, out.ctypes.data,
                                                            col.ctypes.data if col is not None else None,
                                                            C.byref(st)))
        return (out, col, self._stats(st)) if want_color else (out, self._stats(st))

    def render_adaptive_reprojected_device(self, rgba_ptr: int, stream_ptr: int | None = None, max_bounces=-1,
                                           **params):
        """rt_render_adaptive_reprojected_device: as render_adaptive_device."""
        d = self.adaptive_reprojected_params(**params)
        self._check(self.lib.rt_render_adaptive_reprojected_device(self.ctx, C.byref(d), max_bounces, rgba_ptr,
                                                                   stream_ptr))

    def adaptive_stats(self) -> dict:
        """rt_adaptive_last_stats: the last adaptive call's statistics (synchronises)."""
        st = abi.AdaptiveStats()
        self._check(self.lib.rt_adaptive_last_stats(self.ctx, C.byref(st)))
        return self._stats(st)

    def counts(self, rows, width):
        """rt_get_counts: per-pixel (frames accumulated, moment batches
        tracked), two (rows, width) uint32 arrays."""
        n = np.empty((rows, width), np.uint32)
        j = np.empty((rows, width), np.uint32)
        self._check(self.lib.rt_get_counts(self.ctx, n.ctypes.data, j.ctypes.data))
        return n, j

    # -- adaptive sampling on row shards (two phases around an all-gather) -------
    def adaptive_export_rows(self, rows_per_shard, width, **params):
        """rt_adaptive_export_rows, phase 1: the window's row sums of this
        context's own rows, a (3, rows_per_shard, width) float32 block — sum v,
        sum M, and the tap counts as int32 bits (block[2].view(np.int32)) — the
        shard's rows first, zero rows after them.  Changes nothing of the
        accumulation; `params` as render_adaptive's (the radius matters)."""
        d = self.adaptive_params(**params)
        block = np.empty((3, rows_per_shard, width), np.float32)
        self._check(self.lib.rt_adaptive_export_rows(self.ctx, C.byref(d), rows_per_shard, block.ctypes.data))
        return block

    def adaptive_export_rows_device(self, block_ptr: int, rows_per_shard, stream_ptr: int | None = None, **params):
        """rt_adaptive_export_rows_device: the block into device memory on a
        stream (asynchronous, ordered like export_shard_device)."""
        d = self.adaptive_params(**params)
        self._check(self.lib.rt_adaptive_export_rows_device(self.ctx, C.byref(d), rows_per_shard, block_ptr, stream_ptr))

    def render_adaptive_shard(self, gathered, rows, width, max_bounces=-1, want_color=False, **params):
        """rt_render_adaptive_shard, phase 2: select this context's rows from
        `gathered`, (shards, 3, rows_per_shard, width) float32 on the host
        (block r = rows r, r + shards, ...), then render, update and resolve
        them.  Returns the shard's `rows` rows in shard order like
        render_adaptive: (RGBA8, stats) or (RGBA8, colour, stats)."""
        d = self.adaptive_params(**params)
        g = np.ascontiguousarray(gathered, dtype=np.float32)
        shards, _, rps, _ = g.shape
        out = np.empty((rows, width, 4), np.uint8)
        col = np.empty((rows, width, 3), np.float32) if want_color else None
        st = abi.AdaptiveStats()
        self._check(self.lib.rt_render_adaptive_shard(self.ctx, C.byref(d), max_bounces, g.ctypes.data, shards, rps,
                                                      out.ctypes.data, col.ctypes.data if col is not None else None,
                                                      C.byref(st)))
        return (out, col, self._stats(st)) if want_color else (out, self._stats(st))

    def render_adaptive_shard_device(self, gathered_ptr: int, shards, rows_per_shard, rgba_ptr: int | None = None,
                                     stream_ptr: int | None = None, max_bounces=-1, **params):
        """rt_render_adaptive_shard_device: phase 2 from device memory with its
        RGBA8 rows into device memory on a stream (asynchronous, no host
        synchronisation; the caller orders the gather before it)."""
        d = self.adaptive_params(**params)
        self._check(self.lib.rt_render_adaptive_shard_device(self.ctx, C.byref(d), max_bounces, gathered_ptr, shards,
                                                             rows_per_shard, rgba_ptr, stream_ptr))

    def set_adaptive_filters(self, enable: bool = True):
        """rt_set_adaptive_filters: let denoise, denoise_var and temporal (and
        their _device forms) run on a non-uniform accumulation, each pixel
        with its own frame count; off (the default) they refuse it."""
        self._check(self.lib.rt_set_adaptive_filters(self.ctx, int(bool(enable))))

    @property
    def adaptive_filters(self) -> bool:
        return bool(self.lib.rt_get_adaptive_filters(self.ctx))

    # -- row shards into one frame: the assembled frame -------------------------
    # (one body per pair of an uncounted entry point and its counted twin: `fn`
    # is the C function)
    def _export_shard(self, fn, rows_per_shard, width, planes):
        block = np.empty((planes, rows_per_shard, width), np.float32)
        n, j = C.c_uint(), C.c_uint()
        self._check(fn(self.ctx, rows_per_shard, planes, block.ctypes.data, C.byref(n), C.byref(j)))
        return block, n.value, j.value

    def _export_shard_device(self, fn, block_ptr, rows_per_shard, planes, stream_ptr):
        n, j = C.c_uint(), C.c_uint()
        self._check(fn(self.ctx, rows_per_shard, planes, block_ptr, stream_ptr, C.byref(n), C.byref(j)))
        return n.value, j.value

    def _assemble(self, fn, gathered, frames, batches):
        g = np.ascontiguousarray(gathered, dtype=np.float32)
        shards, planes, rps, _ = g.shape
        self._check(fn(self.ctx, g.ctypes.data, shards, rps, planes, frames, batches))

    def _assemble_device(self, fn, gathered_ptr, shards, rows_per_shard, planes, frames, batches, stream_ptr):
        self._check(fn(self.ctx, gathered_ptr, shards, rows_per_shard, planes, frames, batches, stream_ptr))

    def export_shard(self, rows_per_shard, width, planes=3):
        """rt_export_shard: this context's block, (planes, rows_per_shard,
        width) float32 — R, G, B of frameSum (then M, M2 with planes=5), the
        shard's rows first, zero rows after them — and the (frames, batches)
        it stands for."""
        return self._export_shard(self.lib.rt_export_shard, rows_per_shard, width, planes)

    def export_shard_device(self, block_ptr: int, rows_per_shard, planes=3, stream_ptr: int | None = None):
        """rt_export_shard_device: the block into device memory on a stream
        (asynchronous; after the last render, and the next render after it).
        Returns (frames, batches)."""
        return self._export_shard_device(self.lib.rt_export_shard_device, block_ptr, rows_per_shard, planes, stream_ptr)

    def assemble(self, gathered, frames, batches=0):
        """rt_assemble: make the assembled frame from `gathered`, (shards,
        planes, rows_per_shard, width) float32 on the host: block r holds rows
        r, r + shards, ...  denoise, denoise_var and temporal on a renderer
        whose own state is a row shard then read it, with its frames / batches."""
        self._assemble(self.lib.rt_assemble, gathered, frames, batches)

    def assemble_device(self, gathered_ptr: int, shards, rows_per_shard, planes, frames, batches=0,
                        stream_ptr: int | None = None):
        """rt_assemble_device: the same from device memory on a stream
        (asynchronous; ordered against the passes that read the assembled frame)."""
        self._assemble_device(self.lib.rt_assemble_device, gathered_ptr, shards, rows_per_shard, planes, frames, batches,
                              stream_ptr)

    def assembled(self):
        """rt_assembled: (frames, batches) of the current assembled frame, or None."""
        n, j = C.c_uint(), C.c_uint()
        return (n.value, j.value) if self.lib.rt_assembled(self.ctx, C.byref(n), C.byref(j)) else None

    def get_assembled(self, width, height, want_moments=False):
        """rt_get_assembled: the assembled frameSum as (H, W, 3) float32 (as
        get_state's), with want_moments also {M, M2} as (H, W, 2)."""
        acc = np.empty((height, width, 3), np.float32)
        mom = np.empty((height, width, 2), np.float32) if want_moments else None
        self._check(self.lib.rt_get_assembled(self.ctx, acc.ctypes.data, mom.ctypes.data if want_moments else None))
        return (acc, mom) if want_moments else acc

    def assemble_drop(self):
        """rt_assemble_drop: forget the assembled frame."""
        self._check(self.lib.rt_assemble_drop(self.ctx))

    def last_assemble_ms(self) -> float:
        return self.lib.rt_last_assemble_ms(self.ctx)

    # -- counted blocks: adaptive (non-uniform) frames of row shards ------------
    def export_shard_adaptive(self, rows_per_shard, width, planes=4):
        """rt_export_shard_adaptive: this context's counted block, (planes,
        rows_per_shard, width) float32 — R, G, B of frameSum and n_p (planes=4),
        or R, G, B, M, M2, n_p, J_p (planes=7); the count planes hold uint32
        bits (block[-1].view(np.uint32)) — and the (frames, batches) of the
        uniform base.  Works on a uniform and on a non-uniform accumulation."""
        return self._export_shard(self.lib.rt_export_shard_adaptive, rows_per_shard, width, planes)

    def export_shard_adaptive_device(self, block_ptr: int, rows_per_shard, planes=4, stream_ptr: int | None = None):
        """rt_export_shard_adaptive_device: the counted block into device
        memory on a stream (asynchronous; after the last render or adaptive
        call, and the next render after it).  Returns (frames, batches)."""
        return self._export_shard_device(self.lib.rt_export_shard_adaptive_device, block_ptr, rows_per_shard, planes,
                                         stream_ptr)

    def assemble_adaptive(self, gathered, frames, batches=0):
        """rt_assemble_adaptive: make the assembled frame with its count plane
        from `gathered`, (shards, planes, rows_per_shard, width) float32 counted
        blocks on the host.  With set_adaptive_filters on, denoise, denoise_var
        and temporal on a renderer whose own state is a row shard then take
        every pixel's own counts; `frames` / `batches` are the uniform base."""
        self._assemble(self.lib.rt_assemble_adaptive, gathered, frames, batches)

    def assemble_adaptive_device(self, gathered_ptr: int, shards, rows_per_shard, planes, frames, batches=0,
                                 stream_ptr: int | None = None):
        """rt_assemble_adaptive_device: the same from device memory on a stream
        (asynchronous; ordered like assemble_device)."""
        self._assemble_device(self.lib.rt_assemble_adaptive_device, gathered_ptr, shards, rows_per_shard, planes, frames,
                              batches, stream_ptr)

    def assembled_counts(self, width, height):
        """rt_get_assembled_counts: the counted assembled frame's per-pixel
        (frames, batches), two (H, W) uint32 arrays (as counts())."""
        n = np.empty((height, width), np.uint32)
        j = np.empty((height, width), np.uint32)
        self._check(self.lib.rt_get_assembled_counts(self.ctx, n.ctypes.data, j.ctypes.data))
        return n, j

    # -- checkpoint / resume -----------------------------------------------
    def get_state(self, rows, width):
        rng = np.empty((6, rows, width), dtype=np.uint32)
        acc = np.empty((rows, width, 3), dtype=np.float32)
        self._check(self.lib.rt_get_state(self.ctx, rng.ctypes.data, acc.ctypes.data))
        return rng, acc

    def set_state(self, rng, acc, frame_counter):
        rng = np.ascontiguousarray(rng, dtype=np.uint32)
        acc = np.ascontiguousarray(acc, dtype=np.float32)
        self._check(self.lib.rt_set_state(self.ctx, rng.ctypes.data, acc.ctypes.data,
                                          frame_counter))


def shard_rows(height: int, row_offset: int, row_stride: int) -> int:
    return len(range(row_offset, height, row_stride)) if row_stride > 0 else 0


def _multi_call(renderers, fn, *args, reports: int = 0):
    """A C function over the renderers' contexts: fn(ctxs, n, *args); a failure
    is raised by renderers[reports] (renderers[0] when that is no index)."""
    arr = (C.c_void_p * len(renderers))(*[r.ctx.value for r in renderers])
    rc = fn(arr, len(renderers), *args)
    if rc != abi.RT_OK:
        renderers[reports if 0 <= reports < len(renderers) else 0]._check(rc)


def render_multi(renderers, width: int, height: int, samples: int) -> np.ndarray:
    """rt_render_multi: one image across several Renderers (one per GPU, same
    scene/camera set on each) in this process; returns (H, W, 4) uint8, row 0
    = bottom.  Renderer i renders rows y = i (mod len(renderers))."""
    out = np.empty((height, width, 4), np.uint8)
    _multi_call(renderers, renderers[0].lib.rt_render_multi, width, height, samples, out.ctypes.data)
    return out


def assemble_multi(renderers, planes: int = 0, dst: int = 0):
    """rt_assemble_multi, beside render_multi: every Renderer exports its row
    shard, renderers[dst] assembles them, and its denoise / denoise_var /
    temporal then run on the whole frame.  planes 3, 5 (with the moments), or
    0 = 5 when every renderer's moments are current.  Returns the (frames,
    batches) of the assembled frame."""
    _multi_call(renderers, renderers[0].lib.rt_assemble_multi, planes, dst, reports=dst)
    return renderers[dst].assembled()


def assemble_adaptive_multi(renderers, planes: int = 0, dst: int = 0):
    """rt_assemble_adaptive_multi, beside render_adaptive_multi: assemble_multi
    with counted blocks, for renderers whose accumulations are uniform or
    non-uniform.  planes 4, 7 (with the moments), or 0 = 7 when every
    renderer's moments are current.  Returns the (frames, batches) of the
    uniform base; renderers[dst].assembled_counts() has the pixels' own."""
    _multi_call(renderers, renderers[0].lib.rt_assemble_adaptive_multi, planes, dst, reports=dst)
    return renderers[dst].assembled()


def render_adaptive_multi(renderers, width: int, height: int, max_bounces=-1, **params):
    """rt_render_adaptive_multi, beside render_multi: one adaptive call across
    the Renderers' row shards (export the row sums, copy every block to every
    renderer, select, render, resolve).  Returns ((H, W, 4) uint8 with row 0 =
    bottom, stats dict: selected and frames_total summed, stage times maxima)."""
    d = renderers[0].adaptive_params(**params)
    out = np.empty((height, width, 4), np.uint8)
    st = abi.AdaptiveStats()
    _multi_call(renderers, renderers[0].lib.rt_render_adaptive_multi, C.byref(d), max_bounces, out.ctypes.data, C.byref(st))
    return out, Renderer._stats(st)
