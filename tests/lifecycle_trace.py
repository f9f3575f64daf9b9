"""Seeded sequences of C ABI calls on one context, and what the context reports
after every call: the frame counter, the moment tracking, the per-pixel counts,
the pixel state, the variance readout, the filters' images and the adaptive
statistics.  No times are recorded, so a recording depends on the library alone:
tests/golden/lifecycle_trace.json is the recording of the library before the
accumulation state got its one owner (csrc/rt_accum.h), and every later library
has to reproduce it (tests/test_lifecycle_trace.py), on the GPU as on the CPU
(tests/test_gpu_adaptive.py).

    python tests/lifecycle_trace.py            the recordings' coverage figures
    python tests/lifecycle_trace.py --write    rewrite the golden from $BWRT_LIB

One rule keeps the sequences inside what all those libraries agree on: between
a call that restarts the accumulation without a render (rt_set_scene,
rt_set_camera, a moving rt_controls, rt_reset_accumulation) and the next call
that settles what the tracked moments describe (a successful uniform render,
rt_init_rand, rt_set_state, an rt_set_moments that flips the switch) no
adaptive call is issued; a render takes its place.  There the old library
continued the old frameSum, and the present one refuses
(tests/test_adaptive.py has that case).
"""
import ctypes as C
import hashlib
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd"))
from bwrt import Renderer, abi, scenes  # noqa: E402

SEEDS = (11, 12, 13, 14)
STEPS = 300
SHAPES = ((33, 17), (20, 9))
BOUNCES = 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lifecycle_trace.json")

# step kinds and their weights: renders and adaptive calls dominate, so that
# the non-uniform state is reached often; the filters and their switch are
# raised so that each filter meets that state with the switch off
WEIGHTS = (("render", 20), ("adaptive", 16), ("denoise", 6), ("denoise_var", 6), ("temporal", 6),
           ("set_filters", 3), ("set_moments", 2), ("set_scene", 1), ("set_camera", 1), ("controls", 2),
           ("reset", 1), ("init_rand", 2), ("state", 2), ("temporal_reset", 1), ("last_stats", 5))

# what a refusal was about: the first of these found in rt_last_error
REASONS = ("non-uniform", "no frame accumulated yet", "not live", "at least 2 batches", "row shard",
           "no adaptive call", "no shard state")


def digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:10]


class Tracer:
    """One context, the generator's view of it, and the recorder."""

    def __init__(self, renderer, seed):
        self.r, self.lib, self.ctx = renderer, renderer.lib, renderer.ctx
        self.rnd = random.Random(seed)
        self.scenes = (scenes.scene_07(), scenes.SCENES["04_box"]())
        self.w, self.h = SHAPES[0]      # the frame of the pixel state
        self.rows = 0                   # its rows (0: no state yet)
        self.restarted = False          # the rule of the module docstring

    def pick(self, seq):
        return seq[int(self.rnd.random() * len(seq))]

    def kind(self):
        x = self.rnd.random() * sum(w for _, w in WEIGHTS)
        for name, w in WEIGHTS:
            x -= w
            if x < 0:
                return name
        return WEIGHTS[-1][0]

    # -- steps: each returns (status, extras of the record) --------------------
    def render(self):
        w, h = self.pick(SHAPES) if self.rnd.random() < 0.1 else (self.w, self.h)
        fc = self.lib.rt_frame_counter(self.ctx)
        first = self.pick((0,) * 8 + (1, fc, fc + 2))
        p = abi.RenderParams(w, h, self.pick((1, 2, 3)), BOUNCES, first, 0, 1)
        rc = self.lib.rt_render_ex(self.ctx, C.byref(p), None, None)
        self.w, self.h, self.rows = w, h, h  # (the implicit rt_init_rand comes before any refusal)
        if rc == 0:
            self.restarted = False
        return rc, {}

    def adaptive(self):
        d = self.r.adaptive_params(samples=self.pick((1, 2)), min_frames=self.pick((0, 0, 100)))
        st = abi.AdaptiveStats()
        rc = self.lib.rt_render_adaptive(self.ctx, C.byref(d), BOUNCES, None, None, C.byref(st))
        return rc, {"stats": [st.selected, st.frames_total]} if rc == 0 else {}

    def _filter(self, call):
        rgba = np.zeros((self.h, self.w, 4), np.uint8)
        rc = call(rgba.ctypes.data)
        return rc, {"rgba": digest(rgba)} if rc == 0 else {}

    def denoise(self):
        d = self.r.denoise_params(iterations=1)
        return self._filter(lambda out: self.lib.rt_denoise(self.ctx, C.byref(d), out, None))

    def denoise_var(self):
        d = self.r.denoise_var_params(iterations=1, min_batches=self.pick((2, 4)))
        return self._filter(lambda out: self.lib.rt_denoise_var(self.ctx, C.byref(d), out, None, None))

    def temporal(self):
        t, d = self.r.temporal_params(), self.r.denoise_params(iterations=1)
        return self._filter(lambda out: self.lib.rt_temporal(self.ctx, C.byref(t), C.byref(d), out, None, None))

    def set_filters(self):
        return self.lib.rt_set_adaptive_filters(self.ctx, int(self.rnd.random() < 0.5)), {}

    def set_moments(self):
        on = int(self.rnd.random() < 0.9)
        if on != self.lib.rt_get_moments(self.ctx):
            self.restarted = False
        return self.lib.rt_set_moments(self.ctx, on), {}

    def set_scene(self):
        rc = self.lib.rt_set_scene(self.ctx, C.byref(self.pick(self.scenes).struct))
        self.restarted = self.restarted or rc == 0
        return rc, {}

    def set_camera(self):
        self.restarted = True
        return self.lib.rt_set_camera(self.ctx, C.byref(self.scenes[0].struct.camera)), {}

    def controls(self):
        moving = self.rnd.random() < 0.5
        flags = self.lib.rt_controls(self.ctx, abi.KEYS["LEFT"] if moving else 0, 0.05)
        self.restarted = self.restarted or bool(flags > 0 and flags & abi.CONTROLS_MOVED)
        return flags, {}

    def reset(self):
        self.restarted = True
        return self.lib.rt_reset_accumulation(self.ctx), {}

    def init_rand(self):
        which = self.pick(("same", "same", "other", "shard"))
        w, h = (self.w, self.h) if which != "other" else SHAPES[SHAPES[0] == (self.w, self.h)]
        off, stride = (1, 2) if which == "shard" else (0, 1)
        rc = self.lib.rt_init_rand(self.ctx, w, h, off, stride)
        if rc == 0:
            self.w, self.h, self.rows = w, h, self.lib.rt_shard_rows(h, off, stride)
            self.restarted = False
        return rc, {}

    def state(self):
        if not self.rows:
            return self.lib.rt_get_state(self.ctx, None, None), {}
        rng, acc = self.r.get_state(self.rows, self.w)
        fc = self.pick((self.lib.rt_frame_counter(self.ctx), 1, 5))
        rc = self.lib.rt_set_state(self.ctx, rng.ctypes.data, acc.ctypes.data, fc)
        if rc == 0:
            self.restarted = False
        return rc, {}

    def temporal_reset(self):
        return self.lib.rt_temporal_reset(self.ctx), {}

    def last_stats(self):
        st = abi.AdaptiveStats()
        rc = self.lib.rt_adaptive_last_stats(self.ctx, C.byref(st))
        return rc, {"stats": [st.selected, st.frames_total]} if rc == 0 else {}

    # -- the recorder ----------------------------------------------------------
    def observe(self):
        lib, ctx = self.lib, self.ctx
        rec = {"frame": lib.rt_frame_counter(ctx), "moments": lib.rt_get_moments(ctx),
               "batches": lib.rt_moments_batches(ctx), "filters": lib.rt_get_adaptive_filters(ctx)}
        npix = max(self.rows, 1) * self.w
        n, j = np.zeros(npix, np.uint32), np.zeros(npix, np.uint32)
        rec["counts"] = [lib.rt_get_counts(ctx, n.ctypes.data, j.ctypes.data)]
        if rec["counts"][0] == 0:
            rec["counts"] += [int(x) for a in (n, j) for x in (a.min(), a.max(), a.sum())]
        rng, acc = np.zeros(6 * npix, np.uint32), np.zeros(3 * npix, np.float32)
        rec["state"] = [lib.rt_get_state(ctx, rng.ctypes.data, acc.ctypes.data)]
        if rec["state"][0] == 0:
            rec["state"].append(digest(rng, acc))
        var, lum = np.zeros(npix, np.float32), np.zeros(npix, np.float32)
        rec["var"] = [lib.rt_get_variance(ctx, var.ctypes.data, lum.ctypes.data)]
        if rec["var"][0] == 0:
            rec["var"].append(digest(var, lum))
        return rec

    def step(self):
        kind = self.kind()
        if kind == "adaptive" and self.restarted:
            kind = "render"
        rc, extra = getattr(self, kind)()
        rec = {"kind": kind, "status": rc}
        if rc < 0:
            msg = self.lib.rt_last_error(self.ctx).decode()
            rec["why"] = next((k for k in REASONS if k in msg), "")
        rec.update(extra)
        rec.update(self.observe())
        return rec


def trace(lib, seed, steps=STEPS, threads=0, gpu=False):
    """The records of one seed's sequence on a fresh context of `lib`: a CPU
    context on `threads` threads, or (gpu) a context of device 0."""
    with (Renderer(0, lib=lib) if gpu else Renderer.cpu(threads, lib=lib)) as r:
        t = Tracer(r, seed)
        assert lib.rt_set_scene(r.ctx, C.byref(t.scenes[0].struct)) == 0
        return [t.step() for _ in range(steps)]


def traces(lib, **kw):
    return {str(seed): trace(lib, seed, **kw) for seed in SEEDS}


def coverage(recording):
    """The figures the committed recording has to meet (test_lifecycle_trace)."""
    ok, refused = {}, {}
    records = unequal = drops = 0
    for recs in recording.values():
        prev = None
        for r in recs:
            records += 1
            c = r["counts"]
            unequal += c[0] == 0 and c[1] != c[2]
            if r["status"] >= 0:
                ok[r["kind"]] = ok.get(r["kind"], 0) + 1
            else:
                key = (r["kind"], r["why"])
                refused[key] = refused.get(key, 0) + 1
            # a successful render with the switch on that ends a live tracking:
            # its first frame was not the next one
            drops += (r["kind"] == "render" and r["status"] == 0 and r["moments"] == 1 and r["batches"] == 0 and
                      prev is not None and prev["batches"] > 0 and prev["moments"] == 1)
            prev = r
    return {"records": records, "unequal": unequal, "drops": drops, "ok": ok, "refused": refused}


if __name__ == "__main__":
    rec = traces(abi.load(), threads=2)
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(rec, f, separators=(",", ":"))
            f.write("\n")
    cov = coverage(rec)
    cov["refused"] = {"/".join(key): n for key, n in cov["refused"].items()}
    print(json.dumps(cov, indent=1))
