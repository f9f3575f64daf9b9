"""Seeded sequences of C ABI calls on one context that move it from view to
view, and what the context reports after every call: the status, what a
refusal was about, the images and planes of the temporal calls, the filters
and the adaptive calls, rt_assembled() with its n and J, and the frame counter.
No times are recorded, so a recording depends on the library alone:
tests/golden/view_trace.json is the recording of the library before the
view-bound host state got its one owner (csrc/rt_view.h) -- it was written
before csrc/ was touched -- and every later library has to reproduce it
(tests/test_view_trace.py), on the GPU as on the CPU (tests/test_gpu_adaptive.py).

    python tests/view_trace.py            the recording's coverage figures
    python tests/view_trace.py --write    rewrite the golden from $BWRT_LIB

The sequences are tests/lifecycle_trace.py's in shape (its digest, its Tracer,
its rule about adaptive calls after a restart) over other step kinds: here the
views, the two temporal history sets and the assembled frame of a shard
context are what the steps exercise.  Moment tracking is on throughout.

A temporal call's length plane holds, without usable history, the frame's own
count n (n_p on a non-uniform frame) and len_h + n with one (csrc/rt_temporal.h),
so "a history length of 1 everywhere" is the one-frame case of "the length is
the own count everywhere".  Every temporal record therefore carries `hist`, the
minimum and maximum of length - own count: [0, 0] is a call that found no
history, a maximum above 0 one that used it.  The coverage counts a promotion
by a maximum above 0 (then the length is above 1) and a dropped history twice:
by hist == [0, 0], and, of those, by a length of 1 everywhere; a fresh
accumulation's first render often takes one sample so that the latter occur.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lifecycle_trace as L  # noqa: E402
from lifecycle_trace import BOUNCES, SEEDS, SHAPES, digest  # noqa: E402,F401
from bwrt import Renderer, abi  # noqa: E402

STEPS = 300
SHARD = (1, 2)  # row offset and stride of the shard context
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "view_trace.json")

# step kinds and their weights, tuned until the recording meets
# test_the_recording_covers_the_views: the temporal calls dominate, so that every
# way of losing a history is followed by one; rt_temporal_var and the adaptive
# call that reads its pending planes are raised so that the three meet in one
# view; the camera moves outweigh what drops a history, so that promotions occur
WEIGHTS = (("render", 22), ("temporal", 9), ("temporal_var", 22), ("temporal_var_counted", 11), ("denoise", 2),
           ("denoise_var", 3), ("adaptive_reprojected", 15), ("adaptive", 10), ("set_scene", 4), ("set_camera", 7),
           ("controls", 7), ("reset", 3), ("init_rand", 6), ("temporal_reset", 4), ("set_filters", 1),
           ("assemble", 8), ("assemble_adaptive", 5), ("assemble_drop", 1))

# what a refusal was about: the first of these found in rt_last_error
REASONS = ("no pending temporal set", "has no moments", "is stale", "row shard", "non-uniform",
           "no frame accumulated yet", "no assembled frame", "not live", "at least 2 batches", "at least 1 batch")

TEMPORAL = ("temporal", "temporal_var", "temporal_var_counted")
FILTERS = TEMPORAL + ("denoise", "denoise_var")


class Tracer(L.Tracer):
    """lifecycle_trace's context and generator with the steps of this module;
    denoise, denoise_var, adaptive, set_filters, set_scene, reset and
    temporal_reset are its own."""

    def __init__(self, renderer, seed):
        super().__init__(renderer, seed)
        self.shard = (0, 1)   # row offset and stride of the pixel state
        self.view = 0         # the generator's count of the context's views
        self.as_n = None      # n_p of the last assembly (None: it carried one count)

    def kind(self):
        x = self.rnd.random() * sum(w for _, w in WEIGHTS)
        for name, w in WEIGHTS:
            x -= w
            if x < 0:
                return name
        return WEIGHTS[-1][0]

    def sharded(self):
        return self.shard != (0, 1)

    # -- steps: each returns (status, extras of the record) --------------------
    def render(self):
        w, h = SHAPES[SHAPES[0] == (self.w, self.h)] if self.rnd.random() < 0.06 else (self.w, self.h)
        fc = self.lib.rt_frame_counter(self.ctx)
        first = self.pick((0,) * 8 + (1, fc, fc + 2))
        # (a fresh accumulation often gets one frame: a temporal call that finds no
        # history there returns the length 1 everywhere)
        p = abi.RenderParams(w, h, self.pick((1, 1, 1, 2, 3) if fc == 1 else (1, 2, 3)), BOUNCES, first, *self.shard)
        if (w, h) != (self.w, self.h) or not self.rows:
            self.view += 1  # (the implicit rt_init_rand comes before any refusal)
        rc = self.lib.rt_render_ex(self.ctx, C.byref(p), None, None)
        self.w, self.h, self.rows = w, h, self.lib.rt_shard_rows(h, *self.shard)
        if rc == 0:
            self.restarted = False
        return rc, {}

    def own_counts(self):
        """The frames behind every pixel of the frame a full-frame pass reads."""
        n, j = C.c_uint(), C.c_uint()
        if self.sharded() and self.lib.rt_assembled(self.ctx, C.byref(n), C.byref(j)):
            return self.as_n if self.as_n is not None else np.float32(n.value)
        cn = np.zeros((self.h, self.w), np.uint32)
        assert self.lib.rt_get_counts(self.ctx, cn.ctypes.data, None) == 0
        return cn

    def _temporal(self, call, mom=None):
        rgba = np.zeros((self.h, self.w, 4), np.uint8)
        ln = np.zeros((self.h, self.w), np.float32)
        rc = call(rgba.ctypes.data, ln.ctypes.data)
        if rc:
            return rc, {}
        hist = ln - self.own_counts()
        rec = {"rgba": digest(rgba), "length": digest(ln), "len": [float(ln.min()), float(ln.max())],
               "hist": [float(hist.min()), float(hist.max())]}
        if mom is not None:
            rec["moments"] = digest(mom)
        return rc, rec

    def temporal(self):
        t = self.r.temporal_params()
        d = C.byref(self.r.denoise_params(iterations=1)) if self.rnd.random() < 0.5 else None
        return self._temporal(lambda out, ln: self.lib.rt_temporal(self.ctx, C.byref(t), d, out, None, ln))

    def _temporal_var(self, fn):
        t = self.r.temporal_params()
        d = (C.byref(self.r.denoise_var_params(iterations=1, min_batches=self.pick((2, 4))))
             if self.rnd.random() < 0.3 else None)
        mom = np.zeros((self.h, self.w, 2), np.float32)
        return self._temporal(lambda out, ln: fn(self.ctx, C.byref(t), d, out, None, ln, mom.ctypes.data), mom)

    def temporal_var(self):
        return self._temporal_var(self.lib.rt_temporal_var)

    def temporal_var_counted(self):
        return self._temporal_var(self.lib.rt_temporal_var_counted)

    def adaptive_reprojected(self):
        d = self.r.adaptive_reprojected_params(samples=self.pick((1, 2)), min_frames=self.pick((0, 0, 100)))
        st = abi.AdaptiveStats()
        rc = self.lib.rt_render_adaptive_reprojected(self.ctx, C.byref(d), BOUNCES, None, None, C.byref(st))
        return rc, {"stats": [st.selected, st.frames_total]} if rc == 0 else {}

    def set_scene(self):
        rc, extra = super().set_scene()
        self.view += rc == 0
        return rc, extra

    def set_camera(self):
        self.view += 1
        return super().set_camera()

    def controls(self):
        flags, extra = super().controls()
        self.view += bool(flags > 0 and flags & abi.CONTROLS_MOVED)
        return flags, extra

    def init_rand(self):
        which = self.pick(("same", "other", "shard"))
        w, h = (self.w, self.h) if which != "other" else SHAPES[SHAPES[0] == (self.w, self.h)]
        shard = SHARD if which == "shard" else (0, 1)
        rc = self.lib.rt_init_rand(self.ctx, w, h, *shard)
        if rc == 0:
            self.w, self.h, self.shard, self.rows = w, h, shard, self.lib.rt_shard_rows(h, *shard)
            self.restarted = False
            self.view += 1
        return rc, {}

    def _assemble(self, fn, planes, counted):
        """Seeded synthetic blocks of the context's shape: the assembly does not
        care where they came from.  Count planes hold uint32 words."""
        shards = SHARD[1]
        rps = (self.h + shards - 1) // shards
        rs = np.random.RandomState(self.rnd.getrandbits(32))
        g = (4.0 * rs.random_sample((shards, planes, rps, self.w))).astype(np.float32)
        as_n = None
        if counted:
            n_p = rs.randint(1, 6, (shards, rps, self.w)).astype(np.uint32)
            g[:, -1 if planes == 4 else -2] = n_p.view(np.float32)
            if planes == 7:
                g[:, -1] = np.minimum(n_p, rs.randint(1, 4, n_p.shape).astype(np.uint32)).view(np.float32)
            as_n = np.stack([n_p[y % shards, y // shards] for y in range(self.h)])
        frames, batches = self.pick((1, 2, 3, 5)), self.pick((0, 1, 2, 4))
        rc = fn(self.ctx, g.ctypes.data, shards, rps, planes, frames, batches)
        if rc == 0:
            self.as_n = as_n
        return rc, {}

    def assemble(self):
        return self._assemble(self.lib.rt_assemble, self.pick((3, 5)), False)

    def assemble_adaptive(self):
        return self._assemble(self.lib.rt_assemble_adaptive, self.pick((4, 7)), True)

    def assemble_drop(self):
        return self.lib.rt_assemble_drop(self.ctx), {}

    # -- the recorder ----------------------------------------------------------
    def observe(self):
        n, j = C.c_uint(), C.c_uint()
        made = self.lib.rt_assembled(self.ctx, C.byref(n), C.byref(j))
        return {"frame": self.lib.rt_frame_counter(self.ctx), "assembled": [made, n.value, j.value] if made else [0],
                # the generator's own state, for the coverage figures
                "view": self.view, "shape": [self.w, self.h], "shard": int(self.sharded())}

    def step(self):
        kind = self.kind()
        if kind in ("adaptive", "adaptive_reprojected") and self.restarted:
            kind = "render"
        if kind in ("assemble", "assemble_adaptive") and not self.sharded():
            kind = "render"  # the host forms are taken on a shard context only
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
        assert lib.rt_set_moments(r.ctx, 1) == 0
        return [t.step() for _ in range(steps)]


def traces(lib, **kw):
    return {str(seed): trace(lib, seed, **kw) for seed in SEEDS}


def coverage(recording):
    """The figures the committed recording has to meet (test_view_trace)."""
    ok, refused = {}, {}
    cov = {"records": 0, "promotions": 0, "drops": {"scene": 0, "init_rand": 0, "render": 0, "temporal_reset": 0},
           "drops_length_1": {"scene": 0, "init_rand": 0, "render": 0, "temporal_reset": 0},
           "var_on_plain_history": 0, "plain_on_var_history": 0,
           "shard_filter_ok": 0, "shard_filter_ok_counted": 0, "assembled": set(), "assembled_lost_after": set()}
    for recs in recording.values():
        prev = None      # the record before
        last = None      # the last successful temporal step: the writer of the pending result
        causes = set()   # what dropped the history since
        counted = False  # the assembled frame carries counts
        for r in recs:
            cov["records"] += 1
            kind, good = r["kind"], r["status"] >= 0
            if good:
                ok[kind] = ok.get(kind, 0) + 1
            else:
                key = (kind, r["why"])
                refused[key] = refused.get(key, 0) + 1
            reshaped = prev is not None and r["shape"] != prev["shape"]
            if kind == "set_scene" and good:
                causes.add("scene")
            if kind in ("init_rand", "render") and reshaped:
                causes.add(kind)
            if kind == "temporal_reset":
                causes.add(kind)
            if kind in ("assemble", "assemble_adaptive") and good:
                counted = kind == "assemble_adaptive"
            if kind in TEMPORAL and good:
                if last is not None and r["view"] != last["view"]:
                    if r["hist"][1] > 0:
                        assert r["len"][1] > 1
                        cov["promotions"] += 1
                        cov["var_on_plain_history"] += kind != "temporal" and last["kind"] == "temporal"
                        cov["plain_on_var_history"] += kind == "temporal" and last["kind"] != "temporal"
                    elif r["hist"] == [0, 0] and len(causes) == 1:
                        cov["drops"][next(iter(causes))] += 1
                        cov["drops_length_1"][next(iter(causes))] += r["len"] == [1, 1]
                last, causes = r, set()
            if kind in FILTERS and good and r["shard"]:
                assert r["assembled"][0] == 1
                cov["shard_filter_ok"] += 1
                cov["shard_filter_ok_counted"] += counted
            cov["assembled"].add(r["assembled"][0])
            if prev is not None and prev["assembled"][0] == 1 and r["assembled"][0] == 0:
                moved = kind == "controls" and r["view"] != prev["view"]
                cov["assembled_lost_after"].add("reshape" if reshaped else "controls_moved" if moved else kind)
            prev = r
    cov["assembled"] = sorted(cov["assembled"])
    cov["assembled_lost_after"] = sorted(cov["assembled_lost_after"])
    cov["shard_filter_refused"] = {why: sum(n for (k, w), n in refused.items() if k in FILTERS and w == why)
                                   for why in ("is stale", "row shard")}
    cov.update(ok=ok, refused=refused)
    return cov


if __name__ == "__main__":
    rec = traces(abi.load(), threads=2)
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(rec, f, separators=(",", ":"))
            f.write("\n")
    cov = coverage(rec)
    cov["refused"] = {"/".join(key): n for key, n in cov["refused"].items()}
    print(json.dumps(cov, indent=1))
