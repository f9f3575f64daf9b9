#!/usr/bin/env python3
"""Grid search of the temporal reprojection's defaults (rt_temporal_params_default).

CPU backend (bit-identical to the GPU), scene 07 at 160x90, 4 bounces, two
cases:

  walk   a camera that keeps moving: 8 views, 2 frames each, a small yaw /
         sideways / dolly step between them, one rt_temporal call per view;
  pair   the case of tests/test_temporal.py's quality test: 4 frames at view
         A, one yaw step, 4 frames at view B.

Every view is rendered once and its state (RNG, frameSum) recorded; a
parameter set replays the states through rt_set_state, so all sets see the
same samples.  The error of a set is the mean absolute RGB difference (8-bit
units) between the last view's temporal RGBA and a 1024-frame render of that
view.  Prints the grid of the walk sorted by error, the raw frame's error, and
the defaults on both cases, also with the default spatial filter on top;
DESIGN.md section 10 records the result.

    python tools/temporal_sweep.py [--threads N]
"""
import argparse
import ctypes as C
import itertools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bwidman-raytracer_amd"))

W, H, BOUNCES, TRUTH_FRAMES = 160, 90, 4, 1024
VIEW_A = dict(dx=0.1, dy=0.2, dz=0.3, dyaw=0.05, dpitch=-0.08)
YAW = dict(dyaw=0.037, dpitch=0.011)
WALK = [YAW, dict(dx=0.15, dy=0.02), dict(dz=-0.15, dx=0.01), YAW, dict(dx=-0.1, dyaw=-0.03), dict(dz=-0.1),
        dict(dyaw=0.025, dpitch=-0.01)]
MAX_HISTORY = (2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 256.0)
NORMAL_COS = (0.0, 0.5, 0.8, 0.9, 0.97, 0.995)
PLANE_TOL = (0.002, 0.005, 0.01, 0.02, 0.05, 0.2, 1.0)


def moved(c, dx=0.0, dy=0.0, dz=0.0, dyaw=0.0, dpitch=0.0):
    from bwrt import scenes
    from bwrt.abi import Camera
    return Camera(scenes.vec(c.position.x + dx, c.position.y + dy, c.position.z + dz),
                  (C.c_float * 2)(c.angle[0] + dyaw, c.angle[1] + dpitch), c.fov)


def mae(a, b):
    return float(np.abs(a[..., :3].astype(np.int32) - b[..., :3].astype(np.int32)).mean())


class Case:
    """A camera path with the recorded state of every view."""

    def __init__(self, moves, frames, threads=0):
        from bwrt import Renderer, scenes
        scene = scenes.scene_07()
        cams = [moved(scene.camera, **VIEW_A)]
        for m in moves:
            cams.append(moved(cams[-1], **m))
        self.cams, self.frames = cams, frames
        with Renderer.cpu(threads) as t:
            t.set_scene(scene)
            t.set_camera(cams[-1])
            self.truth = t.render(W, H, TRUTH_FRAMES, BOUNCES, first_frame=1)
        self.r = Renderer.cpu(threads)
        self.r.set_scene(scene)
        self.states = []
        for cam in cams:
            self.r.set_camera(cam)
            self.raw = self.r.render(W, H, frames, BOUNCES)
            self.states.append(self.r.get_state(H, W))

    def replay(self, denoise=None, **tp):
        """The last view's temporal RGBA for one parameter set."""
        r = self.r
        r.temporal_reset()
        for i, (cam, (rng, acc)) in enumerate(zip(self.cams, self.states)):
            r.set_camera(cam)
            r.set_state(rng, acc, self.frames + 1)
            out = r.temporal(W, H, denoise=denoise if i == len(self.cams) - 1 else None, **tp)
        return out

    def denoised(self):
        r = self.r
        r.set_camera(self.cams[-1])
        r.set_state(*self.states[-1], self.frames + 1)
        return r.denoise(W, H)


def report_defaults(name, case):
    raw, truth = case.raw, case.truth
    e_raw, e_t = mae(raw, truth), mae(case.replay(), truth)
    e_d, e_td = mae(case.denoised(), truth), mae(case.replay(denoise={}), truth)
    print(f"{name}: raw {e_raw:.4f}  temporal {e_t:.4f} (ratio {e_t / e_raw:.3f})  denoise {e_d:.4f}  "
          f"temporal + denoise {e_td:.4f} (ratio to denoise {e_td / e_d:.3f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=0)
    args = ap.parse_args()
    walk = Case(WALK, 2, args.threads)
    rows = []
    for mh, nc, pt in itertools.product(MAX_HISTORY, NORMAL_COS, PLANE_TOL):
        rows.append((mae(walk.replay(max_history=mh, normal_cos_min=nc, plane_tol=pt), walk.truth), mh, nc, pt))
    rows.sort()
    print(f"walk: {len(walk.cams)} views x {walk.frames} frames; raw last view: mean |error| {mae(walk.raw, walk.truth):.4f}")
    print("error    max_history normal_cos_min plane_tol")
    for e, mh, nc, pt in rows[:12] + rows[-3:]:
        print(f"{e:.4f}  {mh:<11g} {nc:<14g} {pt:g}")
    d = walk.r.lib.rt_temporal_params_default()
    print("one parameter at a time around the defaults:")
    for name, values in (("max_history", MAX_HISTORY), ("normal_cos_min", NORMAL_COS), ("plane_tol", PLANE_TOL)):
        errs = [mae(walk.replay(**{name: v}), walk.truth) for v in values]
        print(f"  {name}: " + "  ".join(f"{v:g}: {e:.3f}" for v, e in zip(values, errs)))
    print(f"defaults (max_history {d.max_history:g}, normal_cos_min {d.normal_cos_min:g}, plane_tol {d.plane_tol:g}):")
    report_defaults("  walk", walk)
    report_defaults("  pair", Case([YAW], 4, args.threads))


if __name__ == "__main__":
    main()
