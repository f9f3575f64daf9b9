#!/usr/bin/env python3
"""Quality of rt_temporal_var on a moving camera, CPU backend:
    python tools/temporal_var_sweep.py [--threads N] [--out profiles/temporal_var/sweep.txt]

The two cases of tools/temporal_sweep.py (scene 07, 160x90, 4 bounces; `walk`: 8
views of 2 frames each; `pair`: 4 frames at view A, a small yaw, 4 frames at
view B), on the scene and on its twin with every emittance times 2^-4.  The
last view against a 1024-frame render of it.  Columns per case and scene: the
raw frame, rt_temporal, rt_temporal + rt_denoise with its defaults,
rt_temporal_var unfiltered (its colour is rt_temporal's), and rt_temporal_var
with five variance-guided levels over sigma_lum x min_batches (tracking off: one
render call per view, the interactive case).  Errors: mean |luminance error| of
the linear colour divided by the scene's factor (so both scenes read on one
scale), and the mean absolute error of the RGBA8 image.  Also the share of hit
pixels whose input variance is the temporal one, and the mean of the returned
variance of the mean (pixels with dof > 0) against the mean squared luminance
error of those pixels: how far signal change between views inflates it.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "bwidman-raytracer_amd"), os.path.join(REPO, "tools")]

from temporal_sweep import BOUNCES, H, TRUTH_FRAMES, VIEW_A, W, WALK, YAW, moved  # noqa: E402

SIGMA_LUM = (4.0, 8.0, 16.0, 32.0, 64.0)
MIN_BATCHES = (2, 4, 8)
LUM = np.array([0.2126, 0.7152, 0.0722])


def dim_scene(factor):
    from bwrt import scenes
    scene = scenes.scene_07()
    for i in range(scene.counts[0]):
        scene.spheres[i].mat.emittance *= factor
    return scene


class Case:
    """A camera path on one scene with the recorded state of every view."""

    def __init__(self, factor, moves, frames, threads):
        from bwrt import Renderer
        scene = dim_scene(factor)
        self.factor, self.frames = factor, frames
        self.cams = [moved(scene.camera, **VIEW_A)]
        for m in moves:
            self.cams.append(moved(self.cams[-1], **m))
        with Renderer.cpu(threads) as t:
            t.set_scene(scene)
            t.set_camera(self.cams[-1])
            self.truth_rgba = t.render(W, H, TRUTH_FRAMES, BOUNCES, first_frame=1)
            self.truth = t.get_state(H, W)[1].astype(np.float64) / TRUTH_FRAMES
        self.r = Renderer.cpu(threads)
        self.r.set_scene(scene)
        self.states = []
        for cam in self.cams:
            self.r.set_camera(cam)
            self.raw_rgba = self.r.render(W, H, frames, BOUNCES)
            self.states.append(self.r.get_state(H, W))
        self.raw = self.states[-1][1] / np.float32(frames)
        self.hit = self.r.render_aov(W, H)["prim"] >= 0

    def replay(self, last):
        """Every view's state again; `last(r)` is the call of the last view, the others are unfiltered."""
        r = self.r
        r.temporal_reset()
        for cam, (rng, acc) in zip(self.cams[:-1], self.states[:-1]):
            r.set_camera(cam)
            r.set_state(rng, acc, self.frames + 1)
            r.temporal_var(W, H)
        r.set_camera(self.cams[-1])
        r.set_state(*self.states[-1], self.frames + 1)
        return last(r)

    def errors(self, rgba, col):
        e_lum = float(np.abs((col.astype(np.float64) - self.truth) @ LUM).mean()) / self.factor
        e_rgba = float(np.abs(rgba[..., :3].astype(np.int32) - self.truth_rgba[..., :3].astype(np.int32)).mean())
        return e_lum, e_rgba


def report(name, case, lines):
    fmt = lambda e: f"{e[0]:.5f}  {e[1]:7.3f}"  # noqa: E731
    lines.append(f"{name}, emittance x {case.factor:g}: {len(case.cams)} views x {case.frames} frames "
                 f"(luminance error / factor, RGBA8 error)")
    lines.append(f"  raw last view                         {fmt(case.errors(case.raw_rgba, case.raw))}")
    t = case.replay(lambda r: r.temporal(W, H, want_color=True))
    lines.append(f"  rt_temporal                           {fmt(case.errors(*t))}")
    td = case.replay(lambda r: r.temporal(W, H, denoise={}, want_color=True))
    lines.append(f"  rt_temporal + rt_denoise (defaults)   {fmt(case.errors(*td))}")
    rgba, col, ln, mom = case.replay(lambda r: r.temporal_var(W, H, want_color=True, want_length=True,
                                                              want_moments=True))
    lines.append(f"  rt_temporal_var, unfiltered           {fmt(case.errors(rgba, col))}")
    known = mom[..., 1] > 0
    sq = ((col.astype(np.float64) - case.truth) @ LUM) ** 2
    lines.append(f"    returned variance of the mean, mean over the {known.mean():.3f} of pixels with dof > 0: "
                 f"{mom[..., 0][known].mean() / case.factor ** 2:.5f}; their mean squared luminance error: "
                 f"{sq[known].mean() / case.factor ** 2:.5f} (both / factor^2)")
    d = case.r.denoise_var_params()
    rows = []
    for mb in MIN_BATCHES:
        share = float((mom[..., 1][case.hit] >= mb - 1.5).mean())
        for sl in SIGMA_LUM:
            f = case.replay(lambda r: r.temporal_var(W, H, denoise_var={"sigma_lum": sl, "min_batches": mb},
                                                     want_color=True))
            rows.append((case.errors(*f), sl, mb, share))
    for e, sl, mb, share in sorted(rows):
        tag = "  <- rt_denoise_var_params_default()" if (sl, mb) == (d.sigma_lum, d.min_batches) else ""
        lines.append(f"  + {d.iterations} levels, sigma_lum {sl:4.0f} min_batches {mb} (temporal source on {share:.3f} "
                     f"of the hit pixels)  {fmt(e)}{tag}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    for name, moves, frames in (("walk", WALK, 2), ("pair", [YAW], 4)):
        for factor in (1.0, 0.0625):
            report(name, Case(factor, moves, frames, args.threads), lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
