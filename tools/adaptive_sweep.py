#!/usr/bin/env python3
"""Parameter sweep of the adaptive sampling on the CPU backend (bit-identical to
the GPU): tools/adaptive_sweep.py [--out profiles/adaptive/sweep.txt] [--budget 32]

Scene 07 at 160x90, 4 bounces, and its twin under a sky (background 0.25, 0.35,
0.5).  Start: 4 calls x 2 frames with tracking on; then rounds of
rt_render_adaptive (8 frames per selected pixel) until the mean frame count per
pixel reaches the budget.  Error: mean absolute error of the RGBA in 8-bit
units against a 2048-frame render.  For each grid point (radius, tolerance,
floor) the sweep reports the mean count reached, its MAE, the frames a uniform
render needs for that MAE (interpolated on uniform renders of 8, 16, .. frames,
linear in log frames against log MAE) and the ratio mean count / uniform
frames: the share of the samples the adaptive render needs for equal error
(below 1: adaptive ahead).  rt_adaptive_params_default() holds the chosen point.
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd")]
from bwrt import Renderer, scenes  # noqa: E402

W, H, BOUNCES, TRUTH = 160, 90, 4, 2048
SKY = (0.25, 0.35, 0.5)
RADII = (0, 1, 2, 3, 4)
TOLERANCES = (0.05, 0.1, 0.2)
FLOORS = (0.0, 0.01, 0.05)


def mae(a, b):
    return float(np.abs(a[..., :3].astype(np.int32) - b[..., :3].astype(np.int32)).mean())


def uniform_curve(r, upto):
    """[(frames, RGBA)] at 8, 16, .. and the TRUTH-frame render."""
    pts = []
    for f in range(8, upto + 1, 8):
        pts.append((f, r.render(W, H, 8, BOUNCES, first_frame=1 if f == 8 else 0)))
    truth = r.render(W, H, TRUTH - upto, BOUNCES)
    return pts, truth


def frames_for(curve, err):
    """Uniform frames with MAE `err`, interpolated in log-log."""
    for (f0, e0), (f1, e1) in zip(curve, curve[1:]):
        if e1 <= err <= e0:
            t = (math.log(e0) - math.log(err)) / (math.log(e0) - math.log(e1)) if e0 > e1 else 0.0
            return math.exp(math.log(f0) + t * (math.log(f1) - math.log(f0)))
    return float("nan")


def adaptive(r, budget, **params):
    for i in range(4):
        r.render(W, H, 2, BOUNCES, first_frame=1 if i == 0 else 0)
    mean, img, rounds = 8.0, None, 0
    while mean < budget and rounds < 64:
        img, st = r.render_adaptive(W, H, BOUNCES, samples=8, **params)
        mean = st["frames_total"] / (W * H)
        rounds += 1
        if st["selected"] == 0:
            break
    return mean, img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--budget", type=float, default=32.0)
    args = ap.parse_args()
    lines = [f"scene 07 {W}x{H}, {BOUNCES} bounces, start 4 x 2 frames, rounds of 8 to a mean of {args.budget:g} "
             f"frames per pixel; MAE in 8-bit units against {TRUTH} frames"]
    best = {}
    with Renderer.cpu(0) as r:
        r.set_scene(scenes.scene_07())
        for case, bg in (("07", (0.0, 0.0, 0.0)), ("07 under a sky", SKY)):
            r.set_background(*bg)
            r.set_moments(False)
            pts, truth = uniform_curve(r, 128)
            curve = [(f, mae(img, truth)) for f, img in pts]
            lines.append(f"--- {case}: uniform MAE " + ", ".join(f"{f}: {e:.2f}" for f, e in curve))
            r.set_moments(True)
            lines.append("radius tolerance floor   mean frames   MAE    uniform frames   share")
            for radius in RADII:
                for tol in TOLERANCES:
                    for floor in FLOORS:
                        mean, img = adaptive(r, args.budget, radius=radius, tolerance=tol, lum_floor=floor)
                        e = mae(img, truth)
                        uf = frames_for(curve, e)
                        share = mean / uf
                        best.setdefault((radius, tol, floor), []).append(share)
                        lines.append(f"{radius:6d} {tol:9.2f} {floor:5.2f}   {mean:11.2f}   {e:5.2f}   {uf:14.1f}   "
                                     f"{share:.3f}{'  (budget not reached)' if mean < args.budget else ''}")
    d = Renderer.cpu(1)
    p = d.adaptive_params()
    d.close()
    ranked = sorted((max(v) if not any(math.isnan(x) for x in v) else float("inf"), k) for k, v in best.items())
    lines.append("--- worst share over both cases, best five: " +
                 "; ".join(f"r{k[0]} tol {k[1]} floor {k[2]}: {s:.3f}" for s, k in ranked[:5]))
    dk = (p.radius, round(p.tolerance, 4), round(p.lum_floor, 4))
    lines.append(f"defaults: radius {p.radius}, tolerance {p.tolerance:.3g}, floor {p.lum_floor:.3g}: shares " +
                 ", ".join(f"{x:.3f}" for x in best.get(dk, [])))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
