#!/usr/bin/env python3
"""What the filters make of an adaptive frame, on the CPU backend (bit-identical
to the GPU): tools/adaptive_post_sweep.py [--out profiles/adaptive_post/sweep.txt] [--budget 32]

The sweep case of tools/adaptive_sweep.py: scene 07 at 160x90, 4 bounces, and
its twin under a sky (background 0.25, 0.35, 0.5).  Start: 4 calls x 2 frames
with tracking on; then rounds of rt_render_adaptive with the defaults until the
mean frame count per pixel reaches the budget, with rt_set_adaptive_filters on.
Error: mean absolute error of the RGBA in 8-bit units against a 2048-frame
render, for
  the raw adaptive frame, and it through rt_denoise and through rt_denoise_var
  (defaults; every pixel has at least 4 batches, so all variances are tracked);
  a uniform render at the nearest whole frame count, made as calls of 8 frames
  (and a last shorter one) so that its moments are tracked too, raw and through
  the same two filters.
"""
import argparse
import os
import sys

import numpy as np

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd")]
from bwrt import Renderer, scenes  # noqa: E402

W, H, BOUNCES, TRUTH = 160, 90, 4, 2048
SKY = (0.25, 0.35, 0.5)


def mae(a, b):
    return float(np.abs(a[..., :3].astype(np.int32) - b[..., :3].astype(np.int32)).mean())


def filtered(r):
    return r.denoise(W, H), r.denoise_var(W, H)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--budget", type=float, default=32.0)
    args = ap.parse_args()
    lines = [f"scene 07 {W}x{H}, {BOUNCES} bounces; adaptive: start 4 x 2 frames, rounds of the defaults to a mean of "
             f"{args.budget:g} frames per pixel; MAE in 8-bit units against {TRUTH} frames (ratio to the raw frame of "
             f"the same row)"]
    with Renderer.cpu(0) as r:
        r.set_scene(scenes.scene_07())
        r.set_adaptive_filters(True)
        for case, bg in (("07", (0.0, 0.0, 0.0)), ("07 under a sky", SKY)):
            r.set_background(*bg)
            r.set_moments(False)
            truth = r.render(W, H, TRUTH, BOUNCES, first_frame=1)
            r.set_moments(True)
            for i in range(4):
                r.render(W, H, 2, BOUNCES, first_frame=1 if i == 0 else 0)
            mean, raw = 8.0, None
            while mean < args.budget:
                raw, st = r.render_adaptive(W, H, BOUNCES)
                mean = st["frames_total"] / (W * H)
                if st["selected"] == 0:
                    break
            n, j = r.counts(H, W)
            rows = [(f"adaptive, mean {mean:.2f} frames (n_p {n.min()}..{n.max()}, J_p {j.min()}..{j.max()})",
                     (raw,) + filtered(r))]
            frames, done = int(round(mean)), 0
            while done < frames:
                k = min(8, frames - done)
                uni = r.render(W, H, k, BOUNCES, first_frame=1 if done == 0 else 0)
                done += k
            rows.append((f"uniform, {frames} frames ({r.moments_batches} batches)", (uni,) + filtered(r)))
            lines.append(f"--- {case}")
            lines.append(f"{'frame':58s} {'raw':>7s} {'rt_denoise':>16s} {'rt_denoise_var':>16s}")
            for name, imgs in rows:
                e = [mae(x, truth) for x in imgs]
                lines.append(f"{name:58s} {e[0]:7.2f} {e[1]:8.2f} ({e[1] / e[0]:.3f}) {e[2]:8.2f} ({e[2] / e[0]:.3f})")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
