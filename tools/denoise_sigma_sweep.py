#!/usr/bin/env python3
"""Grid search of the denoiser's default sigmas (rt_denoise_params_default).

CPU backend (bit-identical to the GPU): scene 07 at 160x90, 8 frames, 4
bounces, 5 a-trous levels; the error of a parameter set is the mean absolute
RGB difference (8-bit units) between the denoised RGBA and a 2048-frame render
of the same view.  Prints the grid sorted by error, the raw frame's error and
the best set; DESIGN.md ("Denoiser") records the result.

    python tools/denoise_sigma_sweep.py [--threads N]
"""
import argparse
import itertools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bwidman-raytracer_amd"))

W, H, FRAMES, BOUNCES, TRUTH_FRAMES, LEVELS = 160, 90, 8, 4, 2048, 5
SIGMA_COLOR = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0)
SIGMA_NORMAL = (0.0625, 0.125, 0.25, 0.5, 1.0)
SIGMA_PLANE = (0.025, 0.05, 0.1, 0.2, 0.4, 0.8, 1.6, 3.2)


def mae(a, b):
    return float(np.abs(a[..., :3].astype(np.int32) - b[..., :3].astype(np.int32)).mean())


def case(threads=0):
    """(renderer holding the 8-frame state, its raw RGBA, the 2048-frame RGBA)."""
    from bwrt import Renderer, scenes
    scene = scenes.scene_07()
    with Renderer.cpu(threads) as t:
        t.set_scene(scene)
        truth = t.render(W, H, TRUTH_FRAMES, BOUNCES, first_frame=1)
    r = Renderer.cpu(threads)
    r.set_scene(scene)
    raw = r.render(W, H, FRAMES, BOUNCES, first_frame=1)
    return r, raw, truth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=0)
    args = ap.parse_args()
    r, raw, truth = case(args.threads)
    rows = []
    for sc, sn, sp in itertools.product(SIGMA_COLOR, SIGMA_NORMAL, SIGMA_PLANE):
        out = r.denoise(W, H, iterations=LEVELS, sigma_color=sc, sigma_normal=sn, sigma_plane=sp)
        rows.append((mae(out, truth), sc, sn, sp))
    rows.sort()
    print(f"raw {FRAMES}-frame RGBA: mean |error| {mae(raw, truth):.4f}")
    print("error   sigma_color sigma_normal sigma_plane")
    for e, sc, sn, sp in rows[:12] + rows[-3:]:
        print(f"{e:.4f}  {sc:<11g} {sn:<12g} {sp:g}")
    d = r.lib.rt_denoise_params_default()
    out = r.denoise(W, H)
    print(f"defaults ({d.iterations} levels, {d.sigma_color:g}, {d.sigma_normal:g}, {d.sigma_plane:g}): "
          f"{mae(out, truth):.4f}  ratio to raw {mae(out, truth) / mae(raw, truth):.3f}")
    r.close()


if __name__ == "__main__":
    main()
