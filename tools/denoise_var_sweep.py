#!/usr/bin/env python3
"""Grid search of the variance-guided filter's defaults
(rt_denoise_var_params_default) on the sweep case of the denoiser and on the
same scene with every emittance times 2^-4.

CPU backend (bit-identical to the GPU): scene 07 at 160x90, 8 frames as 8
render calls (8 tracked batches), 4 bounces, 5 a-trous levels; the error of a
parameter set is the mean absolute RGB difference (8-bit units) between the
filtered RGBA and a 2048-frame render of the same view.  min_batches at most 8
filters with the tracked variance, above 8 with the spatial estimate.  Prints,
per scene, the grid over sigma_lum x min_batches, the raw frame's error, the
defaults' and rt_denoise's with its default (fixed) sigma_color; DESIGN.md
section 11 records the result.

    python tools/denoise_var_sweep.py [--threads N]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bwidman-raytracer_amd"))

W, H, CALLS, BOUNCES, TRUTH_FRAMES, LEVELS = 160, 90, 8, 4, 2048, 5
SIGMA_LUM = (0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0)
MIN_BATCHES = (2, 4, 8, 9)  # 9: above the 8 tracked batches, i.e. the spatial estimate


def mae(a, b):
    return float(np.abs(a[..., :3].astype(np.int32) - b[..., :3].astype(np.int32)).mean())


def scene_scaled(factor):
    from bwrt import scenes
    scene = scenes.scene_07()
    for i in range(scene.counts[0]):
        scene.spheres[i].mat.emittance *= factor
    return scene


def case(scene, threads=0):
    """(renderer holding the 8-call tracked state, its raw RGBA, the 2048-frame RGBA)."""
    from bwrt import Renderer
    with Renderer.cpu(threads) as t:
        t.set_scene(scene)
        truth = t.render(W, H, TRUTH_FRAMES, BOUNCES, first_frame=1)
    r = Renderer.cpu(threads)
    r.set_scene(scene)
    r.set_moments(True)
    for i in range(CALLS):
        raw = r.render(W, H, 1, BOUNCES, first_frame=1 if i == 0 else 0)
    assert r.moments_batches == CALLS
    return r, raw, truth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=0)
    args = ap.parse_args()
    for name, factor in (("scene 07", 1.0), ("scene 07, emittances x 2^-4", 0.0625)):
        r, raw, truth = case(scene_scaled(factor), args.threads)
        e_raw = mae(raw, truth)
        print(f"{name}: raw {CALLS}-frame RGBA: mean |error| {e_raw:.4f}")
        print("sigma_lum  " + "  ".join(f"min_batches {m}{' (spatial)' if m > CALLS else ''}" for m in MIN_BATCHES))
        for sl in SIGMA_LUM:
            errs = [mae(r.denoise_var(W, H, iterations=LEVELS, sigma_lum=sl, min_batches=m), truth)
                    for m in MIN_BATCHES]
            print(f"{sl:<9g}  " + "  ".join(f"{e:<13.4f}" for e in errs))
        d = r.lib.rt_denoise_var_params_default()
        e_def = mae(r.denoise_var(W, H), truth)
        e_fix = mae(r.denoise(W, H), truth)
        print(f"defaults ({d.iterations} levels, sigma_lum {d.sigma_lum:g}, min_batches {d.min_batches}): {e_def:.4f}  "
              f"ratio to raw {e_def / e_raw:.3f}")
        print(f"rt_denoise with its defaults (sigma_color {r.lib.rt_denoise_params_default().sigma_color:g}): "
              f"{e_fix:.4f}  ratio to raw {e_fix / e_raw:.3f}; rt_denoise_var / rt_denoise {e_def / e_fix:.3f}")
        r.close()


if __name__ == "__main__":
    main()
