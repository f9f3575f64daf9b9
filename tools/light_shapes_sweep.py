#!/usr/bin/env python3
"""Error of next-event estimation with polygon lights (rt_set_light_shapes,
RT_LIGHT_SHAPES_ALL) against the default estimator and, on the Mixed scene,
against sphere-only NEE, at equal frames and at equal time, on the CPU backend
(bit-identical to the GPU): tools/light_shapes_sweep.py [--out FILE]

Three scenes at 160x90 with 4 bounces (tools/light_shapes_scenes.py): the quad
panel, the triangle panel and Mixed.  Truth: a 2048-frame ALL render (uniform
pick) on RNG streams of its own (every pixel starts on another pixel's
stream).  Error: mean |luminance - truth| over the frame, relative to the
truth's mean luminance.  The truth's own noise (printed: ALL's curve
extrapolated to 2048 frames) is a floor under every figure and flatters the
ratios of the last rows.  For 4, 8, .. 128 frames the sweep renders ALL from
frame 1 and reports its error and measured render time (the CPU pass), then
against each baseline (whose curve runs to 1024 frames)
  equal frames     error(ALL, f) / error(baseline, f)
  equal time       error(ALL, f) / error(baseline at the time ALL took for f
                   frames), the baseline error interpolated in log time
                   against log error
  baseline frames  the baseline needs for ALL's error, and that over f
  time to equal error   ALL's time for f frames over the baseline's time for
                   those frames (clamped to the curve: "<=" where the baseline
                   does not reach ALL's error within 1024 frames)
and the frame mean of each estimator relative to the truth's.
"""
import argparse
import math
import os
import sys

import numpy as np

import light_shapes_scenes as ls
from bwrt import Renderer  # noqa: E402
from light_picking_sweep import interp, lum_of  # noqa: E402

TRUTH = 2048
LUM = np.array([0.2126, 0.7152, 0.0722])
FRAMES = (4, 8, 16, 32, 64, 128)
BASE_FRAMES = FRAMES + (256, 512, 1024)
W, H, BOUNCES = 160, 90, 4
CASES = (("quad panel", ls.quad_panel, ("default",)), ("triangle panel", ls.triangle_panel, ("default",)),
         ("Mixed", ls.mixed, ("default", "spheres")))
MODES = {"all": (True, "all"), "spheres": (True, "spheres"), "default": (False, "spheres")}


def context(scene, mode):
    on, shapes = MODES[mode]
    r = Renderer.cpu(0)
    r.set_scene(scene)
    r.set_light_sampling(on)
    r.set_light_shapes(shapes)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = [f"error = mean |luminance - truth| / mean truth, truth = {TRUTH} ALL frames on other RNG streams; CPU backend, "
             f"{W}x{H}, {BOUNCES} bounces, uniform pick"]
    for name, make, bases in CASES:
        sc = make()
        with context(sc, "all") as r:
            r.init_rand(W, H)
            rng, acc = r.get_state(H, W)
            r.set_state(np.roll(rng, (11, 37), axis=(1, 2)), acc, 1)  # every pixel on another pixel's stream
            _, acc = r.render(W, H, TRUTH, BOUNCES, first_frame=1, want_accum=True)
            truth = (acc.astype(np.float64) / TRUTH) @ LUM
        err = lambda img: float(np.abs(img - truth).mean() / truth.mean())  # noqa: E731
        with context(sc, "all") as r:
            imgs = [(f,) + lum_of(r, W, H, f, BOUNCES) for f in FRAMES]
        a = [(f, err(img), ms) for f, img, ms in imgs]
        k = a[-1]
        lines.append(f"--- {name} (the truth's noise about {k[1] * math.sqrt(k[0] / TRUTH):.4f})")
        lines.append("ALL: " + ", ".join(f"{f}: {e:.4f} ({ms:.1f} ms, mean {img.mean() / truth.mean():.4f})"
                                         for (f, e, ms), (_, img, _) in zip(a, imgs)))
        for base in bases:
            with context(sc, base) as r:
                bimgs = [(f,) + lum_of(r, W, H, f, BOUNCES) for f in BASE_FRAMES]
            b = [(f, err(img), ms) for f, img, ms in bimgs]
            lines.append(f"{base}: " + ", ".join(f"{f}: {e:.4f} ({ms:.1f} ms)" for f, e, ms in b))
            lines.append(f"frames   err {base:8s}   err ALL   ms {base:8s}   ms ALL   equal frames   equal time   "
                         f"{base} frames for ALL's error (per frame)   time to equal error   mean {base}")
            for (f, ea, msa), (_, eb, msb), (_, ib, _) in zip(a, b, bimgs):
                et = interp(b, msa, 2, 1)
                bf = interp(b, ea, 1, 0)
                tb = interp(b, bf, 0, 2)
                mark = "<=" if ea < b[-1][1] else "  "
                lines.append(f"{f:6d}   {eb:12.4f}   {ea:7.4f}   {msb:11.1f}   {msa:6.1f}   {ea / eb:12.3f}   {ea / et:10.3f}   "
                             f"{bf:14.0f} ({bf / f:.2f})   {mark}{msa / tb:25.3f}   {ib.mean() / truth.mean():12.4f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
