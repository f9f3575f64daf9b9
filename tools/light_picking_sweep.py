#!/usr/bin/env python3
"""Error of weighted light picking against uniform picking (both with light
sampling on) at equal frames and at equal time, on the CPU backend
(bit-identical to the GPU): tools/light_picking_sweep.py [--out FILE]

Three cases: scene 07 at 160x90 with 4 bounces and with 1, and
stress_scene(2000, 64, 8) at 96x54 with 4 bounces (a BVH scene).  Truth: a
2048-frame uniform-NEE render on RNG streams of its own (every pixel starts on
another pixel's stream).  Error: mean |luminance - truth| over the frame,
relative to the truth's mean luminance.  The truth's own noise (printed: the
uniform curve extrapolated to 2048 frames) is a floor under every figure and
flatters the ratios of the last rows.  For 4, 8, .. 128 frames the sweep renders
both picks from frame 1 and reports each one's error and measured render time
(the CPU pass), then
  equal frames   error(weighted, f) / error(uniform, f)
  equal time     error(weighted, f) / error(uniform at the time weighted took
                 for f frames), the uniform error interpolated in log time
                 against log error (its curve runs to 1024 frames)
  uniform frames the uniform pick needs for weighted's error, and that over f:
                 the frame equivalent of one weighted frame
and the frame mean of each pick relative to the truth's.
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd")]
from bwrt import Renderer, scenes  # noqa: E402

TRUTH = 2048
LUM = np.array([0.2126, 0.7152, 0.0722])
FRAMES = (4, 8, 16, 32, 64, 128)
UNIFORM_FRAMES = FRAMES + (256, 512, 1024)
CASES = (
    ("07, 160x90, 4 bounces", scenes.scene_07, 160, 90, 4),
    ("07, 160x90, 1 bounce", scenes.scene_07, 160, 90, 1),
    ("stress_scene(2000, 64, 8), 96x54, 4 bounces", lambda: scenes.stress_scene(2000, 64, 8), 96, 54, 4),
)


def context(scene, pick):
    r = Renderer.cpu(0)
    r.set_scene(scene)
    r.set_light_sampling(True)
    r.set_light_picking(pick)
    return r


def lum_of(r, w, h, frames, bounces):
    """(luminance image, ms) of a render of `frames` frames from frame 1; the best of three times."""
    ms = []
    for _ in range(3):
        r.init_rand(w, h)
        _, acc = r.render(w, h, frames, bounces, first_frame=1, want_accum=True)
        ms.append(r.last_kernel_ms())
    return (acc.astype(np.float64) / frames) @ LUM, min(ms)


def interp(curve, x, xi, yi):
    """y at x on the curve's (xi, yi) columns, log-log, clamped to its ends."""
    pts = sorted((c[xi], c[yi]) for c in curve)
    if x <= pts[0][0]:
        return pts[0][1]
    for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
        if x0 <= x <= x1:
            t = (math.log(x) - math.log(x0)) / (math.log(x1) - math.log(x0))
            return math.exp(math.log(y0) + t * (math.log(y1) - math.log(y0)))
    return pts[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = [f"error = mean |luminance - truth| / mean truth, truth = {TRUTH} uniform-NEE frames on other RNG streams; "
             f"CPU backend, light sampling on in every render"]
    for name, make, w, h, bounces in CASES:
        sc = make()
        with context(sc, "uniform") as r:
            r.init_rand(w, h)
            rng, acc = r.get_state(h, w)
            r.set_state(np.roll(rng, (11, 37), axis=(1, 2)), acc, 1)  # every pixel on another pixel's stream
            _, acc = r.render(w, h, TRUTH, bounces, first_frame=1, want_accum=True)
            truth = (acc.astype(np.float64) / TRUTH) @ LUM
        imgs = {}
        for pick in ("uniform", "weighted"):
            with context(sc, pick) as r:
                imgs[pick] = [(f,) + lum_of(r, w, h, f, bounces) for f in (FRAMES if pick == "weighted" else UNIFORM_FRAMES)]
        err = lambda img: float(np.abs(img - truth).mean() / truth.mean())
        u = [(f, err(img), ms) for f, img, ms in imgs["uniform"]]
        wt = [(f, err(img), ms) for f, img, ms in imgs["weighted"]]
        k = [c for c in u if c[0] == 128][0]
        lines.append(f"--- {name} (the truth's noise about {k[1] * math.sqrt(k[0] / TRUTH):.4f})")
        lines.append("uniform: " + ", ".join(f"{f}: {e:.4f} ({ms:.1f} ms)" for f, e, ms in u))
        lines.append("frames   err uniform   err weighted   ms uniform   ms weighted   equal frames   equal time   "
                     "uniform frames for weighted's error (per frame)   mean uniform   mean weighted")
        for (f, ew, msw), (_, eu, msu), (_, iu, _), (_, iw, _) in zip(wt, u, imgs["uniform"], imgs["weighted"]):
            et = interp(u, msw, 2, 1)
            uf = interp(u, ew, 1, 0)
            lines.append(f"{f:6d}   {eu:11.4f}   {ew:12.4f}   {msu:10.1f}   {msw:11.1f}   {ew / eu:12.3f}   {ew / et:10.3f}   "
                         f"{uf:12.0f} ({uf / f:.2f})   {iu.mean() / truth.mean():32.4f}   {iw.mean() / truth.mean():13.4f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
