#!/usr/bin/env python3
"""Error of the two estimators at equal frames and at equal time, on the CPU
backend (bit-identical to the GPU): tools/light_sampling_sweep.py [--out FILE]

Scene 07 at 160x90, 4 bounces, and its twin with every emittance times 2^-4.
Truth: a 1024-frame render of the DEFAULT estimator on RNG streams of its own
(every pixel starts on another pixel's stream).  Error: mean |luminance - truth|
over the frame, relative to the truth's mean luminance.  That truth is itself
noisy (its noise is printed: the default's error curve extrapolated to 1024
frames) and is a floor under every figure, which flatters the default
estimator; the same table is therefore printed a second time against a
1024-frame truth of the NEE estimator, likewise on streams of its own, whose
noise is several times smaller (both estimators have the same expectation:
tests/test_light_sampling.py).  For 4, 8, .. 128 frames the sweep
renders both estimators from frame 1 and reports each one's error and measured
render time (the CPU pass, one thread per chunk as ever), then
  equal frames  error(nee, f) / error(default, f)
  equal time    error(nee, f) / error(default at the time nee took for f frames),
                the default's error interpolated in log time against log error
                (its curve runs to 1024 frames)
and the frames the default estimator needs for NEE's error.
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd")]
from bwrt import Renderer, scenes  # noqa: E402

W, H, BOUNCES, TRUTH = 160, 90, 4, 1024
LUM = np.array([0.2126, 0.7152, 0.0722])
FRAMES = (4, 8, 16, 32, 64, 128)
DEFAULT_FRAMES = FRAMES + (256, 512, 1024)


def scene(factor):
    s = scenes.scene_07()
    for i in range(s.counts[0]):
        s.spheres[i].mat.emittance *= factor
    return s


def lum_of(r, frames):
    """(luminance image, ms) of a render of `frames` frames from frame 1; the best of three times."""
    ms = []
    for _ in range(3):
        r.init_rand(W, H)
        _, acc = r.render(W, H, frames, BOUNCES, first_frame=1, want_accum=True)
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
    lines = [f"scene 07 {W}x{H}, {BOUNCES} bounces; error = mean |luminance - truth| / mean truth, truth = {TRUTH} "
             f"default frames on other RNG streams; CPU backend"]
    for name, factor in (("bright (07)", 1.0), ("dim (07, emittance x 2^-4)", 2.0 ** -4)):
        sc = scene(factor)
        truths = {}
        for on in (False, True):
            with Renderer.cpu(0) as r:
                r.set_scene(sc)
                r.set_light_sampling(on)
                r.init_rand(W, H)
                rng, acc = r.get_state(H, W)
                r.set_state(np.roll(rng, (11, 37), axis=(1, 2)), acc, 1)  # every pixel on another pixel's stream
                _, acc = r.render(W, H, TRUTH, BOUNCES, first_frame=1, want_accum=True)
                truths[on] = (acc.astype(np.float64) / TRUTH) @ LUM
        imgs = {}
        for on in (False, True):
            with Renderer.cpu(0) as r:
                r.set_scene(sc)
                r.set_light_sampling(on)
                imgs[on] = [(f,) + lum_of(r, f) for f in (FRAMES if on else DEFAULT_FRAMES)]
        for ton, tname in ((False, "default"), (True, "nee")):
            truth = truths[ton]
            err = lambda img: float(np.abs(img - truth).mean() / truth.mean())
            d = [(f, err(img), ms) for f, img, ms in imgs[False]]
            n = [(f, err(img), ms) for f, img, ms in imgs[True]]
            src = n if ton else d
            k = [c for c in src if c[0] == 128][0]
            floor = k[1] * math.sqrt(k[0] / TRUTH)
            lines.append(f"--- {name}, against the {tname} estimator's {TRUTH}-frame truth (its noise about {floor:.4f})")
            lines.append("default: " + ", ".join(f"{f}: {e:.4f} ({ms:.1f} ms)" for f, e, ms in d))
            lines.append("frames   err default   err nee   ms default   ms nee   equal frames   equal time   default frames for nee's error")
            for (f, en, msn), (_, ed, msd) in zip(n, d):
                et = interp(d, msn, 2, 1)
                lines.append(f"{f:6d}   {ed:11.4f}   {en:7.4f}   {msd:10.1f}   {msn:6.1f}   {en / ed:12.3f}   {en / et:10.3f}   "
                             f"{interp(d, en, 1, 0):8.0f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
