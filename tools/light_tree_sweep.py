#!/usr/bin/env python3
"""Luminance error at equal frames of the light hierarchy, the weighted table
walk and uniform picking (light sampling on in all three), and the render time of
each, on the CPU backend (bit-identical to the GPU, and deterministic):
tools/light_tree_sweep.py [--out FILE]

The scenes of tools/light_tree_scenes.py — tables of 3, 8, 64, 256 and 1,012
lights — at 96x54 with 4 bounces.  Truth: a 2048-frame table-walk render on RNG
streams of its own (every pixel starts on another pixel's stream).  Error: mean
|luminance - truth| over the frame, relative to the truth's mean luminance; the
truth's own noise is a floor under every figure.  For 8, 32 and 128 frames each
pick renders from frame 1; the time is the best of three CPU passes, so
  equal frames   error(hierarchy, f) / error(walk, f) and / error(uniform, f)
  time           ms(hierarchy, f) / ms(walk, f)
and the frame mean of each pick relative to the truth's.
"""
import argparse
import os
import sys

import numpy as np

import light_tree_scenes as lts
from bwrt import Renderer  # noqa: E402

TRUTH = 2048
LUM = np.array([0.2126, 0.7152, 0.0722])
FRAMES = (8, 32, 128)
W, H, BOUNCES = 96, 54, 4
PICKS = (("hierarchy", "weighted", True), ("walk", "weighted", False), ("uniform", "uniform", False))


def context(scene, shapes, pick, hierarchy):
    r = Renderer.cpu(0)
    r.set_scene(scene)
    r.set_light_sampling(True)
    r.set_light_shapes(shapes)
    r.set_light_picking(pick)
    r.set_light_hierarchy(hierarchy)
    return r


def lum_of(r, frames):
    ms = []
    for _ in range(3):
        r.init_rand(W, H)
        _, acc = r.render(W, H, frames, BOUNCES, first_frame=1, want_accum=True)
        ms.append(r.last_kernel_ms())
    return (acc.astype(np.float64) / frames) @ LUM, min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = [f"error = mean |luminance - truth| / mean truth, truth = {TRUTH} table-walk frames on other RNG streams; CPU "
             f"backend, {W}x{H}, {BOUNCES} bounces, light sampling on in every render"]
    for name, (make, shapes) in lts.TABLES.items():
        sc = make()
        with context(sc, shapes, "weighted", False) as r:
            n = len(r.lights())
            depth = 0
            t = r.light_tree()
            for j in range(n):
                k, d = n - 1 + j, 0
                while t[k]["parent"] >= 0:
                    k, d = int(t[k]["parent"]), d + 1
                depth = max(depth, d)
            r.init_rand(W, H)
            rng, acc = r.get_state(H, W)
            r.set_state(np.roll(rng, (11, 37), axis=(1, 2)), acc, 1)
            _, acc = r.render(W, H, TRUTH, BOUNCES, first_frame=1, want_accum=True)
            truth = (acc.astype(np.float64) / TRUTH) @ LUM
        lines.append(f"--- {sc.name}: {n} lights, leaf depth at most {depth}")
        lines.append("frames   err hierarchy   err walk   err uniform   hier / walk   hier / uniform   ms hierarchy   ms walk   "
                     "ms uniform   ms hier / walk   mean hierarchy   mean walk   mean uniform")
        got = {}
        for what, pick, hierarchy in PICKS:
            with context(sc, shapes, pick, hierarchy) as r:
                got[what] = [lum_of(r, f) for f in FRAMES]
        err = lambda img: float(np.abs(img - truth).mean() / truth.mean())
        for i, f in enumerate(FRAMES):
            (ih, mh), (iw, mw), (iu, mu) = got["hierarchy"][i], got["walk"][i], got["uniform"][i]
            eh, ew, eu = err(ih), err(iw), err(iu)
            lines.append(f"{f:6d}   {eh:13.4f}   {ew:8.4f}   {eu:11.4f}   {eh / ew:11.3f}   {eh / eu:14.3f}   {mh:12.1f}   "
                         f"{mw:7.1f}   {mu:10.1f}   {mh / mw:14.3f}   {ih.mean() / truth.mean():14.4f}   "
                         f"{iw.mean() / truth.mean():9.4f}   {iu.mean() / truth.mean():12.4f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
