#!/usr/bin/env python3
"""Cost of a render call that samples polygon lights (rt_set_light_shapes,
RT_LIGHT_SHAPES_ALL: the polygon-aware instantiations of csrc/rt_kernel_nee.h)
against the sphere-only call and the default estimator's call on the same
scene, on GPU 0 in one job:
tools/time_light_shapes.py [--out FILE] [--rounds 3] [--reps 20]
                           [--parent DIR [--bench-out FILE] [--bench-rounds 3] [--bench-first parent|new]
                            [--bench-only]]

Each configuration in `rounds` alternating rounds over its modes.  At
1920x1080, 8 frames per call, 4 bounces: the Mixed scene (scene 07's three
sphere lights and a ceiling panel of four quads) and the quad panel alone,
under ALL with uniform and with weighted picking, under SPHERES (Mixed: the
sphere-only NEE kernel; the panel alone: an empty table, the default kernel)
and with light sampling off; Mixed's 1/8 row shard; scene 07 under ALL against
SPHERES (no polygon emitter: the same kernel, the difference is noise); and c5
(stress scene, 32 frames, 8 bounces, BVH) with four emissive triangles, 3
calls per point.  A point is the median rt_last_kernel_ms of `reps` calls
behind two warm-ups, the result the median of the rounds' points.

--parent DIR: as tools/time_light_picking.py's (bench.py alternating between
the parent commit's tree and this one).
"""
import argparse
import os
import statistics

os.environ["BWRT_TUNING"] = "1"
import timing_common as tc  # noqa: E402
from timing_common import BOUNCES, FRAMES, H, W  # noqa: E402
from bwrt import Renderer, scenes  # noqa: E402
import light_shapes_scenes as ls  # noqa: E402
from time_light_picking import bench_ab, point  # noqa: E402

SHARD = dict(row_offset=0, row_stride=8)
# mode -> (light sampling, shapes, picking)
MODES = {"all": (True, "all", "uniform"), "all,weighted": (True, "all", "weighted"), "spheres": (True, "spheres", "uniform"),
         "spheres,weighted": (True, "spheres", "weighted"), "default": (False, "spheres", "uniform")}


def make(scene, mode):
    on, shapes, pick = MODES[mode]
    r = Renderer(0)
    r.set_scene(scene)
    r.set_light_sampling(on)
    r.set_light_shapes(shapes)
    r.set_light_picking(pick)
    return r


def compare(lines, what, scene, modes, buf, rounds, reps, **kw):
    ctx = {k: make(scene, k) for k in modes}
    got = {k: [] for k in modes}
    for rnd in range(rounds):
        for k in modes:
            got[k].append(point(ctx[k], buf, reps, **kw))
        lines.append(f"  round {rnd}: " + ", ".join(f"{k} {got[k][-1]:.4f}" for k in modes) + " ms")
    med = {k: statistics.median(v) for k, v in got.items()}
    for k in modes:
        lines.append(f"  {k}: {med[k]:.4f} ms ({min(got[k]):.4f} .. {max(got[k]):.4f})  {ctx[k].last_kernel_name()}")
    base = modes[-1]
    lines.append(f"{what}: " + ", ".join(f"{k} / {base} {med[k] / med[base]:.3f}" for k in modes[:-1]))
    if "spheres" in modes and base != "spheres":
        lines.append(f"{what}: " + ", ".join(f"{k} / spheres {med[k] / med['spheres']:.3f}" for k in modes if k.startswith("all")))
    for r in ctx.values():
        r.close()
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", default="")
    ap.add_argument("--bench-out", default="")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-first", default="parent", choices=("parent", "new"))
    ap.add_argument("--bench-only", action="store_true")
    args = ap.parse_args()
    if args.bench_only:
        return bench_ab(os.path.abspath(args.parent), args.bench_rounds, args.bench_out, args.bench_first)
    buf = tc.output_buffer()
    lines = [f"polygon lights (ALL) against sphere-only NEE (SPHERES) and the default estimator, {args.rounds} alternating "
             f"rounds, median rt_last_kernel_ms; {W}x{H}, {FRAMES} frames per call, {BOUNCES} bounces, {args.reps} calls per point"]
    five = ("all", "all,weighted", "spheres", "spheres,weighted", "default")
    lines.append("Mixed: scene 07 (3 sphere lights) and a panel of 4 quad lights")
    compare(lines, "Mixed", ls.mixed(), five, buf, args.rounds, args.reps)
    lines.append("Mixed, 1/8 row shard")
    compare(lines, "Mixed 1/8 shard", ls.mixed(), five, buf, args.rounds, args.reps, **SHARD)
    lines.append("quad panel: scene 07's geometry lit by the 4 quad lights alone (SPHERES: an empty table, the default kernel)")
    compare(lines, "quad panel", ls.quad_panel(), ("all", "all,weighted", "spheres", "default"), buf, args.rounds, args.reps)
    lines.append("scene 07, no polygon emitter: ALL and SPHERES launch the same kernel")
    compare(lines, "07", scenes.scene_07(), ("all", "spheres"), buf, args.rounds, args.reps)
    lines.append("c5 with 4 emissive triangles: stress scene, 32 frames per call, 8 bounces, 8 sphere lights; 3 calls per point")
    compare(lines, "c5", ls.stress_with_emissive_triangles(), five, buf, args.rounds, 3, frames=32, bounces=8)
    tc.write_out(lines, args.out)
    if args.parent:
        bench_ab(os.path.abspath(args.parent), args.bench_rounds, args.bench_out, args.bench_first)


if __name__ == "__main__":
    main()
