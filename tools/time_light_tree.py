#!/usr/bin/env python3
"""Cost of a render call with the light hierarchy (rt_set_light_hierarchy, the
tree instantiations of csrc/rt_kernel_nee.h) against the same call with the
weighted table walk and with the uniform pick, light sampling on in all three,
on GPU 0 in one job:
tools/time_light_tree.py [--out FILE] [--rounds 3] [--reps 10]
                         [--parent DIR [--bench-out FILE] [--bench-rounds 3] [--bench-first parent|new]
                          [--bench-only]]

The scenes of tools/light_tree_scenes.py, tables of 3, 8, 64, 256 and 1,012
lights, each in `rounds` alternating rounds (hierarchy, walk, uniform,
hierarchy, ...): the headline frame (scene 07, 1920x1080, 8 frames per call, 4
bounces) and its 1/8 row shard, the 8-light row at the headline size, and the
BVH scenes (64 and 256 sphere lights, the 1,012-triangle mesh) at 1920x1080 with
2 frames per call and 4 bounces, 3 calls per point: a table walk over a thousand
records is long.  A point is the median rt_last_kernel_ms of the calls behind
two warm-ups, the result the median of the rounds' points.

--parent DIR: tools/time_light_picking.py's bench.py comparison against a
checkout of the parent commit with its library built (the default estimator,
whose kernels this change must not move).
"""
import argparse
import os
import statistics

os.environ["BWRT_TUNING"] = "1"
import timing_common as tc  # noqa: E402
from timing_common import BOUNCES, FRAMES, H, W  # noqa: E402
import light_tree_scenes as lts  # noqa: E402
from time_light_picking import SHARD, bench_ab, point  # noqa: E402
from bwrt import Renderer  # noqa: E402

PICKS = (("hierarchy", "weighted", True), ("walk", "weighted", False), ("uniform", "uniform", False))


def make(scene, shapes, pick, hierarchy):
    r = Renderer(0)
    r.set_scene(scene)
    r.set_light_sampling(True)
    r.set_light_shapes(shapes)
    r.set_light_picking(pick)
    r.set_light_hierarchy(hierarchy)
    return r


def compare(lines, what, ctx, buf, rounds, reps, **kw):
    got = {k: [] for k in ctx}
    for rnd in range(rounds):
        for k in ctx:
            got[k].append(point(ctx[k], buf, reps, **kw))
        lines.append(f"  round {rnd}: " + ", ".join(f"{k} {got[k][-1]:.4f}" for k in ctx) + " ms")
    med = {k: statistics.median(v) for k, v in got.items()}
    for k in ctx:
        lines.append(f"  {k}: {med[k]:.4f} ms ({min(got[k]):.4f} .. {max(got[k]):.4f})  {ctx[k].last_kernel_name()}")
    lines.append(f"{what}: hierarchy / walk {med['hierarchy'] / med['walk']:.3f}, hierarchy / uniform "
                 f"{med['hierarchy'] / med['uniform']:.3f}, walk / uniform {med['walk'] / med['uniform']:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent", default="")
    ap.add_argument("--bench-out", default="")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-first", default="parent", choices=("parent", "new"))
    ap.add_argument("--bench-only", action="store_true")
    args = ap.parse_args()
    if args.bench_only:
        return bench_ab(os.path.abspath(args.parent), args.bench_rounds, args.bench_out, args.bench_first)
    buf = tc.output_buffer()
    lines = [f"light sampling on in every call; the hierarchy against the weighted table walk and uniform picking, "
             f"{args.rounds} alternating rounds, median rt_last_kernel_ms; {W}x{H}, {BOUNCES} bounces"]
    for name, (mk, shapes) in lts.TABLES.items():
        scene = mk()
        ctx = {k: make(scene, shapes, pick, h) for k, pick, h in PICKS}
        n = len(ctx["walk"].lights())
        if name in ("3", "8"):
            lines.append(f"{scene.name}: {n} lights, {FRAMES} frames per call; {args.reps} calls per point")
            compare(lines, f"{n} lights, full frame", ctx, buf, args.rounds, args.reps)
            if name == "3":
                compare(lines, f"{n} lights, 1/8 row shard", ctx, buf, args.rounds, args.reps, **SHARD)
        else:
            lines.append(f"{scene.name}: {n} lights (a BVH scene), 2 frames per call; 3 calls per point")
            compare(lines, f"{n} lights", ctx, buf, args.rounds, 3, frames=2)
        for r in ctx.values():
            r.close()
    tc.write_out(lines, args.out)
    if args.parent:
        bench_ab(os.path.abspath(args.parent), args.bench_rounds, args.bench_out, args.bench_first)


if __name__ == "__main__":
    main()
