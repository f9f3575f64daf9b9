#!/usr/bin/env python3
"""Cost of a render call with weighted light picking (rt_set_light_picking,
the weighted instantiations of csrc/rt_kernel_nee.h) against the same call with
the uniform pick, light sampling on in both, on GPU 0 in one job:
tools/time_light_picking.py [--out FILE] [--rounds 3] [--reps 20]
                            [--parent DIR [--bench-out FILE] [--bench-rounds 3] [--bench-first parent|new]
                             [--bench-only]]

Three configurations, each in `rounds` alternating rounds (weighted, uniform,
weighted, ...): the headline frame (scene 07, 1920x1080, 8 frames per call, 4
bounces), its 1/8 row shard, and c5 (stress scene, 32 frames, 8 bounces: the
BVH instantiation, 3 calls per point).  A point is the median
rt_last_kernel_ms of `reps` calls behind two warm-ups, the result the median
of the rounds' points.

--parent DIR: a checkout of the parent commit with its library built.  Then
`bench.py --gpus 1 --steps 200 --warmup 20` (the default estimator, whose
kernels this change must not move) runs in DIR and in this tree alternately,
`bench-rounds` times each, one child process per run, the order within a round
swapping from round to round and starting with --bench-first; the summary goes
to --bench-out.  --bench-only skips the picking comparison.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

os.environ["BWRT_TUNING"] = "1"
import timing_common as tc  # noqa: E402
from timing_common import BOUNCES, FRAMES, H, W  # noqa: E402
from bwrt import Renderer, scenes  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARD = dict(row_offset=0, row_stride=8)
PICKS = ("weighted", "uniform")


def make(scene, pick):
    r = Renderer(0)
    r.set_scene(scene)
    r.set_light_sampling(True)
    r.set_light_picking(pick)
    return r


def point(r, buf, reps, frames=FRAMES, bounces=BOUNCES, **shard):
    ts = []
    for i in range(reps + 2):
        r.render_device(r.params(W, H, frames, bounces, first_frame=1, **shard), buf.data_ptr(), None)
        r.synchronize()
        if i >= 2:
            ts.append(r.last_kernel_ms())
    return statistics.median(ts)


def compare(lines, what, ctx, buf, rounds, reps, **kw):
    got = {k: [] for k in PICKS}
    for rnd in range(rounds):
        for k in PICKS:
            got[k].append(point(ctx[k], buf, reps, **kw))
        lines.append(f"  round {rnd}: " + ", ".join(f"{k} {got[k][-1]:.4f}" for k in PICKS) + " ms")
    med = {k: statistics.median(v) for k, v in got.items()}
    for k in PICKS:
        lines.append(f"  {k}: {med[k]:.4f} ms ({min(got[k]):.4f} .. {max(got[k]):.4f})  {ctx[k].last_kernel_name()}")
    lines.append(f"{what}: weighted / uniform {med['weighted'] / med['uniform']:.3f}")
    return med


def bench(tree):
    cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20"]
    env = {k: v for k, v in os.environ.items() if k != "BWRT_TUNING"}
    out = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=600, check=True)
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    return res["ms_per_step"], res["kernel_ms_avg"]


def bench_ab(parent, rounds, out, first):
    lines = ["bench.py --gpus 1 --steps 200 --warmup 20 (the default estimator), the parent commit's tree and library "
             "against this one, alternating in one job; ms per step"]
    got = {"parent": [], "new": []}
    for rnd in range(rounds):
        order = [("parent", parent), ("new", REPO)]
        if (rnd % 2 == 0) != (first == "parent"):
            order.reverse()
        row = []
        for k, tree in order:
            ms, kms = bench(tree)
            got[k].append(ms)
            row.append(f"{k} {rnd + 1}: {ms:.4f} (kernel {kms:.4f})")
        lines.append("  " + "   ".join(row))
    for k, v in got.items():
        lines.append(f"{k}: median {statistics.median(v):.4f} ms, spread {min(v):.4f} .. {max(v):.4f}")
    tc.write_out(lines, out)


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
    lines = [f"light sampling on in every call; weighted against uniform picking, {args.rounds} alternating rounds, median "
             f"rt_last_kernel_ms"]
    s07 = scenes.scene_07()
    ctx = {k: make(s07, k) for k in PICKS}
    lines.append(f"scene 07 {W}x{H}, {FRAMES} frames per call, {BOUNCES} bounces, 3 lights; {args.reps} calls per point")
    compare(lines, "headline frame", ctx, buf, args.rounds, args.reps)
    compare(lines, "c3 1/8 row shard", ctx, buf, args.rounds, args.reps, **SHARD)
    for r in ctx.values():
        r.close()
    stress = scenes.stress_scene()
    ctx = {k: make(stress, k) for k in PICKS}
    lines.append(f"c5: stress scene {W}x{H}, 32 frames per call, 8 bounces, 8 lights; 3 calls per point")
    compare(lines, "c5", ctx, buf, args.rounds, 3, frames=32, bounces=8)
    for r in ctx.values():
        r.close()
    tc.write_out(lines, args.out)
    if args.parent:
        bench_ab(os.path.abspath(args.parent), args.bench_rounds, args.bench_out, args.bench_first)


if __name__ == "__main__":
    main()
