#!/usr/bin/env python3
"""Cost of a render call with light sampling on (rt_set_light_sampling, the
kernel of csrc/rt_kernel_nee.h) against the default call on GPU 0, in one job:
tools/time_light_sampling.py [--out FILE] [--rounds 3] [--reps 20] [--other-lib LIB]

Headline frame (scene 07, 1920x1080, 8 frames per call, 4 bounces).  A round
measures, one after the other,
  nee      light sampling on: rt_render_nee_kernel
  default  the launch policy's kernel (sorted)
  simple   the default estimator forced onto the one-path-per-lane kernel
           (BWRT_KERNEL=simple): the NEE kernel's own shape without its work
  other    (--other-lib: a library built with the shadow-ray placements
           swapped, tools/variants.sh nee_swapped "-DRT_NEE_INLINE_BRUTE=0
           -DRT_NEE_INLINE_BVH=1": brute-force kernels with the one call site
           per iteration, BVH kernels with a second walk inside the diffuse
           branch) the NEE kernel of that library, measured in a child process
           that loads it
`rounds` rounds alternate them; a point is the median rt_last_kernel_ms of
`reps` calls behind two warm-ups, the result the median of the rounds' points.
Then, once each with its default call beside it: the c3 1/8 row shard and c5
(stress scene, 32 frames, 8 bounces: the BVH instantiation).  The summary goes
to stdout and to --out.
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


SHARD = dict(row_offset=0, row_stride=8)


def make(scene, on, simple=False):
    if simple:
        os.environ["BWRT_KERNEL"] = "simple"
    r = Renderer(0)
    os.environ.pop("BWRT_KERNEL", None)
    r.set_scene(scene)
    r.set_light_sampling(on)
    return r


def point(r, buf, reps, frames=FRAMES, bounces=BOUNCES, **shard):
    ts = []
    for i in range(reps + 2):
        r.render_device(r.params(W, H, frames, bounces, first_frame=1, **shard), buf.data_ptr(), None)
        r.synchronize()
        if i >= 2:
            ts.append(r.last_kernel_ms())
    return statistics.median(ts)


def child(reps, extra):
    """The NEE point of the library this process loaded (BWRT_LIB), as JSON;
    `extra`: the 1/8 shard and c5 as well."""
    buf = tc.output_buffer()
    with make(scenes.scene_07(), True) as r:
        res = {"ms": point(r, buf, reps), "kernel": r.last_kernel_name()}
        if extra:
            res["shard"] = point(r, buf, reps, **SHARD)
    if extra:
        with make(scenes.stress_scene(), True) as r:
            res["c5"] = point(r, buf, 3, frames=32, bounces=8)
    print(json.dumps(res))


def run_child(lib, reps, extra=False):
    env = dict(os.environ, BWRT_LIB=os.path.abspath(lib))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)] + (["--extra"] if extra else [])
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, check=True)
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--other-lib", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--extra", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.reps, args.extra)
    buf = tc.output_buffer()
    s07 = scenes.scene_07()
    ctx = {"nee": make(s07, True), "default": make(s07, False), "simple": make(s07, False, simple=True)}
    lines = [f"scene 07 {W}x{H}, {FRAMES} frames per call, {BOUNCES} bounces; {args.reps} calls per point, median "
             f"rt_last_kernel_ms"]
    rounds = {k: [] for k in list(ctx) + ["other"]}
    names = {}
    for rnd in range(args.rounds):
        got = {}
        for k, r in ctx.items():
            got[k] = point(r, buf, args.reps)
            names[k] = r.last_kernel_name()
        if args.other_lib:
            res = run_child(args.other_lib, args.reps)
            got["other"] = res["ms"]
            names["other"] = res["kernel"] + " (placements swapped)"
        for k, v in got.items():
            rounds[k].append(v)
        lines.append(f"round {rnd}: " + ", ".join(f"{k} {v:.4f}" for k, v in got.items()) + " ms")
    med = {k: statistics.median(v) for k, v in rounds.items() if v}
    for k, v in med.items():
        lines.append(f"{k}: {v:.4f} ms ({min(rounds[k]):.4f} .. {max(rounds[k]):.4f})  {names[k]}")
    lines.append(f"nee / default {med['nee'] / med['default']:.3f}, nee / simple {med['nee'] / med['simple']:.3f}"
                 + (f", other / nee {med['other'] / med['nee']:.3f}" if "other" in med else ""))
    # the c3 1/8 row shard
    a, b = point(ctx["nee"], buf, args.reps, **SHARD), point(ctx["default"], buf, args.reps, **SHARD)
    lines.append(f"c3 1/8 row shard: nee {a:.4f} ms ({ctx['nee'].last_kernel_name()}), default {b:.4f} ms "
                 f"({ctx['default'].last_kernel_name()}): {a / b:.3f}")
    for r in ctx.values():
        r.close()
    # c5: the stress scene
    stress = scenes.stress_scene()
    with make(stress, True) as n, make(stress, False) as d:
        a, b = point(n, buf, 3, frames=32, bounces=8), point(d, buf, 3, frames=32, bounces=8)
        lines.append(f"c5 (stress {W}x{H}, 32 frames, 8 bounces): nee {a:.3f} ms ({n.last_kernel_name()}), default "
                     f"{b:.3f} ms ({d.last_kernel_name()}): {a / b:.3f}")
    if args.other_lib:
        res = run_child(args.other_lib, args.reps, extra=True)
        lines.append(f"other (placements swapped): c3 1/8 row shard {res['shard']:.4f} ms, c5 {res['c5']:.3f} ms")
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
