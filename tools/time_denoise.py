#!/usr/bin/env python3
"""A/B of the denoiser's filter kernels on GPU 0 and their time against the
render step: tools/time_denoise.py [--out FILE] [--pairs 3] [--reps 50] [--levels 5]

Headline frame (scene 07, 1920x1080, 8 frames, 4 bounces).  Per variant
(BWRT_DENOISE_KERNEL=direct|tiled, one context each in this process): 10
warm-up calls, then `reps` calls of rt_denoise_device per level count 1..5,
timed with device events (rt_last_denoise_ms); the variants alternate, `pairs`
times.  Level i's time is the median of T(i + 1 levels) - T(i levels); its
streaming floor is (48 B read + 16 B written) x pixels at 6.3 TB/s.  The plain
render step (8 frames in one launch, rt_last_kernel_ms) runs in the same job
for scale.  The summary goes to stdout and to --out.
"""
import argparse
import os
import statistics

os.environ["BWRT_TUNING"] = "1"
import timing_common as tc  # noqa: E402
from timing_common import BOUNCES, FRAMES, H, W  # noqa: E402

LEVELS = 5
FLOOR_MS = tc.floor_ms(48 + 16)


def make(variant):
    r = tc.make(variant)
    r.render(W, H, FRAMES, BOUNCES, first_frame=1)
    return r


def timed(r, buf, levels, reps):
    return tc.timed(lambda: r.denoise_device(buf.data_ptr(), None, iterations=levels), r.last_denoise_ms, reps)


def main():
    global LEVELS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--levels", type=int, default=LEVELS, help="level counts timed (6 adds step 32)")
    args = ap.parse_args()
    LEVELS = args.levels
    buf = tc.output_buffer()
    ctx = {v: make(v) for v in ("direct", "tiled", None)}
    lines = [f"denoise A/B: scene 07 {W}x{H}, {FRAMES} frames, {BOUNCES} bounces; {args.reps} calls per point, "
             f"median ms; streaming floor per level {FLOOR_MS:.4f} ms"]
    for r in ctx.values():
        timed(r, buf, LEVELS, 10)  # warm-up
    level_ms = {"direct": [[] for _ in range(LEVELS)], "tiled": [[] for _ in range(LEVELS)]}
    total = {"direct": [], "tiled": [], None: []}
    for pair in range(args.pairs):
        for v in ("direct", "tiled"):
            t = [timed(ctx[v], buf, k, args.reps) for k in range(0, LEVELS + 1)]
            total[v].append(t[LEVELS])
            for i in range(LEVELS):
                level_ms[v][i].append(t[i + 1] - t[i])
            lines.append(f"pair {pair} {v:6s}: levels 0..{LEVELS} total " + " ".join(f"{x:.4f}" for x in t))
        total[None].append(timed(ctx[None], buf, LEVELS, args.reps))
        lines.append(f"pair {pair} policy: {LEVELS} levels {total[None][-1]:.4f}")
    lines.append("level step  direct  tiled   (x floor)      winner")
    for i in range(LEVELS):
        d, t = statistics.median(level_ms["direct"][i]), statistics.median(level_ms["tiled"][i])
        lines.append(f"{i:5d} {1 << i:4d}  {d:.4f}  {t:.4f}  ({d / FLOOR_MS:.1f}x / {t / FLOOR_MS:.1f}x)  "
                     f"{'direct' if d <= t else 'tiled'}")
    step = tc.render_step_ms(ctx[None])
    for v in ("direct", "tiled", None):
        m = statistics.median(total[v])
        lines.append(f"{v or 'policy':6s}: {LEVELS} levels {m:.4f} ms = {m / step:.3f} of the render step ({step:.4f} ms)")
    for r in ctx.values():
        r.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
