#!/usr/bin/env python3
"""Time of the temporal reprojection pass on GPU 0 against its streaming floor,
the denoiser's levels and the render step:
tools/time_temporal.py [--out FILE] [--rounds 3] [--reps 50]

Headline frame (scene 07, 1920x1080, 4 bounces): 8 frames at view A, one
temporal call, one scripted yaw step (rt_controls LEFT, 0.02 s = 0.04 rad), 8
frames at view B.  Then 10 warm-up calls and, per round, `reps` calls each of
  history     rt_temporal_device in view B (every call reprojects view A: a
              repeated call in one view leaves the history alone),
  no-history  the same after rt_temporal_reset in a second context (every
              pixel takes the early exit),
  filtered    rt_temporal_device with the default denoiser behind it (the
              reprojection pass alone is reported, and the levels),
  levels      rt_denoise_device at 0..5 levels (level i = T(i + 1) - T(i)),
timed with device events (rt_last_temporal_ms / rt_last_denoise_ms), medians;
the points alternate within a round.  The render step (8 frames in one launch,
rt_last_kernel_ms) runs in the same job.

Streaming floor per pixel: reads 32 B guides + 12 B frameSum + ~48 B of
distinct history (guide a, guide b, colour + length: neighbouring lanes'
bilinear footprints overlap, so each history texel is fetched about once);
writes 16 B pending colour + 32 B guide copy + 4 B RGBA; at 6.3 TB/s.  The
summary goes to stdout and to --out.
"""
import argparse
import statistics

import timing_common as tc
from timing_common import BOUNCES, FRAMES, H, W
from timing_common import timed as med

LEVELS = 5
READ_B, WRITE_B = 32 + 12 + 48, 16 + 32 + 4
FLOOR_MS = tc.floor_ms(READ_B + WRITE_B)
FLOOR_NOHIST_MS = tc.floor_ms(32 + 12 + WRITE_B)


def make(with_history):
    r = tc.make()
    r.render(W, H, FRAMES, BOUNCES, first_frame=1)
    r.temporal(W, H)
    assert r.controls(["LEFT"], 0.02) & 1
    r.render(W, H, FRAMES, BOUNCES)
    if not with_history:
        r.temporal_reset()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    buf = tc.output_buffer()
    rh, rn = make(True), make(False)
    _, ln = rh.temporal(W, H, want_length=True)
    share = float((ln > FRAMES).mean())
    p = buf.data_ptr()
    points = {
        "history": (lambda: rh.temporal_device(p), rh.last_temporal_ms),
        "no-history": (lambda: (rn.temporal_reset(), rn.temporal_device(p)), rn.last_temporal_ms),
        "filtered": (lambda: rh.temporal_device(p, denoise={}), rh.last_temporal_ms),
        "filter-levels": (lambda: rh.temporal_device(p, denoise={}), rh.last_denoise_ms),
    }
    for k in range(LEVELS + 1):
        points[f"denoise-{k}"] = (lambda k=k: rh.denoise_device(p, None, iterations=k), rh.last_denoise_ms)
    lines = [f"temporal timing: scene 07 {W}x{H}, {FRAMES} frames per view, {BOUNCES} bounces, one yaw step; "
             f"{share:.3f} of the pixels reprojected; {args.reps} calls per point, median ms",
             f"streaming floor {FLOOR_MS:.4f} ms ({READ_B} B read + {WRITE_B} B written per pixel at 6.3 TB/s); "
             f"without history {FLOOR_NOHIST_MS:.4f} ms"]
    for fn, read in points.values():
        med(fn, read, 10)  # warm-up
    res = {k: [] for k in points}
    for rnd in range(args.rounds):
        for k, (fn, read) in points.items():
            res[k].append(med(fn, read, args.reps))
        lines.append(f"round {rnd}: " + "  ".join(f"{k} {v[-1]:.4f}" for k, v in res.items()))
    m = {k: statistics.median(v) for k, v in res.items()}
    step = tc.render_step_ms(rn)
    levels = [m[f"denoise-{k + 1}"] - m[f"denoise-{k}"] for k in range(LEVELS)]
    lines += [
        f"reprojection pass, history:    {m['history']:.4f} ms = {m['history'] / FLOOR_MS:.2f} x floor = "
        f"{m['history'] / step:.4f} of the render step ({step:.4f} ms, {FRAMES} frames)",
        f"reprojection pass, no history: {m['no-history']:.4f} ms = {m['no-history'] / FLOOR_NOHIST_MS:.2f} x its floor",
        f"reprojection pass before the filter (no RGBA store): {m['filtered']:.4f} ms; the {LEVELS} levels behind "
        f"it {m['filter-levels']:.4f} ms (rt_denoise alone: {m[f'denoise-{LEVELS}']:.4f} ms)",
        "denoiser levels (policy): " + " ".join(f"{x:.4f}" for x in levels) + f"; cheapest {min(levels):.4f} ms; "
        f"the reprojection pass is {m['history'] / min(levels):.2f} x the cheapest level",
    ]
    rh.close()
    rn.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
