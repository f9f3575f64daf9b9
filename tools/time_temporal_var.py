#!/usr/bin/env python3
"""Time of rt_temporal_var's passes on GPU 0 against their streaming floors and
against rt_temporal's pass measured in the same job:
tools/time_temporal_var.py [--out FILE] [--rounds 3] [--reps 50]

Headline frame and protocol of tools/time_temporal.py (scene 07, 1920x1080, 4
bounces: 8 frames at view A, one call, one scripted yaw step, 8 frames at view
B; 10 warm-up calls, then per round `reps` calls of every point, the points
alternating within a round; medians of device-event times).  Points:
  tv-history          rt_temporal_var_device in view B, tracking off
  tv-history-tracked  the same with the frame's moments tracked (two batches of
                      4 frames per view: the lane also reads its {M, M2})
  tv-no-history       after rt_temporal_reset in a second context
  temporal            rt_temporal_device in view B: the pass this one extends
  (rt_last_temporal_var_ms / rt_last_temporal_ms: the reprojection pass alone)
  tv-1-temporal       one level behind the call in the tracked context with
                      min_batches 2: every pixel has dof >= 1 there, so every
                      lane takes s2 / len (rt_last_denoise_var_ms)
  tv-1-mixed          the same with tracking off: the reprojected pixels take
                      s2 / len, misses and uncovered pixels (dof 0) the 7 x 7
                      window, and a wave with both kinds runs both paths
  tv-1-spatial        min_batches 1000: every pixel takes the window
  dv-0, dv-1, dv-5    rt_denoise_var alone at 0, 1 and 5 levels
  tv-5                five levels behind the call (min_batches 4: the default)
The input stage is not bracketed on its own: it is T(tv-1-*) minus the sigma
pass and level that rt_denoise_var runs unchanged, T(dv-1) - T(dv-0); dv-0 is
rt_denoise_var's own input stage (spatial: the frame is not tracked).

Streaming floors per pixel at 6.3 TB/s.  Reprojection: reads 32 B guides + 12 B
frameSum (+ 8 B {M, M2} tracked) + ~56 B of distinct history (guide a, guide b,
colour + length, {s2, dof}: each history texel is fetched about once); writes
16 B colour + length, 8 B {s2, dof}, 32 B guide copy, 4 B RGBA.  Input stage,
temporal source: 16 + 8 B read, 16 B written; spatial source: 16 B colour +
32 B guides + 8 B read (each texel of the window about once), 16 B written.
"""
import argparse
import statistics

import timing_common as tc
from timing_common import BOUNCES, FRAMES, H, W
from timing_common import timed as med

WRITE_B = 16 + 8 + 32 + 4
BYTES = {
    "tv-history": 32 + 12 + 56 + WRITE_B,
    "tv-history-tracked": 32 + 12 + 8 + 56 + WRITE_B,
    "tv-no-history": 32 + 12 + WRITE_B,
    "temporal": 32 + 12 + 48 + 16 + 32 + 4,
    "input-temporal": 16 + 8 + 16,
    "input-mixed": 16 + 8 + 16,  # (the floor of the temporal source: what the mix costs shows against it)
    "input-spatial": 16 + 32 + 8 + 16,
}


def make(tracked=False, with_history=True):
    r = tc.make()
    r.set_moments(tracked)

    def frames(first):
        if tracked:  # two batches
            r.render(W, H, FRAMES // 2, BOUNCES, first_frame=first)
            r.render(W, H, FRAMES - FRAMES // 2, BOUNCES)
        else:
            r.render(W, H, FRAMES, BOUNCES, first_frame=first)

    frames(1)
    r.temporal_var(W, H)
    assert r.controls(["LEFT"], 0.02) & 1
    frames(0)
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
    rh, rt, rn = make(), make(tracked=True), make(with_history=False)
    _, mom = rh.temporal_var(W, H, want_moments=True)
    share = float((mom[..., 1] >= 0.5).mean())
    p = buf.data_ptr()
    one = lambda mb: dict(iterations=1, min_batches=mb)  # noqa: E731
    points = {
        "tv-history": (lambda: rh.temporal_var_device(p), rh.last_temporal_var_ms),
        "tv-history-tracked": (lambda: rt.temporal_var_device(p), rt.last_temporal_var_ms),
        "tv-no-history": (lambda: (rn.temporal_reset(), rn.temporal_var_device(p)), rn.last_temporal_var_ms),
        "temporal": (lambda: rh.temporal_device(p), rh.last_temporal_ms),
        "tv-1-temporal": (lambda: rt.temporal_var_device(p, denoise_var=one(2)), rt.last_denoise_var_ms),
        "tv-1-mixed": (lambda: rh.temporal_var_device(p, denoise_var=one(2)), rh.last_denoise_var_ms),
        "tv-1-spatial": (lambda: rh.temporal_var_device(p, denoise_var=one(1000)), rh.last_denoise_var_ms),
        "tv-5": (lambda: rh.temporal_var_device(p, denoise_var={}), rh.last_denoise_var_ms),
    }
    for k in (0, 1, 5):
        points[f"dv-{k}"] = (lambda k=k: rh.denoise_var_device(p, None, iterations=k), rh.last_denoise_var_ms)
    lines = [f"temporal_var timing: scene 07 {W}x{H}, {FRAMES} frames per view, {BOUNCES} bounces, one yaw step; "
             f"{share:.3f} of the pixels reprojected (tv-1-mixed: their share takes the temporal source); "
             f"{args.reps} calls per point, median ms"]
    for fn, read in points.values():
        med(fn, read, 10)  # warm-up
    res = {k: [] for k in points}
    for rnd in range(args.rounds):
        for k, (fn, read) in points.items():
            res[k].append(med(fn, read, args.reps))
        lines.append(f"round {rnd}: " + "  ".join(f"{k} {v[-1]:.4f}" for k, v in res.items()))
    m = {k: statistics.median(v) for k, v in res.items()}
    level1 = m["dv-1"] - m["dv-0"]
    m["input-temporal"] = m["tv-1-temporal"] - level1
    m["input-mixed"] = m["tv-1-mixed"] - level1
    m["input-spatial"] = m["tv-1-spatial"] - level1
    for k, b in BYTES.items():
        fl = tc.floor_ms(b)
        lines.append(f"{k + ':':20s} {m[k]:.4f} ms = {m[k] / fl:.2f} x its floor {fl:.4f} ms ({b} B per pixel)"
                     + (f" = {m[k] / m['temporal']:.2f} x rt_temporal's pass" if k.startswith("tv-") else ""))
    lines += [
        f"sigma pass + level 1 of rt_denoise_var (dv-1 - dv-0): {level1:.4f} ms; its own input stage, spatial "
        f"(dv-0): {m['dv-0']:.4f} ms",
        f"five levels behind the call: {m['tv-5']:.4f} ms; rt_denoise_var alone: {m['dv-5']:.4f} ms",
        f"unfiltered call {m['tv-history']:.4f} ms, filtered call {m['tv-history'] + m['tv-5']:.4f} ms; the input "
        f"stage (mixed sources, as this frame has them: {m['input-mixed']:.4f} ms) is what a fused kernel could save "
        f"at most",
    ]
    for r in (rh, rt, rn):
        r.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
