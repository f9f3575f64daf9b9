#!/usr/bin/env python3
"""Cost of the count-aware post-render passes on GPU 0, each next to the same
call on a uniform accumulation in the same job:
tools/time_adaptive_post.py [--out FILE] [--rounds 3] [--reps 50]

Two contexts on the headline frame (scene 07, 1920x1080, 4 bounces), both
through two views one scripted yaw step apart (rt_controls LEFT, 0.02 s), with a
temporal call at the end of the first, so the second has a history:
  adaptive  per view the sequence of tools/time_adaptive.py: 4 calls x 2 frames
            with tracking on, then one rt_render_adaptive of 8 frames with the
            defaults; rt_set_adaptive_filters on.  Non-uniform: n_p 8 or 16,
            J_p 4 or 5.
  uniform   per view the same start, then one uniform call of the frames that
            give the same mean count (rounded); J = 5.
10 warm-up calls per point, then per round `reps` calls of each point, timed
with device events (rt_last_denoise_ms, rt_last_denoise_var_ms,
rt_last_temporal_ms); the points alternate within a round; medians of the
rounds' medians.  Points, on both contexts:
  rt_denoise at 0 levels (the conversion pass), 1 level (level 0 alone, the one
    count-aware level) and 5 levels;
  rt_denoise_var at 0 levels (the input stage) and 5 levels with min_batches 4
    (every pixel tracked) and 64 (every pixel spatial); on the adaptive context
    also min_batches 5: the selected pixels tracked, the others spatial;
  rt_temporal (every call reprojects the first view).
Streaming floors at 6.3 TB/s, bytes per pixel, uniform -> count-aware (the
count adds 8): conversion pass 32 -> 40 (12 frameSum; 16 colour + 4 RGBA
written), level 0 with its RGBA 64 -> 72 (12 + 32 guides; 20 written), input
stage tracked 40 -> 48 (12 + 8 moments; 20 written), spatial 64 -> 72 (12 + 32
guides; 20 written; the window's overlap is served by the caches), reprojection
144 -> 152 (tools/time_temporal.py).  The summary goes to stdout and to --out.
"""
import argparse
import os
import statistics

os.environ["BWRT_TUNING"] = "1"
import timing_common as tc  # noqa: E402
from timing_common import BOUNCES, H, W, timed  # noqa: E402

START = (2, 2, 2, 2)
K = 8
FLOORS = {"denoise-0": (32, 40), "denoise-1": (64, 72), "var-tracked-0": (40, 48), "var-spatial-0": (64, 72),
          "temporal": (144, 152)}


def view(r, buf, extra):
    """The start, then the adaptive call (extra None) or `extra` uniform frames."""
    for i, k in enumerate(START):
        r.render_device(r.params(W, H, k, BOUNCES, first_frame=1 if i == 0 else 0), buf.data_ptr(), None)
    if extra is None:
        r.render_adaptive_device(buf.data_ptr(), None, BOUNCES, samples=K)
        return r.adaptive_stats()
    r.render_device(r.params(W, H, extra, BOUNCES), buf.data_ptr(), None)
    r.synchronize()
    return None


def make(buf, extra):
    r = tc.make()
    r.set_moments(True)
    r.set_adaptive_filters(True)
    view(r, buf, extra)
    r.temporal(W, H)
    assert r.controls(["LEFT"], 0.02) & 1
    return r, view(r, buf, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    buf = tc.output_buffer()
    p = buf.data_ptr()
    ra, st = make(buf, None)
    npix = W * H
    share = st["selected"] / npix
    mean = st["frames_total"] / npix
    extra = max(1, int(round(mean)) - sum(START))
    ru, _ = make(buf, extra)
    lines = [f"scene 07 {W}x{H}, {BOUNCES} bounces, second of two views; adaptive: start {len(START)} x 2 frames + one "
             f"call of {K}, selected share {share:.4f}, mean {mean:.2f} frames; uniform: {sum(START) + extra} frames, "
             f"{ru.moments_batches} batches; {args.reps} calls per point, median ms"]
    points = {}
    for name, r in (("adaptive", ra), ("uniform", ru)):
        for k in (0, 1, 5):
            points[name, f"denoise-{k}"] = (lambda r=r, k=k: r.denoise_device(p, None, iterations=k), r.last_denoise_ms)
        modes = {"tracked": 4, "spatial": 64}
        if name == "adaptive":
            modes["mixed"] = 5
        for mode, mb in modes.items():
            for k in (0, 5):
                points[name, f"var-{mode}-{k}"] = (
                    lambda r=r, k=k, mb=mb: r.denoise_var_device(p, None, iterations=k, min_batches=mb),
                    r.last_denoise_var_ms)
        points[name, "temporal"] = (lambda r=r: r.temporal_device(p), r.last_temporal_ms)
    for fn, read in points.values():
        timed(fn, read, 10)  # warm-up
    res = {k: [] for k in points}
    for rnd in range(args.rounds):
        for k, (fn, read) in points.items():
            res[k].append(timed(fn, read, args.reps))
        lines.append(f"round {rnd}: " + "  ".join(f"{k[0][0]}:{k[1]} {v[-1]:.4f}" for k, v in res.items()))
    m = {k: statistics.median(v) for k, v in res.items()}
    _, ln = ra.temporal(W, H, want_length=True)
    n = ra.counts(H, W)[0]
    lines.append(f"reprojected share of the adaptive context {float((ln > n).mean()):.3f}")
    lines.append("point             count-aware   uniform    ratio   floor bytes (ratio)   count-aware / its floor")
    for point in [k[1] for k in points if k[0] == "adaptive"]:
        twin = point.replace("mixed", "tracked")
        a, u = m["adaptive", point], m["uniform", twin]
        fb = FLOORS.get(twin)
        tail = (f"   {fb[0]:3d} -> {fb[1]:3d} ({fb[1] / fb[0]:.3f})     {a / tc.floor_ms(fb[1]):.2f}" if fb else "")
        lines.append(f"{point:17s} {a:10.4f} {u:10.4f} {a / u:8.3f}{tail}")
    lines.append("(var-mixed-*: against the uniform context's tracked point; its spatial point is the other bound)")
    ra.close()
    ru.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
