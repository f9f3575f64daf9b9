#!/usr/bin/env python3
"""Cost of the moving-camera adaptive loop on GPU 0:
tools/time_adaptive_temporal.py [--out FILE] [--rounds 3] [--reps 50]

Method of tools/time_adaptive.py: warm-ups, `reps` timed points, the points
alternating within a round, `rounds` rounds, medians of the rounds' medians of
device-event times.  Headline frame (scene 07, 1920x1080, 4 bounces), the second
view after one scripted yaw step; view A went through the loop once, so view B
has a history with moments.  Points, each queued on the context's stream:
  loop      rt_render_device (K frames, frame 1: one tracked batch),
            rt_temporal_var_device, rt_render_adaptive_reprojected_device (K
            frames, the defaults), rt_temporal_var_counted_device.  Read: the
            uniform kernel, the rt_temporal_var pass (TvPixel, the frame not yet
            tracked: one batch), the adaptive call's three stages
            (rt_adaptive_last_stats), the counted pass (TvPixelCnt).
  uniform   rt_render_device (K frames, frame 1), rt_temporal_var_device,
            rt_render_device (K more frames), rt_temporal_var_device: the
            uniform call of the same frames, and TvPixel on a tracked frame of
            two batches.
  adaptive  tools/time_adaptive.py's point in a second context (4 x 2 frames,
            then rt_render_adaptive_device): the selection this one is compared
            with.
Streaming floors at 6.3 TB/s, bytes per pixel (s = selected share):
  selection, reprojected   8 (fill) + 36 (rows: 24 read, 12 written) + 28 (test: 12 + 8 + 4 + 4 read) + 4 s (list)
  selection, rt_adaptive   8 + 28 + 20 + 4 s
  TvPixel                  160 untracked, 168 tracked (tools/time_temporal_var.py)
  TvPixelCnt               168 + 8 s: the counts, and {M, M2} where J_p >= 2 (the selected pixels)
"""
import argparse
import os
import statistics

os.environ["BWRT_TUNING"] = "1"
import timing_common as tc  # noqa: E402
from timing_common import BOUNCES, H, W  # noqa: E402

K = 8
START = (2, 2, 2, 2)
med = statistics.median


def make():
    r = tc.make()
    r.set_moments(True)
    r.set_adaptive_filters(True)
    return r


def loop_point(r, p):
    r.render_device(r.params(W, H, K, BOUNCES, first_frame=1), p, None)
    r.temporal_var_device(p)
    out = {"kernel": r.last_kernel_ms(), "tv": r.last_temporal_var_ms()}
    r.render_adaptive_reprojected_device(p, None, BOUNCES, samples=K)
    st = r.adaptive_stats()
    r.temporal_var_counted_device(p)
    out.update(select=st["select_ms"], render=st["render_ms"], resolve=st["resolve_ms"], tvc=r.last_temporal_var_ms(),
               selected=st["selected"])
    return out


def uniform_point(r, p):
    r.render_device(r.params(W, H, K, BOUNCES, first_frame=1), p, None)
    r.temporal_var_device(p)
    r.render_device(r.params(W, H, K, BOUNCES), p, None)
    r.synchronize()
    out = {"kernel2": r.last_kernel_ms()}
    r.temporal_var_device(p)
    out["tv_tracked"] = r.last_temporal_var_ms()
    return out


def adaptive_point(r, p):
    for i, k in enumerate(START):
        r.render_device(r.params(W, H, k, BOUNCES, first_frame=1 if i == 0 else 0), p, None)
    r.render_adaptive_device(p, None, BOUNCES, samples=K)
    st = r.adaptive_stats()
    return {"ad_select": st["select_ms"], "ad_selected": st["selected"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    buf = tc.output_buffer()
    p = buf.data_ptr()
    rl, ru, ra = make(), make(), make()
    ra.set_adaptive_filters(False)
    for r, point in ((rl, loop_point), (ru, uniform_point)):  # view A, the yaw step, then view B is where the points run
        point(r, p)
        assert r.controls(["LEFT"], 0.02) & 1
    points = {"loop": (rl, loop_point), "uniform": (ru, uniform_point), "adaptive": (ra, adaptive_point)}
    for r, point in points.values():
        for _ in range(10):
            last = point(r, p)
    npix = W * H
    lines = [f"scene 07 {W}x{H}, {BOUNCES} bounces, view B after one yaw step, {K} + {K} frames; {args.reps} per point, "
             f"median ms", f"list render kernel: {rl.last_kernel_name()}"]
    rounds = {}
    for rnd in range(args.rounds):
        got = {}
        for name, (r, point) in points.items():
            pts = [point(r, p) for _ in range(args.reps)]
            for k in pts[0]:
                got[k] = med(x[k] for x in pts)
        for k, v in got.items():
            rounds.setdefault(k, []).append(v)
        lines.append(f"round {rnd}: " + "  ".join(f"{k} {v:.4f}" for k, v in got.items() if "selected" not in k))
    m = {k: med(v) for k, v in rounds.items()}
    s, s_ad = m["selected"] / npix, m["ad_selected"] / npix
    lines.append(f"selected share: reprojected {s:.4f}, rt_render_adaptive {s_ad:.4f}")
    fl_sel, fl_ad = tc.floor_ms(8 + 36 + 28 + 4 * s), tc.floor_ms(8 + 28 + 20 + 4 * s_ad)
    lines.append(f"selection, reprojected: {m['select']:.4f} ms = {m['select'] / fl_sel:.2f} x its floor {fl_sel:.4f} ms "
                 f"({8 + 36 + 28 + 4 * s:.1f} B per pixel) = {m['select'] / m['ad_select']:.3f} x rt_render_adaptive's "
                 f"{m['ad_select']:.4f} ms ({m['ad_select'] / fl_ad:.2f} x its floor {fl_ad:.4f} ms)")
    for k, name, b in (("tv", "TvPixel, one batch (untracked)", 160), ("tv_tracked", "TvPixel, two batches (tracked)", 168),
                       ("tvc", "TvPixelCnt", 168 + 8 * s)):
        fl = tc.floor_ms(b)
        lines.append(f"{name + ':':34s} {m[k]:.4f} ms = {m[k] / fl:.2f} x its floor {fl:.4f} ms ({b:.1f} B per pixel)")
    lines.append(f"TvPixelCnt / TvPixel tracked: {m['tvc'] / m['tv_tracked']:.3f}; / TvPixel untracked: "
                 f"{m['tvc'] / m['tv']:.3f}")
    step34 = m["select"] + m["render"] + m["resolve"] + m["tvc"]
    uni = m["kernel2"] + m["tv_tracked"]
    lines.append(f"steps 3 + 4: select {m['select']:.4f} + list render {m['render']:.4f} + update and resolve "
                 f"{m['resolve']:.4f} + counted pass {m['tvc']:.4f} = {step34:.4f} ms against a uniform call of the same "
                 f"{K} frames + rt_temporal_var {m['kernel2']:.4f} + {m['tv_tracked']:.4f} = {uni:.4f} ms: "
                 f"{step34 / uni:.3f} at a selected share of {s:.3f}")
    for r in (rl, ru, ra):
        r.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
