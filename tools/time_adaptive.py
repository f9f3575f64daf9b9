#!/usr/bin/env python3
"""Cost of one adaptive render call on GPU 0 against the uniform render call it
replaces, in the same job: tools/time_adaptive.py [--out FILE] [--pairs 3] [--reps 50]

Headline frame (scene 07, 1920x1080, 4 bounces) accumulated as 4 calls x 2
frames with tracking on.  A point is that start followed by one call of 8
frames, queued back to back on the context's stream:
  queued   rt_render_adaptive_device with the defaults, BWRT_ADAPTIVE_KERNEL=queued
  simple   the same, BWRT_ADAPTIVE_KERNEL=simple (one path per lane)
  uniform  rt_render_device of 8 frames continuing the accumulation
Warm-ups, then `reps` timed points; the three alternate within a round,
`pairs` rounds, medians of the rounds' medians.  An adaptive call's three
stages are bracketed by device events (rt_adaptive_last_stats): selection
(count fill of the accumulation's first call, row sums, column sums + test,
scan, scatter), the list render kernel, update + resolve; the uniform call is
rt_last_kernel_ms (render kernel + moment update).  Streaming floors at 6.3
TB/s, bytes per pixel (s = selected share):
  selection        8 (fill) + 28 (rows: 16 read, 12 written) + 20 (test: 12 + 8 read) + 4 s (list)
  update + resolve 68 s (listed pixels: 40 read, 28 written) + 24 (resolve: 20 read, 4 written)
The per-kernel split of the selection shows in a kernel trace of this tool
(rocprofv3 --kernel-trace --stats).  The summary goes to stdout and to --out.
"""
import argparse
import os
import statistics

os.environ["BWRT_TUNING"] = "1"
import timing_common as tc  # noqa: E402
from timing_common import BOUNCES, H, W  # noqa: E402

START = (2, 2, 2, 2)
K = 8


def make(kernel):
    os.environ["BWRT_ADAPTIVE_KERNEL"] = kernel
    r = tc.make()
    os.environ.pop("BWRT_ADAPTIVE_KERNEL", None)
    r.set_moments(True)
    return r


def start(r, buf):
    for i, k in enumerate(START):
        r.render_device(r.params(W, H, k, BOUNCES, first_frame=1 if i == 0 else 0), buf.data_ptr(), None)


def adaptive_point(r, buf):
    start(r, buf)
    r.render_adaptive_device(buf.data_ptr(), None, BOUNCES, samples=K)
    return r.adaptive_stats()


def uniform_point(r, buf):
    start(r, buf)
    r.render_device(r.params(W, H, K, BOUNCES), buf.data_ptr(), None)
    r.synchronize()
    return r.last_kernel_ms()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    buf = tc.output_buffer()
    ctx = {"queued": make("queued"), "simple": make("simple")}
    lines = [f"scene 07 {W}x{H}, {BOUNCES} bounces, start {len(START)} calls x 2 frames, then {K} frames; "
             f"{args.reps} per point, median ms"]
    for name, r in ctx.items():
        for _ in range(10):
            st = adaptive_point(r, buf)
        lines.append(f"{name}: {r.last_kernel_name()}")
    for _ in range(10):
        uniform_point(ctx["queued"], buf)
    lines.append(f"uniform: {ctx['queued'].last_kernel_name()}")
    npix = W * H
    share = st["selected"] / npix
    lines.append(f"selected {st['selected']} of {npix} pixels: share {share:.4f}")
    med = statistics.median
    rounds = {k: [] for k in ("queued", "simple", "uniform", "select", "resolve")}
    for rnd in range(args.pairs):
        got = {}
        for name, r in ctx.items():
            pts = [adaptive_point(r, buf) for _ in range(args.reps)]
            got[name] = med(p["render_ms"] for p in pts)
            if name == "queued":
                got["select"] = med(p["select_ms"] for p in pts)
                got["resolve"] = med(p["resolve_ms"] for p in pts)
        got["uniform"] = med(uniform_point(ctx["queued"], buf) for _ in range(args.reps))
        for k, v in got.items():
            rounds[k].append(v)
        lines.append(f"round {rnd}: select {got['select']:.4f}, list render queued {got['queued']:.4f} / simple "
                     f"{got['simple']:.4f}, update + resolve {got['resolve']:.4f}; uniform {K}-frame call "
                     f"{got['uniform']:.4f} ms")
    m = {k: med(v) for k, v in rounds.items()}
    sel_floor = tc.floor_ms(8 + 28 + 20 + 4 * share)
    res_floor = tc.floor_ms(68 * share + 24)
    lines.append(f"selection: {m['select']:.4f} ms = {m['select'] / sel_floor:.2f}x its streaming floor "
                 f"({sel_floor:.4f} ms, {8 + 28 + 20 + 4 * share:.1f} B/pixel)")
    lines.append(f"update + resolve: {m['resolve']:.4f} ms = {m['resolve'] / res_floor:.2f}x its streaming floor "
                 f"({res_floor:.4f} ms, {68 * share + 24:.1f} B/pixel)")
    per_uniform = m["uniform"] / (npix * K)
    for name in ("queued", "simple"):
        ratio = m[name] / (st["selected"] * K) / per_uniform
        lines.append(f"list render {name}: {m[name]:.4f} ms; per selected pixel-frame / uniform per pixel-frame = "
                     f"{ratio:.3f}; break-even selected share {1 / ratio:.3f}")
    whole = m["select"] + min(m["queued"], m["simple"]) + m["resolve"]
    lines.append(f"whole adaptive call (faster kernel) {whole:.4f} ms against the uniform call {m['uniform']:.4f} ms: "
                 f"{whole / m['uniform']:.3f}")
    for r in ctx.values():
        r.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
