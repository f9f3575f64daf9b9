#!/usr/bin/env python3
"""Cost of the moment tracking and A/B of the variance-guided filter's kernels on
GPU 0, next to rt_denoise's levels in the same job:
tools/time_denoise_var.py [--out FILE] [--pairs 3] [--reps 50] [--levels 5]

Headline frame (scene 07, 1920x1080, 4 bounces, 8 one-frame render calls, so
the tracking holds 8 batches).

Tracking: 8 render calls of 1 frame from frame 1, queued back to back on the
context's stream, with tracking on against off, `pairs` alternating rounds of
`reps` sequences each: the median of the per-call kernel time
(rt_last_kernel_ms of the last call: render kernel + update pass) and of the
wall time of the 8 calls.  The update pass is the difference; its streaming
floor is 52 B x pixels at 6.3 TB/s.

Filter: per variant (BWRT_DENOISE_KERNEL=direct|tiled, one context each in this
process) and variance mode (tracked: 8 batches; spatial: min_batches above
them): 10 warm-up calls, then `reps` calls of rt_denoise_var_device per level
count 0..levels, timed with device events (rt_last_denoise_var_ms); the
variants alternate, `pairs` times.  The input stage is the time of 0 levels
(it also writes the RGBA there); level i (sigma pass + level kernel) the median
of T(i + 1 levels) - T(i levels).  rt_denoise's levels are timed the same way
in the same rounds.  The sigma pass alone shows in a kernel trace of this tool
(rocprofv3 --kernel-trace --stats).  The summary goes to stdout and to --out.
"""
import argparse
import os
import statistics
import time

os.environ["BWRT_TUNING"] = "1"
import timing_common as tc  # noqa: E402
from timing_common import BOUNCES, H, W, timed  # noqa: E402

CALLS = 8
LEVEL_FLOOR_MS = tc.floor_ms(48 + 16)
UPDATE_FLOOR_MS = tc.floor_ms(52)


def accumulate(r, buf, track):
    """The 8 one-frame calls, queued back to back; (last call's kernel ms, wall ms of the 8)."""
    r.set_moments(track)
    r.synchronize()
    t0 = time.perf_counter()
    for i in range(CALLS):
        r.render_device(r.params(W, H, 1, BOUNCES, first_frame=1 if i == 0 else 0), buf.data_ptr(), None)
    r.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return r.last_kernel_ms(), wall


def make(variant, buf):
    r = tc.make(variant)
    accumulate(r, buf, True)
    assert r.moments_batches == CALLS
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--levels", type=int, default=5, help="level counts timed (6 adds step 32)")
    args = ap.parse_args()
    L = args.levels
    buf = tc.output_buffer()
    lines = [f"scene 07 {W}x{H}, {CALLS} one-frame calls, {BOUNCES} bounces; {args.reps} per point, median ms"]

    # ---- the tracking -----------------------------------------------------------
    r = tc.make()
    for track in (True, False):
        for _ in range(5):
            accumulate(r, buf, track)
    kern = {True: [], False: []}
    wall = {True: [], False: []}
    for rnd in range(args.pairs):
        for track in (True, False):
            got = [accumulate(r, buf, track) for _ in range(args.reps)]
            kern[track].append(statistics.median(g[0] for g in got))
            wall[track].append(statistics.median(g[1] for g in got))
            lines.append(f"round {rnd} tracking {'on ' if track else 'off'}: call {kern[track][-1]:.4f} ms, "
                         f"{CALLS} calls wall {wall[track][-1]:.4f} ms")
    k_on, k_off = statistics.median(kern[True]), statistics.median(kern[False])
    w_on, w_off = statistics.median(wall[True]), statistics.median(wall[False])
    upd = k_on - k_off
    lines.append(f"update pass: {upd:.4f} ms per call = {upd / UPDATE_FLOOR_MS:.2f}x its streaming floor "
                 f"({UPDATE_FLOOR_MS:.4f} ms), {upd / k_off:.3%} of the render call ({k_off:.4f} ms); "
                 f"wall per call {w_on / CALLS:.4f} vs {w_off / CALLS:.4f} ms")
    r.close()

    # ---- the filter ---------------------------------------------------------------
    ctx = {v: make(v, buf) for v in ("direct", "tiled", None)}
    modes = {"tracked": 2, "spatial": CALLS + 1}  # min_batches

    def var_call(r, k, mode):
        return lambda: r.denoise_var_device(buf.data_ptr(), None, iterations=k, min_batches=modes[mode])

    def dn_call(r, k):
        return lambda: r.denoise_device(buf.data_ptr(), None, iterations=k)

    for r in ctx.values():
        for mode in modes:
            timed(var_call(r, L, mode), r.last_denoise_var_ms, 10)  # warm-up
        timed(dn_call(r, L), r.last_denoise_ms, 10)
    keys = [(v, m) for v in ("direct", "tiled") for m in ("tracked", "spatial", "rt_denoise")]
    level_ms = {k: [[] for _ in range(L)] for k in keys}
    input_ms = {k: [] for k in keys}
    total = {k: [] for k in keys + [(None, m) for m in ("tracked", "spatial", "rt_denoise")]}
    for pair in range(args.pairs):
        for v in ("direct", "tiled"):
            r = ctx[v]
            for m in ("tracked", "spatial", "rt_denoise"):
                if m == "rt_denoise":
                    t = [timed(dn_call(r, k), r.last_denoise_ms, args.reps) for k in range(0, L + 1)]
                else:
                    t = [timed(var_call(r, k, m), r.last_denoise_var_ms, args.reps) for k in range(0, L + 1)]
                total[v, m].append(t[L])
                input_ms[v, m].append(t[0])
                for i in range(L):
                    level_ms[v, m][i].append(t[i + 1] - t[i])
                lines.append(f"pair {pair} {v:6s} {m:10s}: levels 0..{L} total " + " ".join(f"{x:.4f}" for x in t))
        r = ctx[None]
        for m in ("tracked", "spatial"):
            total[None, m].append(timed(var_call(r, L, m), r.last_denoise_var_ms, args.reps))
        total[None, "rt_denoise"].append(timed(dn_call(r, L), r.last_denoise_ms, args.reps))
    med = statistics.median
    lines.append(f"input stage (0 levels): tracked {med(input_ms['direct', 'tracked']):.4f}, spatial "
                 f"{med(input_ms['direct', 'spatial']):.4f}; rt_denoise's conversion pass "
                 f"{med(input_ms['direct', 'rt_denoise']):.4f} ms")
    lines.append(f"level = sigma pass + level kernel; streaming floor of a level kernel {LEVEL_FLOOR_MS:.4f} ms")
    lines.append("level step  var direct  var tiled  winner   rt_denoise direct  tiled")
    for i in range(L):
        d, t = med(level_ms["direct", "tracked"][i]), med(level_ms["tiled", "tracked"][i])
        ds, ts = med(level_ms["direct", "spatial"][i]), med(level_ms["tiled", "spatial"][i])
        pd, pt = med(level_ms["direct", "rt_denoise"][i]), med(level_ms["tiled", "rt_denoise"][i])
        lines.append(f"{i:5d} {1 << i:4d}  {d:.4f}      {t:.4f}     {'direct' if d <= t else 'tiled ':6s}   "
                     f"{pd:.4f}             {pt:.4f}   (spatial-mode frame: {ds:.4f} / {ts:.4f})")
    for m in ("tracked", "spatial", "rt_denoise"):
        lines.append(f"{m:10s} {L} levels: direct {med(total['direct', m]):.4f}, tiled {med(total['tiled', m]):.4f}, "
                     f"policy {med(total[None, m]):.4f} ms")
    for r in ctx.values():
        r.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
