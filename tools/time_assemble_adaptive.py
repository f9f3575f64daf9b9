#!/usr/bin/env python3
"""Cost of a counted assembled frame on GPU 0:
tools/time_assemble_adaptive.py [--out FILE] [--pairs 3] [--reps 50]

Headline frame (scene 07, 1920x1080, 4 bounces) as 8 row shards held by 8
contexts on the one GPU after 4 render calls of 2 frames with the moments
tracked and one adaptive call of 8 frames (rt_render_adaptive_multi), and the
same sequence on one full-frame context (rt_render_adaptive).

Export: rt_export_shard_adaptive_device of one shard (135 rows) with 4 and
with 7 planes, beside rt_export_shard_device with 3 and 5 planes of a shard
context that stayed uniform; device events around the call on a caller's
stream.  Assembly: rt_assemble_adaptive_device of the 8 gathered blocks with 4
and 7 planes beside rt_assemble_device with 3 and 5 (rt_last_assemble_ms).
Each against its streaming floor: every word is read once and written once, so
8 B x words moved at 6.3 TB/s.  Filters: rt_denoise (5 levels), rt_denoise_var
and rt_temporal on the shard context that holds the counted assembled frame (7
planes) against the same call on the full-frame adaptive context: the same
kernels on other buffers, so the ratio is what is reported.  10 warm-up calls,
the points alternating, `reps` calls per point, `pairs` rounds, medians.  The
summary goes to stdout and to --out.
"""
import argparse
import os
import statistics

os.environ["BWRT_TUNING"] = "1"
import timing_common as tc  # noqa: E402
from timing_common import BOUNCES, H, W, timed  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bwrt import render_adaptive_multi  # noqa: E402

SHARDS = 8
CALLS = 4
FRAMES = 2
ADAPTIVE = dict(samples=8, tolerance=0.1, lum_floor=0.01, radius=2)
RPS = -(-H // SHARDS)
PLANES = (3, 5, 4, 7)


def floor_ms(words):
    return 8 * words / 6.3e12 * 1e3


def accumulate(r, off=0, stride=1):
    r.set_moments(True)
    r.set_max_bounces(BOUNCES)
    for k in range(CALLS):
        r.render(W, H, FRAMES, BOUNCES, first_frame=1 if k == 0 else 0, row_offset=off, row_stride=stride)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    lines = [f"scene 07 {W}x{H}, {CALLS} x {FRAMES} frames then one adaptive call of {ADAPTIVE['samples']}, {BOUNCES} "
             f"bounces, {SHARDS} row shards on one GPU; {args.reps} per point, median ms"]
    rs = [tc.make() for _ in range(SHARDS)]
    full, uniform = tc.make(), tc.make()
    for i, r in enumerate(rs):
        accumulate(r, i, SHARDS)
    accumulate(full)
    accumulate(uniform, 0, SHARDS)  # shard 0 again, kept uniform: the 3- and 5-plane export
    _, st = render_adaptive_multi(rs, W, H, BOUNCES, **ADAPTIVE)
    _, fst = full.render_adaptive(W, H, BOUNCES, **ADAPTIVE)
    assert st["selected"] == fst["selected"] and 0 < st["selected"] < W * H, (st, fst)
    lines.append(f"the adaptive call selected {st['selected']} of {W * H} pixels")
    for r in rs + [full]:
        r.set_adaptive_filters(True)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    gathered = {p: torch.zeros((SHARDS, p, RPS, W), dtype=torch.float32, device="cuda") for p in PLANES}
    out = tc.output_buffer()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    base = {}

    def export(i, planes):
        ptr = gathered[planes][i].data_ptr()
        if planes in (4, 7):
            base[planes] = rs[i].export_shard_adaptive_device(ptr, RPS, planes, sp)
        else:
            base[planes] = uniform.export_shard_device(ptr, RPS, planes, sp)

    def export_ms(i, planes):
        e0.record(stream)
        export(i, planes)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def assemble(planes):
        n, j = base[planes]
        ptr = gathered[planes].data_ptr()
        if planes in (4, 7):
            return lambda: rs[0].assemble_adaptive_device(ptr, SHARDS, RPS, planes, n, j, sp)
        return lambda: rs[0].assemble_device(ptr, SHARDS, RPS, planes, n, j, sp)

    for p in PLANES:  # every block (the uniform context's for every slot of 3 and 5), then the warm-ups
        for i in range(SHARDS):
            export(i, p)
        for _ in range(10):
            export_ms(0, p)
        timed(assemble(p), rs[0].last_assemble_ms, 10)
    assert base[7] == (CALLS * FRAMES, CALLS), base
    ex = {p: [] for p in PLANES}
    asm = {p: [] for p in PLANES}
    for rnd in range(args.pairs):
        for p in PLANES:
            ex[p].append(statistics.median(export_ms(0, p) for _ in range(args.reps)))
            asm[p].append(timed(assemble(p), rs[0].last_assemble_ms, args.reps))
        lines.append(f"round {rnd}: export 3/5/4/7 planes " + " / ".join(f"{ex[p][-1]:.4f}" for p in PLANES)
                     + ", assembly " + " / ".join(f"{asm[p][-1]:.4f}" for p in PLANES))
    # the filters read the counted frame of 7 planes
    assemble(7)()
    passes = {
        "rt_denoise, 5 levels": (lambda r: (lambda: r.denoise_device(out.data_ptr(), None, iterations=5)),
                                 lambda r: r.last_denoise_ms),
        "rt_denoise_var": (lambda r: (lambda: r.denoise_var_device(out.data_ptr(), None)),
                           lambda r: r.last_denoise_var_ms),
        "rt_temporal": (lambda r: (lambda: r.temporal_device(out.data_ptr(), None)), lambda r: r.last_temporal_ms),
    }
    flt = {name: {"assembled": [], "full": []} for name in passes}
    for name, (call, ms) in passes.items():
        for r in (rs[0], full):
            timed(call(r), ms(r), 10)
    for rnd in range(args.pairs):
        for name, (call, ms) in passes.items():
            flt[name]["assembled"].append(timed(call(rs[0]), ms(rs[0]), args.reps))
            flt[name]["full"].append(timed(call(full), ms(full), args.reps))
        lines.append(f"round {rnd}: " + ", ".join(
            f"{name} assembled / full {flt[name]['assembled'][-1]:.4f} / {flt[name]['full'][-1]:.4f}" for name in passes))
    med = statistics.median
    for p in PLANES:
        fe, fa = floor_ms(p * RPS * W), floor_ms(p * H * W)
        lines.append(f"export of one shard, {p} planes ({8 * p * RPS * W / 1e6:.1f} MB moved): {med(ex[p]):.4f} ms = "
                     f"{med(ex[p]) / fe:.2f}x its streaming floor ({fe:.4f} ms; events around the call)")
        lines.append(f"assembly, {p} planes ({8 * p * H * W / 1e6:.1f} MB moved): {med(asm[p]):.4f} ms = "
                     f"{med(asm[p]) / fa:.2f}x its streaming floor ({fa:.4f} ms)")
    for name in passes:
        a, f = med(flt[name]["assembled"]), med(flt[name]["full"])
        lines.append(f"{name}: on the counted assembled frame {a:.4f} ms, on the full-frame adaptive context "
                     f"{f:.4f} ms ({a / f:.3f}x)")
    # the counted assembled frame is the full frame
    n, j = rs[0].assembled_counts(W, H)
    fn, fj = full.counts(H, W)
    acc = rs[0].get_assembled(W, H)
    same = acc.tobytes() == full.get_state(H, W)[1].tobytes() and np.array_equal(n, fn) and np.array_equal(j, fj)
    lines.append("assembled frameSum and counts equal the full-frame context's: " + ("yes" if same else "NO"))
    for r in rs + [full, uniform]:
        r.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
