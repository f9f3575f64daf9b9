#!/usr/bin/env python3
"""Cost of assembling row shards into one frame on GPU 0:
tools/time_assemble.py [--out FILE] [--pairs 3] [--reps 50]

Headline frame (scene 07, 1920x1080, 4 bounces, 8 one-frame render calls with
the moments tracked) as 8 row shards held by 8 contexts on the one GPU, and the
same frame on one full-frame context.

Export: rt_export_shard_device of one shard (135 rows) with 3 and with 5
planes, timed with device events around the call on a caller's stream.
Assembly: rt_assemble_device of the 8 gathered blocks with 3 and with 5 planes
(rt_last_assemble_ms).  Each against its streaming floor: every float is read
once and written once, so 8 B x floats moved at 6.3 TB/s.  Filter: rt_denoise
(5 levels) on the shard context that holds the assembled frame against
rt_denoise on the full-frame context, alternating.  10 warm-up calls, then
`reps` calls per point, `pairs` rounds, medians.  The summary goes to stdout
and to --out.
"""
import argparse
import os
import statistics

os.environ["BWRT_TUNING"] = "1"
import timing_common as tc  # noqa: E402
from timing_common import BOUNCES, H, W, timed  # noqa: E402

import torch  # noqa: E402

SHARDS = 8
CALLS = 8
RPS = -(-H // SHARDS)


def floor_ms(floats):
    return 8 * floats / 6.3e12 * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    lines = [f"scene 07 {W}x{H}, {CALLS} one-frame calls, {BOUNCES} bounces, {SHARDS} row shards on one GPU; "
             f"{args.reps} per point, median ms"]
    rs = [tc.make() for _ in range(SHARDS)]
    full = tc.make()
    for i, r in enumerate(rs + [full]):
        r.set_moments(True)
        for k in range(CALLS):
            if r is full:
                r.render(W, H, 1, BOUNCES, first_frame=1 if k == 0 else 0)
            else:
                r.render(W, H, 1, BOUNCES, first_frame=1 if k == 0 else 0, row_offset=i, row_stride=SHARDS)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    gathered = {p: torch.zeros((SHARDS, p, RPS, W), dtype=torch.float32, device="cuda") for p in (3, 5)}
    out = tc.output_buffer()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    counts = {}

    def export_ms(i, planes):
        e0.record(stream)
        counts[planes] = rs[i].export_shard_device(gathered[planes][i].data_ptr(), RPS, planes, sp)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def assemble(planes):
        n, j = counts[planes]
        return lambda: rs[0].assemble_device(gathered[planes].data_ptr(), SHARDS, RPS, planes, n, j, sp)

    for p in (3, 5):  # every block, then the warm-ups
        for i in range(SHARDS):
            export_ms(i, p)
        for _ in range(10):
            export_ms(0, p)
        timed(assemble(p), rs[0].last_assemble_ms, 10)
    assert counts[5] == (CALLS, CALLS), counts

    def denoise(r):
        return lambda: r.denoise_device(out.data_ptr(), None, iterations=5)

    timed(denoise(rs[0]), rs[0].last_denoise_ms, 10)
    timed(denoise(full), full.last_denoise_ms, 10)
    ex = {3: [], 5: []}
    asm = {3: [], 5: []}
    dn = {"assembled": [], "full": []}
    for rnd in range(args.pairs):
        for p in (3, 5):
            ex[p].append(statistics.median(export_ms(0, p) for _ in range(args.reps)))
            asm[p].append(timed(assemble(p), rs[0].last_assemble_ms, args.reps))
        dn["assembled"].append(timed(denoise(rs[0]), rs[0].last_denoise_ms, args.reps))
        dn["full"].append(timed(denoise(full), full.last_denoise_ms, args.reps))
        lines.append(f"round {rnd}: export 3/5 planes {ex[3][-1]:.4f} / {ex[5][-1]:.4f}, assembly 3/5 planes "
                     f"{asm[3][-1]:.4f} / {asm[5][-1]:.4f}, rt_denoise assembled / full "
                     f"{dn['assembled'][-1]:.4f} / {dn['full'][-1]:.4f}")
    med = statistics.median
    for p in (3, 5):
        fe, fa = floor_ms(p * RPS * W), floor_ms(p * H * W)
        lines.append(f"export of one shard, {p} planes ({8 * p * RPS * W / 1e6:.1f} MB moved): {med(ex[p]):.4f} ms = "
                     f"{med(ex[p]) / fe:.2f}x its streaming floor ({fe:.4f} ms; events around the call)")
        lines.append(f"assembly, {p} planes ({8 * p * H * W / 1e6:.1f} MB moved): {med(asm[p]):.4f} ms = "
                     f"{med(asm[p]) / fa:.2f}x its streaming floor ({fa:.4f} ms)")
    lines.append(f"rt_denoise, 5 levels: on the assembled frame {med(dn['assembled']):.4f} ms, on the full-frame "
                 f"context {med(dn['full']):.4f} ms ({med(dn['assembled']) / med(dn['full']):.3f}x)")
    # the assembled frame is the full frame
    acc = rs[0].get_assembled(W, H)
    lines.append("assembled frameSum equals the full-frame context's: "
                 + ("yes" if acc.tobytes() == full.get_state(H, W)[1].tobytes() else "NO"))
    for r in rs + [full]:
        r.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
