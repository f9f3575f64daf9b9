#!/usr/bin/env python3
"""Cost of one adaptive render call on row shards, per rank, against the
single-context adaptive call and the uniform shard render it replaces, in the
same job: tools/time_adaptive_multi.py [--out FILE] [--pairs 3] [--reps 20]

Headline frame (scene 07, 1920x1080, 4 bounces) as 8 shard contexts on GPU 0
(rank r holds rows r, r + 8, ...; N contexts on one GPU stand in for N GPUs),
each accumulated as 4 calls x 2 frames with tracking on.  A point is that start
followed by one call of 8 frames.  Everything is queued on one stream, so a
rank's figures are that rank's alone:
  sharded  rt_adaptive_export_rows_device on every rank (phase 1, bracketed by
           events on the stream), then rt_render_adaptive_shard_device on every
           rank with its three stages from rt_adaptive_last_stats: selection
           (count fill, sharded test, scan, scatter), the list render kernel,
           update + resolve
  single   rt_render_adaptive_device on one context that holds the whole frame
           (its selection includes the row sums, which are phase 1 above)
  uniform  rt_render_device of 8 frames continuing the accumulation, per rank
           (rt_last_kernel_ms: render kernel + moment update)
Warm-ups, then `reps` timed points; the three alternate within a round, `pairs`
rounds, medians of the rounds' medians.  The blocks are written straight into
one gathered buffer: the all-gather itself (12 bytes per frame pixel to every
rank) moves nothing inside one device and is not part of these figures.  The
summary goes to stdout and to --out.
"""
import argparse
import os
import statistics

os.environ["BWRT_TUNING"] = "1"
import timing_common as tc  # noqa: E402
from timing_common import BOUNCES, H, W  # noqa: E402

import torch  # noqa: E402

START = (2, 2, 2, 2)
K = 8
SHARDS = 8
RPS = -(-H // SHARDS)
STAGES = ("export", "select", "render", "resolve", "uniform")


def rows_of(i):
    return len(range(i, H, SHARDS))


def start(r, buf, off=0, stride=1):
    # reseeded: every point renders the same frames, so the ranks select, together, what the single context selects
    r.init_rand(W, H, off, stride)
    r.set_moments(True)
    for i, k in enumerate(START):
        r.render_device(r.params(W, H, k, BOUNCES, first_frame=1 if i == 0 else 0, row_offset=off, row_stride=stride),
                        buf.data_ptr(), None)


def sharded_point(rs, bufs, gathered, stream):
    """Per rank {export, select, render, resolve} ms of one sharded call."""
    sp = stream.cuda_stream
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in rs]
    for i, r in enumerate(rs):
        start(r, bufs[i], i, SHARDS)
    for i, r in enumerate(rs):
        r.synchronize()  # the start ran on the context's stream: the export's bracket holds the export alone
        ev[i][0].record(stream)
        r.adaptive_export_rows_device(gathered[i].data_ptr(), RPS, sp, samples=K)
        ev[i][1].record(stream)
    for i, r in enumerate(rs):
        r.render_adaptive_shard_device(gathered.data_ptr(), SHARDS, RPS, bufs[i].data_ptr(), sp, BOUNCES, samples=K)
    out = []
    for i, r in enumerate(rs):
        st = r.adaptive_stats()
        out.append({"kernel": r.last_kernel_name(), "export": ev[i][0].elapsed_time(ev[i][1]), "select": st["select_ms"],
                    "render": st["render_ms"], "resolve": st["resolve_ms"], "selected": st["selected"]})
    return out


def uniform_point(rs, bufs):
    out = []
    for i, r in enumerate(rs):
        start(r, bufs[i], i, SHARDS)
        r.render_device(r.params(W, H, K, BOUNCES, row_offset=i, row_stride=SHARDS), bufs[i].data_ptr(), None)
        r.synchronize()
        out.append(r.last_kernel_ms())
    return out


def single_point(r, buf):
    start(r, buf)
    r.render_adaptive_device(buf.data_ptr(), None, BOUNCES, samples=K)
    return r.adaptive_stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    med = statistics.median
    buf = tc.output_buffer()
    bufs = [torch.zeros(rows_of(i) * W, dtype=torch.int32, device="cuda") for i in range(SHARDS)]
    gathered = torch.zeros((SHARDS, 3, RPS, W), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    rs = []
    for _ in range(SHARDS):
        r = tc.make()
        r.set_moments(True)
        rs.append(r)
    one = tc.make()
    one.set_moments(True)
    lines = [f"scene 07 {W}x{H}, {BOUNCES} bounces, {SHARDS} shard contexts on one GPU ({RPS} rows per block), start "
             f"{len(START)} calls x 2 frames, then {K} frames; {args.reps} per point, median ms"]
    for _ in range(5):
        uniform_point(rs, bufs)
        uniform_kernel = rs[0].last_kernel_name()
        pts = sharded_point(rs, bufs, gathered, stream)
        st1 = single_point(one, buf)
    lines.append(f"list render kernel: rank 0 {pts[0]['kernel']}, single context {one.last_kernel_name()}; uniform shard "
                 f"render: {uniform_kernel}")
    sel = sum(p["selected"] for p in pts)
    if sel != st1["selected"]:
        raise SystemExit(f"the ranks selected {sel} pixels, the single context {st1['selected']}")
    lines.append(f"selected {sel} of {W * H} pixels, over the ranks as on the single context: share {sel / (W * H):.4f}")
    # rounds[stage][rank] -> the rounds' medians; "single" -> per stage
    rounds = {s: [[] for _ in range(SHARDS)] for s in STAGES}
    single = {s: [] for s in ("select", "render", "resolve")}
    for rnd in range(args.pairs):
        sh, un, si = [], [], []
        for _ in range(args.reps):
            sh.append(sharded_point(rs, bufs, gathered, stream))
            un.append(uniform_point(rs, bufs))
            si.append(single_point(one, buf))
        for i in range(SHARDS):
            for s in STAGES[:4]:
                rounds[s][i].append(med(p[i][s] for p in sh))
            rounds["uniform"][i].append(med(u[i] for u in un))
        for s in single:
            single[s].append(med(p[s + "_ms"] for p in si))
        lines.append(f"round {rnd}: rank 0 export {rounds['export'][0][-1]:.4f}, select {rounds['select'][0][-1]:.4f}, list "
                     f"render {rounds['render'][0][-1]:.4f}, update + resolve {rounds['resolve'][0][-1]:.4f}; uniform "
                     f"{rounds['uniform'][0][-1]:.4f}; single select {single['select'][-1]:.4f}, render "
                     f"{single['render'][-1]:.4f}, resolve {single['resolve'][-1]:.4f}")
    m = {s: [med(v) for v in rounds[s]] for s in STAGES}
    lines.append("rank: phase 1 (row sums) | test + scan + scatter | list render | update + resolve | sum | uniform "
                 f"{K}-frame shard render")
    for i in range(SHARDS):
        total = sum(m[s][i] for s in STAGES[:4])
        lines.append(f"  {i}: {m['export'][i]:.4f} | {m['select'][i]:.4f} | {m['render'][i]:.4f} | {m['resolve'][i]:.4f} | "
                     f"{total:.4f} | {m['uniform'][i]:.4f}")
    worst = {s: max(m[s]) for s in STAGES}
    total = max(sum(m[s][i] for s in STAGES[:4]) for i in range(SHARDS))
    lines.append(f"slowest rank: phase 1 {worst['export']:.4f}, test + scan + scatter {worst['select']:.4f}, list render "
                 f"{worst['render']:.4f}, update + resolve {worst['resolve']:.4f}; whole call {total:.4f} ms against its "
                 f"uniform shard render {worst['uniform']:.4f} ms: {total / worst['uniform']:.3f}")
    s1 = {s: med(v) for s, v in single.items()}
    whole1 = sum(s1.values())
    lines.append(f"single context: selection (with row sums) {s1['select']:.4f}, list render {s1['render']:.4f}, update + "
                 f"resolve {s1['resolve']:.4f}; whole call {whole1:.4f} ms")
    lines.append(f"sum over the ranks / single context: selection {(sum(m['export']) + sum(m['select'])) / s1['select']:.2f}, "
                 f"list render {sum(m['render']) / s1['render']:.2f}, update + resolve "
                 f"{sum(m['resolve']) / s1['resolve']:.2f}; slowest rank's whole call / single context's "
                 f"{total / whole1:.3f} (ideal {1 / SHARDS:.3f})")
    lines.append(f"all-gather payload: {12 * W * H / 1e6:.1f} MB to every rank per call (not moved here: one device)")
    for r in rs + [one]:
        r.close()
    tc.write_out(lines, args.out)


if __name__ == "__main__":
    main()
