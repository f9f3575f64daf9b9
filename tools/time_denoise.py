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
import sys

os.environ["BWRT_TUNING"] = "1"
sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd")]
import torch  # noqa: E402,F401  (one HIP runtime with libbwrt)

from bwrt import Renderer, scenes  # noqa: E402

W, H, FRAMES, BOUNCES, LEVELS = 1920, 1080, 8, 4, 5
FLOOR_MS = (48 + 16) * W * H / 6.3e12 * 1e3


def make(variant):
    if variant:
        os.environ["BWRT_DENOISE_KERNEL"] = variant
    else:
        os.environ.pop("BWRT_DENOISE_KERNEL", None)
    r = Renderer(0)
    r.set_scene(scenes.scene_07())
    r.render(W, H, FRAMES, BOUNCES, first_frame=1)
    return r


def timed(r, buf, levels, reps):
    ts = []
    for _ in range(reps):
        r.denoise_device(buf.data_ptr(), None, iterations=levels)
        ts.append(r.last_denoise_ms())
    return statistics.median(ts)


def main():
    global LEVELS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--levels", type=int, default=LEVELS, help="level counts timed (6 adds step 32)")
    args = ap.parse_args()
    LEVELS = args.levels
    buf = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
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
    r = ctx[None]
    ks = []
    for _ in range(12):
        r.render(W, H, FRAMES, BOUNCES, first_frame=1)
        ks.append(r.last_kernel_ms())
    step = statistics.median(ks[2:])
    for v in ("direct", "tiled", None):
        m = statistics.median(total[v])
        lines.append(f"{v or 'policy':6s}: {LEVELS} levels {m:.4f} ms = {m / step:.3f} of the render step ({step:.4f} ms)")
    for r in ctx.values():
        r.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
