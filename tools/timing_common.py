"""What the timing tools share (time_denoise.py, time_denoise_var.py,
time_temporal.py): the package on the path and one HIP runtime with libbwrt,
the headline frame, a context per forced filter variant, the median of
repeated calls timed with device events, the render step for scale, and the
write-out of the summary."""
import os
import statistics
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd")]
import torch  # noqa: E402,F401  (one HIP runtime with libbwrt)

from bwrt import Renderer, scenes  # noqa: E402

W, H, FRAMES, BOUNCES = 1920, 1080, 8, 4


def floor_ms(bytes_per_pixel):
    """Streaming floor of a pass over the headline frame at 6.3 TB/s."""
    return bytes_per_pixel * W * H / 6.3e12 * 1e3


def make(variant=None):
    """A context on GPU 0 with scene 07; variant: BWRT_DENOISE_KERNEL (read at
    rt_create under BWRT_TUNING=1), None = the measured policy."""
    if variant:
        os.environ["BWRT_DENOISE_KERNEL"] = variant
    else:
        os.environ.pop("BWRT_DENOISE_KERNEL", None)
    r = Renderer(0)
    r.set_scene(scenes.scene_07())
    return r


def timed(call, ms, reps):
    """Median of ms() behind each of `reps` calls."""
    ts = []
    for _ in range(reps):
        call()
        ts.append(ms())
    return statistics.median(ts)


def render_step_ms(r):
    """The plain render step: FRAMES frames in one launch, rt_last_kernel_ms."""
    ks = []
    for _ in range(12):
        r.render(W, H, FRAMES, BOUNCES, first_frame=1)
        ks.append(r.last_kernel_ms())
    return statistics.median(ks[2:])


def output_buffer():
    buf = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return buf


def write_out(lines, out):
    """The summary to stdout and, when given, to the file `out`."""
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
