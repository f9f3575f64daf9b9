"""Child process of tests/test_gpu_assemble_adaptive.py:
bwrt.dist.render_adaptive then bwrt.dist.gather_frame_adaptive at world size 1
over nccl (RCCL), started fresh under torch.distributed.run.  The one rank
renders the whole frame with the moments tracked, runs an adaptive call, gathers
its counted block to itself and assembles it on the device; the assembled frame
and counts must be its own accumulation's.  Exits 0 on success."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "bwidman-raytracer_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libbwrt: one shared HIP runtime)
import torch.distributed as dist  # noqa: E402

from bwrt import Renderer, scenes  # noqa: E402
from bwrt.dist import ShardPlan, gather_frame_adaptive, render_adaptive  # noqa: E402


def main():
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    w, h = 64, 36
    plan = ShardPlan(h, dist.get_world_size(), dist.get_rank())
    ok = True
    with Renderer(0) as r:
        r.set_scene(scenes.scene_07())
        r.set_moments(True)
        r.set_adaptive_filters(True)
        for i, k in enumerate((2, 2, 3)):
            r.render(w, h, k, 4, first_frame=1 if i == 0 else 0, row_offset=plan.row_offset,
                     row_stride=plan.row_stride)
        for stream in (None, torch.cuda.Stream()):
            render_adaptive(r, plan, w, 4, stream=stream, samples=2, tolerance=0.1, lum_floor=0.01, radius=2)
            for planes in (7, 4):
                r.assemble_drop()
                assert gather_frame_adaptive(r, plan, w, planes=planes, stream=stream) is True
                assert r.assembled() == (7, 3 if planes == 7 else 0), r.assembled()
                n, j = r.assembled_counts(w, h)  # (waits for the assembly)
                wn, wj = r.counts(h, w)
                ok = ok and len(np.unique(wn)) >= 2 and np.array_equal(n, wn)
                ok = ok and np.array_equal(j, wj if planes == 7 else np.zeros_like(wj))
                acc = r.get_assembled(w, h)
                ok = ok and acc.tobytes() == r.get_state(h, w)[1].tobytes()
                if planes == 7:
                    mom = r.get_assembled(w, h, want_moments=True)[1]
                    ok = ok and mom[..., 0].tobytes() == r.variance(h, w, want_lum=True)[1].tobytes()
    dist.barrier()
    dist.destroy_process_group()
    print("counted assembled frame equals the accumulation" if ok else "counted assembled frame DIFFERS", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
