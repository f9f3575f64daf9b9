"""gather_frame on CPU (gloo): one process per rank renders its interleaved
rows with the moments tracked, the ranks' blocks {frameSum, M, M2} are gathered
to rank 0 and assembled there, and rank 0's variance-guided filter must give
the bits of one context that rendered the whole frame (built like
tests/test_dist.py)."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from bwrt.dist import ShardPlan, gather_frame

CALLS = (2, 2, 3)
BOUNCES = 4


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, w, h, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(os.path.dirname(here), "bwidman-raytracer_amd")]
    from bwrt import Renderer, scenes
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    plan = ShardPlan(h, world, rank)
    with Renderer.cpu(1) as c:
        c.set_scene(scenes.scene_07())
        c.set_moments(True)
        for i, k in enumerate(CALLS):
            c.render(w, h, k, BOUNCES, first_frame=1 if i == 0 else 0, row_offset=plan.row_offset,
                     row_stride=plan.row_stride)
        root = gather_frame(c, plan, w, planes=5)
        assert root == (rank == 0)
        if root:
            assert c.assembled() == (sum(CALLS), len(CALLS))
            q.put((c.get_assembled(w, h), c.denoise_var(w, h, min_batches=2)))
        else:
            assert c.assembled() is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("h,world", [(55, 3), (30, 8)])
def test_gather_frame_feeds_the_filter(h, world):
    w = 96
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, w, h, q)) for r in range(world)]
    for p in procs:
        p.start()
    acc, rgba = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    from bwrt import Renderer, scenes
    with Renderer.cpu(2) as c:  # one context, the whole frame
        c.set_scene(scenes.scene_07())
        c.set_moments(True)
        for i, k in enumerate(CALLS):
            c.render(w, h, k, BOUNCES, first_frame=1 if i == 0 else 0)
        assert acc.tobytes() == c.get_state(h, w)[1].tobytes()
        assert np.array_equal(rgba, c.denoise_var(w, h, min_batches=2))
        assert not np.array_equal(rgba, c.denoise_var(w, h, min_batches=4))  # (the tracked variance was used)
