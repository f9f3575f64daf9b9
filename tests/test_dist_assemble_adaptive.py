"""bwrt.dist.gather_frame_adaptive on CPU (gloo): one process per rank renders
its interleaved rows with the moments tracked, the ranks run two adaptive calls
(bwrt.dist.render_adaptive), then gather their counted blocks to rank 0, which
assembles them and runs the variance-guided filter on the whole frame.  Its
output and the assembled counts must be one context's that ran
rt_render_adaptive on the whole frame (built like
tests/test_dist_adaptive.py)."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from bwrt.dist import ShardPlan, gather_frame_adaptive, render_adaptive

CALLS = (2, 2, 3)
BOUNCES = 4
ADAPTIVE = (dict(samples=3, tolerance=0.1, lum_floor=0.01, radius=2),
            dict(samples=2, tolerance=0.1, lum_floor=0.01, radius=3))
MIN_BATCHES = 5  # J_p is 3, 4 or 5 after the two calls: tracked and spatial pixels both occur


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
        c.set_adaptive_filters(True)
        if plan.rows > 0:
            for i, k in enumerate(CALLS):
                c.render(w, h, k, BOUNCES, first_frame=1 if i == 0 else 0, row_offset=plan.row_offset,
                         row_stride=plan.row_stride)
        for params in ADAPTIVE:
            render_adaptive(c, plan, w, BOUNCES, **params)
        out = {}
        for planes in (7, 4):
            assert gather_frame_adaptive(c, plan, w, planes) == (rank == 0)
            if rank == 0:
                assert c.assembled() == (sum(CALLS), len(CALLS) if planes == 7 else 0)
                out[planes] = (c.assembled_counts(w, h),
                               c.denoise_var(w, h, want_color=True, want_var=True, min_batches=MIN_BATCHES))
        if rank == 0:
            q.put(out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("h,world", [(55, 3), (30, 8)])
def test_rank0_filters_the_adaptive_frame(h, world):
    w = 96
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, w, h, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    from bwrt import Renderer, scenes
    with Renderer.cpu(2) as c:  # one context, the whole frame
        c.set_scene(scenes.scene_07())
        c.set_moments(True)
        c.set_adaptive_filters(True)
        for i, k in enumerate(CALLS):
            c.render(w, h, k, BOUNCES, first_frame=1 if i == 0 else 0)
        for params in ADAPTIVE:
            c.render_adaptive(w, h, BOUNCES, **params)
        n, j = c.counts(h, w)
        assert len(np.unique(n)) >= 2 and (j >= MIN_BATCHES).any() and (j < MIN_BATCHES).any()
        kw = dict(want_color=True, want_var=True)
        want = {7: c.denoise_var(w, h, min_batches=MIN_BATCHES, **kw),
                4: c.denoise_var(w, h, min_batches=int(j.max()) + 1, **kw)}  # no moments: all spatial
    assert want[7][1].tobytes() != want[4][1].tobytes()
    for planes in (7, 4):
        (gn, gj), out = got[planes]
        assert np.array_equal(gn, n) and np.array_equal(gj, j if planes == 7 else np.zeros_like(j)), planes
        for a, b in zip(out, want[planes]):
            assert a.tobytes() == b.tobytes(), planes
