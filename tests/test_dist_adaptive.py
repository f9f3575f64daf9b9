"""bwrt.dist.render_adaptive on CPU (gloo): one process per rank renders its
interleaved rows with the moments tracked, then two adaptive calls — export
the row sums, all_gather, select and render the rank's own rows.  The ranks'
counts and frameSum, interleaved, must be one context's that ran
rt_render_adaptive on the whole frame (built like tests/test_dist_assemble.py)."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from bwrt.dist import ShardPlan, render_adaptive

CALLS = (2, 2, 3)
BOUNCES = 4
ADAPTIVE = (dict(samples=3, tolerance=0.1, lum_floor=0.01, radius=2),
            dict(samples=2, tolerance=0.1, lum_floor=0.01, radius=3))


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
        if plan.rows > 0:
            for i, k in enumerate(CALLS):
                c.render(w, h, k, BOUNCES, first_frame=1 if i == 0 else 0, row_offset=plan.row_offset,
                         row_stride=plan.row_stride)
        selected = 0
        for params in ADAPTIVE:
            res = render_adaptive(c, plan, w, BOUNCES, **params)
            assert (res is None) == (plan.rows == 0)
            if res is not None:
                assert res[0].shape == (plan.rows, w, 4)
                selected += res[1]["selected"]
        if plan.rows > 0:
            q.put((rank, c.counts(plan.rows, w), c.get_state(plan.rows, w)[1], selected))
        else:
            q.put((rank, None, None, 0))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("h,world", [(55, 3), (30, 8)])
def test_ranks_equal_one_context(h, world):
    w = 96
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, w, h, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    n = np.zeros((h, w), np.uint32)
    j = np.zeros((h, w), np.uint32)
    acc = np.zeros((h, w, 3), np.float32)
    covered = np.zeros(h, bool)
    selected = 0
    for rank, counts, a, sel in got:
        if counts is not None:
            n[rank::world], j[rank::world] = counts
            acc[rank::world] = a
            covered[rank::world] = True
        selected += sel
    assert covered.all()
    from bwrt import Renderer, scenes
    with Renderer.cpu(2) as c:  # one context, the whole frame
        c.set_scene(scenes.scene_07())
        c.set_moments(True)
        for i, k in enumerate(CALLS):
            c.render(w, h, k, BOUNCES, first_frame=1 if i == 0 else 0)
        want = sum(c.render_adaptive(w, h, BOUNCES, **params)[1]["selected"] for params in ADAPTIVE)
        assert 0 < want < 2 * w * h and selected == want
        wn, wj = c.counts(h, w)
        assert np.array_equal(n, wn) and np.array_equal(j, wj)
        assert acc.tobytes() == c.get_state(h, w)[1].tobytes()
