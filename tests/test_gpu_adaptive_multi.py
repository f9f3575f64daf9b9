"""Adaptive sampling on row shards on the MI355X: GPU
shard contexts against the GPU full-frame context bit for bit, and against the
CPU backend (NaN sign bits differ between the backends: same_values).  One
process, at most 8 shard contexts on one device; tests/test_adaptive_multi.py
checks the CPU backend against rt_render_adaptive.
"""
import numpy as np
import pytest

import adaptive_multi_case as M
from bwrt import Renderer, render_adaptive_multi, scenes

pytestmark = pytest.mark.gpu


def check(lib, name, w, h, shards, seq, bounces=M.BOUNCES, cpu=True):
    got = M.run_shards(lib, name, w, h, shards, seq, gpu=True, bounces=bounces)
    want = M.oracle(lib, name, w, h, seq, gpu=True, bounces=bounces)
    M.assert_same(got, want)
    if cpu:
        M.assert_same(got, M.oracle(lib, name, w, h, seq, bounces=bounces), eq=M.same_values)
    return want


@pytest.mark.parametrize("shards", [2, 3, 8])
def test_shards_equal_the_full_frame_and_the_cpu(bwrt_lib, shards):
    w, h = 67, 45
    want = check(bwrt_lib, "07", w, h, shards, M.sequence(2))
    assert 0 < want["calls"][0]["selected"] < w * h


@pytest.mark.parametrize("radius", [0, 4])
def test_radii(bwrt_lib, radius):
    check(bwrt_lib, "07", 67, 45, 3, M.sequence(radius))


def test_lists_over_several_groups(bwrt_lib):
    """333x187 with 2 shards: a shard's list spans several 256-lane groups."""
    w, h = 333, 187
    want = check(bwrt_lib, "07", w, h, 2, M.sequence(2))
    assert want["calls"][0]["selected"] > 4 * 256


def test_ranks_beyond_the_height(bwrt_lib):
    want = check(bwrt_lib, "07", 5, 3, 8, M.sequence(2, min_frames=9))
    assert want["calls"][0]["selected"] == 15


def test_bvh_scene(bwrt_lib):
    """The stress scene at 96x54 with 8 shards: lists that are empty or shorter than a wave."""
    check(bwrt_lib, "stress", 96, 54, 8, M.sequence(2))


def test_max_bounces_12(bwrt_lib):
    check(bwrt_lib, "07", 67, 45, 3, M.sequence(2), bounces=12)


@pytest.mark.parametrize("shards,extra", [(1, 2), (2, 0), (3, 3)])
def test_row_sum_blocks_equal_the_cpu(bwrt_lib, shards, extra):
    """Phase 1 alone: the blocks' words against the CPU backend's, the padding
    rows (one by the geometry, `extra` more by the caller's choice) zero, in the
    uniform state and behind an adaptive call."""
    w, h = 67, 45
    rps = -(-h // shards) + extra
    assert M.rows_of(h, shards, shards - 1) < rps  # the last shard has padding rows
    blocks = []
    for gpu in (True, False):
        rs = M.contexts(bwrt_lib, scenes.scene_07(), w, h, shards, gpu=gpu)
        got = [M.export_all(rs, w, h, dict(M.DEFAULTS, samples=3), rps)]
        M.two_phase(rs, w, h, dict(M.DEFAULTS, samples=3))
        got.append(M.export_all(rs, w, h, dict(M.DEFAULTS, samples=1, radius=4), rps))
        blocks.append(got)
        M.close(rs)
    for g, c in zip(*blocks):
        assert M.same(g.view(np.uint32), c.view(np.uint32))  # finite sums and integers: bit for bit
        for i in range(shards):
            rows = M.rows_of(h, shards, i)
            assert (g[i, :, rows:].view(np.uint32) == 0).all()
            assert g[i, 2, :rows].view(np.int32).min() >= 1


def multi_call(rs, w, h, p, bounces):
    rgba, st = render_adaptive_multi(rs, w, h, bounces, **p)
    assert st["select_ms"] > 0 and st["render_ms"] > 0 and st["resolve_ms"] > 0
    return {"rgba": rgba, "selected": st["selected"], "frames_total": st["frames_total"]}


@pytest.mark.parametrize("w,h,shards", [(67, 45, 3), (5, 3, 8)])
def test_multi_equals_the_full_frame(bwrt_lib, w, h, shards):
    seq = M.sequence(2, min_frames=9 if h == 3 else 0)
    want = M.oracle(bwrt_lib, "07", w, h, seq, gpu=True)
    got = M.run_shards(bwrt_lib, "07", w, h, shards, seq, gpu=True, call=multi_call)
    for a, b in zip(got["calls"], want["calls"]):
        assert a["selected"] == b["selected"] and a["frames_total"] == b["frames_total"]
        assert M.same(a["rgba"], b["rgba"])
    for k in want["final"]:
        assert M.same(got["final"][k], want["final"][k]), k


@pytest.mark.parametrize("own_stream", [False, True])
def test_device_entry_points(bwrt_lib, own_stream):
    """rt_adaptive_export_rows_device and rt_render_adaptive_shard_device with an
    rt_render_device queued directly before them and a restarting render
    (first_frame 1) directly behind, on a caller's stream (every context on the
    same one: the stream orders the phases) and on the contexts' own streams
    (the caller orders the gather: a synchronisation between the phases)."""
    import torch
    lib, w, h, s = bwrt_lib, 67, 45, 2
    scene = scenes.scene_07()
    seq = M.sequence(2, ks=(3, 2))
    (c,) = M.contexts(lib, scene, w, h, 1)
    img_mid = [M.full_call(c, w, h, p) for p in seq][-1]["rgba"]
    mid = M.snapshot([c], w, h)
    c.render_adaptive(w, h, M.BOUNCES, samples=1, tolerance=1e30)  # selects nothing
    restart_want = c.render(w, h, 2, M.BOUNCES, first_frame=1)
    end = M.snapshot([c], w, h, variance=False)  # one batch behind the restart: no variance yet
    c.close()

    rps = -(-h // s)
    rs = []
    for i in range(s):
        g = Renderer(0, lib=lib)
        g.set_scene(scene)
        g.set_moments(True)
        rs.append(g)
    stream = torch.cuda.Stream()
    gathered = torch.zeros((s, 3, rps, w), dtype=torch.float32, device="cuda")
    bufs = [torch.zeros(M.rows_of(h, s, i) * w, dtype=torch.int32, device="cuda") for i in range(s)]
    bufs2 = [torch.zeros_like(b) for b in bufs]
    torch.cuda.synchronize()
    sp = None if own_stream else stream.cuda_stream

    def settle():
        if own_stream:
            for g in rs:
                g.synchronize()

    for i, g in enumerate(rs):
        for k, n in enumerate(M.CALLS):
            g.render_device(g.params(w, h, n, M.BOUNCES, first_frame=1 if k == 0 else 0, row_offset=i, row_stride=s),
                            bufs[i].data_ptr(), sp)
    for p in seq:
        for i, g in enumerate(rs):
            g.adaptive_export_rows_device(gathered[i].data_ptr(), rps, sp, **p)
        settle()
        for i, g in enumerate(rs):
            g.render_adaptive_shard_device(gathered.data_ptr(), s, rps, bufs[i].data_ptr(), sp, M.BOUNCES, **p)
        settle()
    got_mid = M.snapshot(rs, w, h)  # waits for the calls
    stats = [g.adaptive_stats() for g in rs]
    assert all(st["select_ms"] > 0 and st["render_ms"] > 0 and st["resolve_ms"] > 0 for st in stats)
    img = np.empty((h, w, 4), np.uint8)
    for i in range(s):
        img[i::s] = bufs[i].cpu().numpy().view(np.uint8).reshape(-1, w, 4)
    for i, g in enumerate(rs):  # directly behind each other: an export, its phase 2, a restarting render
        g.adaptive_export_rows_device(gathered[i].data_ptr(), rps, sp, samples=1, tolerance=1e30)
    settle()
    for i, g in enumerate(rs):
        g.render_adaptive_shard_device(gathered.data_ptr(), s, rps, bufs[i].data_ptr(), sp, M.BOUNCES, samples=1,
                                       tolerance=1e30)
        g.render_device(g.params(w, h, 2, M.BOUNCES, first_frame=1, row_offset=i, row_stride=s), bufs2[i].data_ptr(), sp)
    got_end = M.snapshot(rs, w, h, variance=False)
    for g in rs:
        g.synchronize()
    stream.synchronize()
    img_end = np.empty((h, w, 4), np.uint8)
    for i in range(s):
        img_end[i::s] = bufs2[i].cpu().numpy().view(np.uint8).reshape(-1, w, 4)
    M.close(rs)
    for k in mid:
        assert M.same_values(got_mid[k], mid[k]), k
    for k in end:
        assert M.same_values(got_end[k], end[k]), k
    assert np.array_equal(img, img_mid)
    assert np.array_equal(img_end, restart_want)


def test_forced_kernels_equal_the_policy(bwrt_lib, monkeypatch):
    w, h, s, seq = 67, 45, 3, M.sequence(2)
    want = M.oracle(bwrt_lib, "07", w, h, seq, gpu=True)
    for which, kernel in (("simple", "rt_render_kernel<"), ("queued", "rt_render_list_kernel<")):
        monkeypatch.setenv("BWRT_ADAPTIVE_KERNEL", which)
        rs = M.contexts(bwrt_lib, scenes.scene_07(), w, h, s, gpu=True)
        got = {"calls": [M.two_phase(rs, w, h, p) for p in seq], "final": M.snapshot(rs, w, h)}
        names = [r.last_kernel_name() for r in rs]
        M.close(rs)
        assert all(n.startswith(kernel) and "list" in n for n in names), names
        M.assert_same(got, want)


def test_five_identical_sequences(bwrt_lib):
    w, h, seq = 333, 187, M.sequence(2)
    runs = [M.run_shards(bwrt_lib, "07", w, h, 2, seq, gpu=True) for _ in range(5)]
    for other in runs[1:]:
        M.assert_same(other, runs[0])
