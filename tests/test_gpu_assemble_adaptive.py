"""Counted assembled frames on the MI355X: the HIP kernels
behind rt_export_shard_adaptive and rt_assemble_adaptive against the CPU
backend (both are copies with the indexing of csrc/rt_assemble.h), the three
passes on the counted frame against one GPU context that ran rt_render_adaptive
on the whole frame, bit for bit, the device-stream entry points,
rt_assemble_adaptive_multi behind rt_render_adaptive_multi and
bwrt.dist.gather_frame_adaptive over nccl.  tests/test_assemble_adaptive.py
checks the CPU backend against its own full-frame context.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import adaptive_multi_case as M
import assemble_adaptive_case as K
from bwrt import Renderer, abi, assemble_adaptive_multi, render_adaptive_multi

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (scene, width, height, shards): the 4-byte form with uneven shards; rows of whole 16-byte groups; many
# workgroups on the 4-byte form; contexts beyond the height; the BVH scene's guides
SHAPES = [("07", 67, 45, 2), ("07", 67, 45, 3), ("07", 67, 45, 8), ("07", 256, 64, 2), ("07", 333, 187, 8),
          ("07", 5, 3, 8), ("stress", 96, 54, 8)]


def blocks_equal(a, b, planes):
    """Float planes by value (a GPU and a CPU render give NaNs of different
    sign bits), count planes word for word."""
    nf = 3 if planes == 4 else 5
    return K.same_values(a[:, :nf], b[:, :nf]) and K.same(a[:, nf:], b[:, nf:])


def pad_with_nans(g, h):
    """One more row per block than needed, every padding row NaN bit patterns."""
    s, planes, rps, w = g.shape
    out = np.empty((s, planes, rps + 1, w), np.float32)
    out.view(np.uint32)[...] = 0x7fc00321
    for i in range(s):
        rows = K.rows_of(h, s, i)
        out[i, :, :rows] = g[i, :, :rows]
    return out


def temporal_of(r, w, h):
    return r.temporal(w, h, denoise={"iterations": 2}, want_color=True, want_length=True)


# ---- 1. the kernels against the CPU backend, the passes against the GPU full-frame context ----------------
@pytest.mark.parametrize("name,w,h,s", SHAPES)
def test_gpu_shards_equal_full_frame_and_cpu(bwrt_lib, name, w, h, s):
    seq = K.sequence(w, h, 1)
    gs = K.shards_after(bwrt_lib, name, w, h, s, seq, gpu=True)
    cs = K.shards_after(bwrt_lib, name, w, h, s, seq)
    full = K.full_after(bwrt_lib, name, w, h, seq, gpu=True)
    try:
        want = K.frame_of(full, w, h)
        if (w, h) == (5, 3):
            mixed = 4  # (every pixel forced: one J_p)
        else:
            assert len(np.unique(want["n"])) >= 2
            mixed = K.mixed_min_batches(want["j"])
        want_f = K.filter_outputs(full, w, h, mixed)
        for planes in (4, 7):
            gg, n, j = K.gather(gs, w, h, planes)
            cg, cn, cj = K.gather(cs, w, h, planes)
            assert (n, j) == (cn, cj) == K.BASE
            assert blocks_equal(gg, cg, planes), planes  # the exported blocks' words, zero padding included
            big = K.gather(gs, w, h, planes, rows_per_shard=gg.shape[2] + 1)[0]
            assert blocks_equal(big, K.gather(cs, w, h, planes, rows_per_shard=gg.shape[2] + 1)[0], planes)
            for i in range(min(s, h)):
                assert not big[i, :, K.rows_of(h, s, i):].view(np.uint32).any()  # zero words
            frames = []
            for r, g in ((gs[0], pad_with_nans(gg, h)), (gs[0], gg), (cs[0], cg)):
                r.assemble_adaptive(g, n, j)
                assert r.assembled() == (n, j if planes == 7 else 0)
                frames.append(K.assembled_of(r, w, h, planes))
            assert gs[0].last_assemble_ms() > 0
            # within the GPU backend bit for bit: the padded and the plain blocks, and the full-frame context
            assert K.same(frames[0], frames[1]), planes
            for key in frames[1]:
                if not (key == "j" and planes == 4):
                    assert K.same(frames[1][key], want[key]), (planes, key)
            assert K.same_values(frames[1], frames[2]), planes
            got = K.filter_outputs(gs[0], w, h, mixed, planes)
            exp = K.expected(want_f, planes)
            cpu = K.filter_outputs(cs[0], w, h, mixed, planes)
            for key in got:
                assert K.same(got[key], exp[key]), (planes, key)
                assert K.same_values(got[key], cpu[key]), (planes, key)
            gs[0].temporal_reset()
            full.temporal_reset()
            assert K.same(temporal_of(gs[0], w, h), temporal_of(full, w, h)), planes
    finally:
        M.close(gs + cs + [full])


def test_gpu_temporal_over_two_views(bwrt_lib):
    name, w, h, s = "07", 67, 45, 3
    (p,) = K.sequence(w, h, 1)
    full = M.contexts(bwrt_lib, M.scene_of(name), w, h, 1, gpu=True)
    gs = M.contexts(bwrt_lib, M.scene_of(name), w, h, s, gpu=True)
    try:
        for r in full + gs:
            r.set_adaptive_filters(True)
        want = K.temporal_outputs(full, w, h, p)
        got = K.temporal_outputs(gs, w, h, p, assemble=lambda: K.assemble_on(gs, w, h, 4))
        for i, (a, b) in enumerate(zip(got, want)):
            assert K.same(a, b), i
        assert want[2][2].max() > K.BASE[0] and len(np.unique(want[0][2])) >= 2
    finally:
        M.close(full + gs)


def test_unaligned_pointer_takes_the_4_byte_path(bwrt_lib):
    """width % 4 == 0, but `gathered_device` and a block 4 bytes off a 16-byte boundary."""
    import torch
    name, w, h, s = "07", 64, 36, 8
    gs = K.shards_after(bwrt_lib, name, w, h, s, K.sequence(w, h, 1), gpu=True)
    try:
        for planes in (7, 4):
            g, n, j = K.assemble_on(gs, w, h, planes)
            want = K.bits(K.assembled_of(gs[0], w, h, planes))
            for off in (0, 1):
                gs[0].assemble_drop()
                buf = torch.zeros(g.size + 4, dtype=torch.float32, device="cuda")
                buf[off:off + g.size] = torch.from_numpy(g.reshape(-1)).cuda()
                assert buf.data_ptr() % 16 == 0
                blk = torch.zeros(g[0].size + 4, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                gs[0].assemble_adaptive_device(buf.data_ptr() + 4 * off, s, g.shape[2], planes, n, j)
                assert K.bits(K.assembled_of(gs[0], w, h, planes)) == want, (planes, off)
                gs[1].export_shard_adaptive_device(blk.data_ptr() + 4 * off, g.shape[2], planes)
                gs[1].synchronize()
                host = blk.cpu().numpy()
                assert K.same(host[off:off + g[0].size].reshape(g[0].shape), g[1]), (planes, off)
                assert not host[off + g[0].size:].view(np.uint32).any()  # nothing past the block
                assert not host[:off].view(np.uint32).any()              # nor before it
        bad = abi.RT_ERR_INVALID_ARGUMENT
        lib = bwrt_lib
        assert lib.rt_assemble_adaptive_device(gs[0].ctx, buf.data_ptr() + 2, s, g.shape[2], 4, n, j, None) == bad
        assert lib.rt_export_shard_adaptive_device(gs[1].ctx, g.shape[2], 4, blk.data_ptr() + 2, None, None, None) == bad
    finally:
        M.close(gs)


def test_capped_grid_gives_the_same_bits(monkeypatch, bwrt_lib):
    """BWRT_DEINT_BLOCKS=1: one workgroup strides over every item (read at rt_create, BWRT_TUNING=1)."""
    name, w, h, s = "07", 67, 45, 3
    seq = K.sequence(w, h, 1)
    ref = K.shards_after(bwrt_lib, name, w, h, s, seq, gpu=True)
    monkeypatch.setenv("BWRT_TUNING", "1")
    monkeypatch.setenv("BWRT_DEINT_BLOCKS", "1")
    gs = K.shards_after(bwrt_lib, name, w, h, s, seq, gpu=True)
    try:
        for planes in (7, 4):
            outs = []
            for rs in (gs, ref):
                g, n, j = K.assemble_on(rs, w, h, planes)
                outs.append((g, K.assembled_of(rs[0], w, h, planes)))
            assert K.same(*outs), planes
    finally:
        M.close(gs + ref)


# ---- 2. the _device forms -------------------------------------------------------------------------------
@pytest.mark.parametrize("own_stream", [True, False])
def test_device_chain_without_host_sync(bwrt_lib, own_stream):
    """Render, the two phases of an adaptive call, counted export, concatenate, assemble and two filters
    queued back to back on one stream (context 0's own, or a caller's torch stream), five times over."""
    import torch
    name, w, h, s = "07", 64, 36, 4
    rps = -(-h // s)
    (p,) = K.sequence(w, h, 1)
    cs = K.shards_after(bwrt_lib, name, w, h, s, [p])
    gs = [Renderer(0, lib=bwrt_lib) for _ in range(s)]
    try:
        K.assemble_on(cs, w, h, 7)
        mixed = K.mixed_min_batches(cs[0].assembled_counts(w, h)[1])
        want_dn = cs[0].denoise(w, h)
        want_dv = cs[0].denoise_var(w, h, min_batches=mixed)
        want_cnt = cs[0].assembled_counts(w, h)
        for g in gs:
            g.set_scene(M.scene_of(name))
            g.set_moments(True)
            g.set_adaptive_filters(True)
        tstream = torch.cuda.ExternalStream(gs[0].stream_handle()) if own_stream else torch.cuda.Stream()
        sp = tstream.cuda_stream
        raws = [torch.zeros(rps * w, dtype=torch.int32, device="cuda") for _ in range(s)]
        rowsums = torch.zeros((s, 3, rps, w), dtype=torch.float32, device="cuda")
        blocks = [torch.zeros((7, rps, w), dtype=torch.float32, device="cuda") for _ in range(s)]
        out_dn, out_dv = (torch.zeros(h * w, dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()  # (the zero fills ran on torch's default stream, unordered with `tstream`)
        runs = []
        for _ in range(5):
            for i, g in enumerate(gs):
                g.init_rand(w, h, i, s)  # the seeds of frame 1: every sequence renders the same frames
            for i, g in enumerate(gs):
                for k, frames in enumerate(M.CALLS):
                    g.render_device(g.params(w, h, frames, M.BOUNCES, 1 if k == 0 else 0, i, s), raws[i].data_ptr(), sp)
                g.adaptive_export_rows_device(rowsums[i].data_ptr(), rps, sp, **p)
            for i, g in enumerate(gs):
                g.render_adaptive_shard_device(rowsums.data_ptr(), s, rps, raws[i].data_ptr(), sp, M.BOUNCES, **p)
                assert g.export_shard_adaptive_device(blocks[i].data_ptr(), rps, 7, sp) == K.BASE
            with torch.cuda.stream(tstream):
                gathered = torch.cat(blocks)
            gs[0].assemble_adaptive_device(gathered.data_ptr(), s, rps, 7, *K.BASE, sp)
            gs[0].denoise_device(out_dn.data_ptr(), sp)
            gs[0].denoise_var_device(out_dv.data_ptr(), sp, min_batches=mixed)
            tstream.synchronize()
            dn = out_dn.cpu().numpy().view(np.uint8).reshape(h, w, 4)
            dv = out_dv.cpu().numpy().view(np.uint8).reshape(h, w, 4)
            assert np.array_equal(dn, want_dn) and np.array_equal(dv, want_dv)
            cnt = gs[0].assembled_counts(w, h)
            assert K.same(cnt, want_cnt)
            runs.append(K.bits((dn, dv, cnt, gs[0].get_assembled(w, h, want_moments=True))))
            assert gs[0].last_assemble_ms() > 0
        assert all(r == runs[0] for r in runs[1:])
    finally:
        M.close(gs + cs)


# ---- 3. rt_assemble_adaptive_multi behind rt_render_adaptive_multi -----------------------------------------
@pytest.mark.parametrize("n", [3, 8])
def test_assemble_adaptive_multi_after_render_adaptive_multi(bwrt_lib, n):
    name, w, h = "07", 67, 45
    seq = M.sequence(2, ks=(3, 1))
    full = K.full_after(bwrt_lib, name, w, h, seq, gpu=True)
    rs = M.contexts(bwrt_lib, M.scene_of(name), w, h, n, gpu=True)
    dst = n - 1 if n == 3 else 0
    try:
        for p in seq:
            render_adaptive_multi(rs, w, h, M.BOUNCES, **p)
        for r in rs:
            r.set_adaptive_filters(True)
        want = K.frame_of(full, w, h)
        mixed = K.mixed_min_batches(want["j"])
        want_f = K.filter_outputs(full, w, h, mixed)
        for planes in (0, 4):
            assert assemble_adaptive_multi(rs, planes, dst) == (K.BASE[0], 0 if planes == 4 else K.BASE[1])
            assert rs[dst].last_assemble_ms() > 0
            p = planes or 7
            got = K.assembled_of(rs[dst], w, h, p)
            for key in got:
                if not (key == "j" and p == 4):
                    assert K.same(got[key], want[key]), (planes, key)
            got = K.filter_outputs(rs[dst], w, h, mixed, p)
            exp = K.expected(want_f, p)
            for key in got:
                assert K.same(got[key], exp[key]), (planes, key)
    finally:
        M.close([full] + rs)


# ---- 4. gather_frame_adaptive over nccl --------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_gather_frame_adaptive_over_nccl_one_rank():
    """World size 1 under torch.distributed.run, one fresh child process (tests/assemble_adaptive_nccl_child.py)."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
                        "--master-addr=127.0.0.1", f"--master-port={_free_port()}",
                        os.path.join(REPO, "tests", "assemble_adaptive_nccl_child.py")],
                       env=env, cwd=REPO, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "counted assembled frame equals the accumulation" in r.stdout


# ---- 5. the four plane counts are one layout ---------------------------------------------------------------
@pytest.mark.parametrize("w,h,s", K.LAYOUT_SHAPES)
def test_gpu_plane_counts_are_one_layout(bwrt_lib, w, h, s):
    """tests/test_assemble_adaptive.py's check on GPU contexts, and the GPU
    blocks against the CPU backend's."""
    gpu = K.one_layout(bwrt_lib, w, h, s, gpu=True)
    cpu = K.one_layout(bwrt_lib, w, h, s)
    assert gpu.keys() == cpu.keys() and len(gpu) == 6
    for (state, planes), g in gpu.items():
        c = cpu[(state, planes)]
        if planes in (4, 7):
            assert blocks_equal(g, c, planes), (state, planes)
        else:
            assert K.same_values(g, c), (state, planes)
