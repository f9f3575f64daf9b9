"""Row shards assembled into one frame on the MI355X: the HIP kernels behind
rt_export_shard and rt_assemble against the CPU backend, bit for bit (both are
copies with the indexing of csrc/rt_assemble.h), the device-stream entry
points, rt_assemble_multi behind rt_render_multi, bwrt.dist.gather_frame over
nccl and the CLI.  The GPU contexts render their shards; the CPU contexts
render the same frames from the same seeds (tests/test_assemble.py checks those
against one full-frame context).
"""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import assemble_case as A
from bwrt import Renderer, abi, assemble_multi, render_multi, scenes

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "bwidman-raytracer_amd", "bin", "bwrt_render")

# (width, height, shards): test_assemble.py's shapes, then many workgroups on the 4-byte path (odd width) and
# rows of exactly full 16-byte groups
SHAPES = [(67, 45, 4), (64, 36, 8), (16, 9, 3), (5, 3, 2), (1, 1, 1), (333, 187, 8), (256, 64, 2)]
TEMPORAL_SHAPES = [(67, 45, 4), (16, 9, 3)]


@pytest.fixture(scope="module")
def scene07():
    return scenes.scene_07()


def close(*groups):
    for rs in groups:
        for r in rs:
            r.close()


def pad_with_nans(g, h):
    """One more row per block than needed, every padding row NaN bit patterns."""
    s, planes, rps, w = g.shape
    out = np.empty((s, planes, rps + 1, w), np.float32)
    out.view(np.uint32)[...] = 0x7fc00321
    for i in range(s):
        rows = A.rows_of(h, s, i)
        out[i, :, :rows] = g[i, :, :rows]
    return out


# ---- 1. the kernels against the CPU backend -----------------------------------------------------------
@pytest.mark.parametrize("w,h,s", SHAPES)
def test_gpu_equals_cpu(bwrt_lib, scene07, w, h, s):
    gs = A.shard_contexts(bwrt_lib, scene07, w, h, s, gpu=True)
    cs = A.shard_contexts(bwrt_lib, scene07, w, h, s)
    try:
        for planes in (3, 5):
            gg, n, j = A.gather(gs, w, h, planes)
            cg, cn, cj = A.gather(cs, w, h, planes)
            assert (n, j) == (cn, cj) == (7, 3)
            assert A.same_values(gg, cg), planes  # the exported blocks, zero padding included
            # larger blocks: the padding is zero-filled there too, and never read
            big, _, _ = A.gather(gs, w, h, planes, rows_per_shard=gg.shape[2] + 1)
            assert A.same_values(big, A.gather(cs, w, h, planes, rows_per_shard=gg.shape[2] + 1)[0])
            for i in range(s):
                assert not big[i, :, A.rows_of(h, s, i):].view(np.uint32).any()  # +0.0 bits
            frames = []
            for r, g in ((gs[0], pad_with_nans(gg, h)), (gs[0], gg), (cs[0], cg)):
                r.assemble(g, n, j)
                assert r.assembled() == (n, j if planes == 5 else 0)
                got = r.get_assembled(w, h, want_moments=planes == 5)
                frames.append(got if planes == 5 else (got,))
            # within the GPU backend bit for bit, NaN payloads included: the padded and the plain
            # blocks, and the shards' own frameSum interleaved
            assert A.same(frames[0], frames[1]) and A.same(frames[1][0], A.interleave(gs, w, h)), planes
            assert A.same_values(frames[1], frames[2]), planes
            assert gs[0].last_assemble_ms() > 0
            got = A.filter_outputs(gs[0], w, h, spatial_only=planes == 3)
            want = A.filter_outputs(cs[0], w, h, spatial_only=planes == 3)
            for name in want:
                assert A.same_values(got[name], want[name]), (planes, name)
    finally:
        close(gs, cs)


@pytest.mark.parametrize("w,h,s", TEMPORAL_SHAPES)
def test_gpu_temporal_equals_cpu(bwrt_lib, scene07, w, h, s):
    gs = A.shard_contexts(bwrt_lib, scene07, w, h, s, gpu=True)
    cs = A.shard_contexts(bwrt_lib, scene07, w, h, s)
    try:
        got = A.temporal_outputs(gs, w, h, assemble=lambda: A.assemble_on(gs, w, h, 3))
        want = A.temporal_outputs(cs, w, h, assemble=lambda: A.assemble_on(cs, w, h, 3))
        for k, (a, b) in enumerate(zip(got, want)):
            assert A.same_values(a, b), k
    finally:
        close(gs, cs)


def test_gpu_bvh_scene_equals_cpu(bwrt_lib):
    w, h, s = 96, 54, 2
    scene = scenes.stress_scene()
    gs = A.shard_contexts(bwrt_lib, scene, w, h, s, gpu=True)
    cs = A.shard_contexts(bwrt_lib, scene, w, h, s)
    try:
        kw = dict(want_color=True, want_var=True, min_batches=2)
        outs = []
        for rs in (gs, cs):
            A.assemble_on(rs, w, h, 5)
            outs.append((rs[0].get_assembled(w, h, want_moments=True), rs[0].denoise_var(w, h, **kw)))
        assert A.same_values(*outs)
    finally:
        close(gs, cs)


def test_unaligned_pointer_takes_the_4_byte_path(bwrt_lib, scene07):
    """width % 4 == 0, but `gathered_device` (and a block) 4 bytes off a 16-byte boundary."""
    import torch
    w, h, s = 64, 36, 8
    gs = A.shard_contexts(bwrt_lib, scene07, w, h, s, gpu=True)
    try:
        g, n, j = A.assemble_on(gs, w, h, 5)
        want = A.bits(gs[0].get_assembled(w, h, want_moments=True))
        for off in (0, 1):
            gs[0].assemble_drop()
            buf = torch.zeros(g.size + 4, dtype=torch.float32, device="cuda")
            buf[off:off + g.size] = torch.from_numpy(g.reshape(-1)).cuda()
            assert buf.data_ptr() % 16 == 0
            blk = torch.zeros(g[0].size + 4, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            gs[0].assemble_device(buf.data_ptr() + 4 * off, s, g.shape[2], 5, n, j)
            assert A.bits(gs[0].get_assembled(w, h, want_moments=True)) == want, off
            gs[1].export_shard_device(blk.data_ptr() + 4 * off, g.shape[2], 5)
            gs[1].synchronize()
            assert A.same(blk.cpu().numpy()[off:off + g[0].size].reshape(g[0].shape), g[1]), off
            assert not blk.cpu().numpy()[off + g[0].size:].any()  # nothing past the block
        bad = abi.RT_ERR_INVALID_ARGUMENT
        assert bwrt_lib.rt_assemble_device(gs[0].ctx, buf.data_ptr() + 2, s, g.shape[2], 5, n, j, None) == bad
        assert bwrt_lib.rt_export_shard_device(gs[1].ctx, g.shape[2], 5, blk.data_ptr() + 2, None, None, None) == bad
    finally:
        close(gs)


def test_capped_grid_gives_the_same_bits(monkeypatch, bwrt_lib, scene07):
    """BWRT_DEINT_BLOCKS=1: one workgroup strides over every item (read at rt_create, BWRT_TUNING=1)."""
    w, h, s = 67, 45, 4
    cs = A.shard_contexts(bwrt_lib, scene07, w, h, s)
    monkeypatch.setenv("BWRT_DEINT_BLOCKS", "1")
    gs = A.shard_contexts(bwrt_lib, scene07, w, h, s, gpu=True)
    try:
        outs = []
        for rs in (gs, cs):
            g, n, j = A.assemble_on(rs, w, h, 5)
            outs.append((g, rs[0].get_assembled(w, h, want_moments=True)))
        assert A.same_values(*outs)
    finally:
        close(gs, cs)


# ---- 2. the _device forms -------------------------------------------------------------------------------
@pytest.mark.parametrize("own_stream", [True, False])
def test_device_chain_without_host_sync(bwrt_lib, scene07, own_stream):
    """Render, export, concatenate, assemble, denoise and a continuing render queued back to back on one
    stream (context 0's own, or a caller's torch stream), five times over."""
    import torch
    w, h, s = 64, 36, 4
    rps = -(-h // s)
    cs = A.shard_contexts(bwrt_lib, scene07, w, h, s)
    gs = [A.new(bwrt_lib, gpu=True) for _ in range(s)]
    try:
        A.assemble_on(cs, w, h, 5)
        want_dn = cs[0].denoise(w, h)
        want_dv = cs[0].denoise_var(w, h, min_batches=2)
        for i, c in enumerate(cs):  # the continuation
            c.render(w, h, 1, A.BOUNCES, row_offset=i, row_stride=s)
        want_state = [c.get_state(A.rows_of(h, s, i), w) for i, c in enumerate(cs)]
        for g in gs:
            g.set_scene(scene07)
            g.set_moments(True)
        if own_stream:
            tstream = torch.cuda.ExternalStream(gs[0].stream_handle())
        else:
            tstream = torch.cuda.Stream()
        sp = tstream.cuda_stream
        raws = [torch.zeros(rps * w, dtype=torch.int32, device="cuda") for _ in range(s)]
        blocks = [torch.zeros((5, rps, w), dtype=torch.float32, device="cuda") for _ in range(s)]
        out_dn, out_dv = (torch.zeros(h * w, dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()  # (the zero fills ran on torch's default stream, unordered with `tstream`)
        runs = []
        for _ in range(5):
            for i, g in enumerate(gs):
                g.init_rand(w, h, i, s)  # the seeds of frame 1: every sequence renders the same frames
            for i, g in enumerate(gs):
                for k, frames in enumerate(A.CALLS):
                    g.render_device(g.params(w, h, frames, A.BOUNCES, 1 if k == 0 else 0, i, s), raws[i].data_ptr(), sp)
                n, j = g.export_shard_device(blocks[i].data_ptr(), rps, 5, sp)
                assert (n, j) == (7, 3)
            with torch.cuda.stream(tstream):
                gathered = torch.cat(blocks)
            gs[0].assemble_device(gathered.data_ptr(), s, rps, 5, n, j, sp)
            gs[0].denoise_device(out_dn.data_ptr(), sp)
            gs[0].denoise_var_device(out_dv.data_ptr(), sp, min_batches=2)
            for i, g in enumerate(gs):
                g.render_device(g.params(w, h, 1, A.BOUNCES, 0, i, s), raws[i].data_ptr(), sp)
            tstream.synchronize()
            dn = out_dn.cpu().numpy().view(np.uint8).reshape(h, w, 4)
            dv = out_dv.cpu().numpy().view(np.uint8).reshape(h, w, 4)
            state = [g.get_state(A.rows_of(h, s, i), w) for i, g in enumerate(gs)]
            assert np.array_equal(dn, want_dn) and np.array_equal(dv, want_dv)
            assert A.same_values(state, want_state)  # the continuation equals an uninterrupted render
            runs.append(A.bits((dn, dv, state, gs[0].get_assembled(w, h, want_moments=True))))
            assert gs[0].last_assemble_ms() > 0
        assert all(r == runs[0] for r in runs[1:])
    finally:
        close(gs, cs)


# ---- 3. rt_assemble_multi behind rt_render_multi ----------------------------------------------------
@pytest.fixture(scope="module")
def full_gpu(bwrt_lib, scene07):
    """(w, h) -> every pass on one GPU context that rendered the whole frame, over two views."""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            with A.full_context(bwrt_lib, scene07, w, h, gpu=True) as r:
                views = []
                for view in range(2):
                    if view:
                        r.controls(["LEFT"], A.DT)
                        A.accumulate(r, w, h, restart=False)
                    views.append((A.filter_outputs(r, w, h),
                                  r.temporal(w, h, denoise={"iterations": 2}, want_color=True, want_length=True)))
                made[w, h] = views
        return made[w, h]

    return get


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("w,h", [(64, 36), (67, 45)])
def test_assemble_multi_after_render_multi(bwrt_lib, scene07, full_gpu, w, h, n):
    want = full_gpu(w, h)
    dst = n - 1 if n == 3 else 0
    rs = [A.new(bwrt_lib, gpu=True) for _ in range(n)]
    try:
        for r in rs:
            r.set_scene(scene07)
            r.set_moments(True)
            r.set_max_bounces(A.BOUNCES)  # (rt_render_multi renders at the context's limit)
        for view in range(2):
            if view:
                for r in rs:
                    r.controls(["LEFT"], A.DT)
                assert rs[dst].assembled() is None
            for k in A.CALLS:
                render_multi(rs, w, h, k)
            assert assemble_multi(rs, 0, dst) == (7, 3)
            assert rs[dst].last_assemble_ms() > 0
            assert A.same(A.filter_outputs(rs[dst], w, h), want[view][0]), view
            got = rs[dst].temporal(w, h, denoise={"iterations": 2}, want_color=True, want_length=True)
            assert A.same(got, want[view][1]), view
    finally:
        close(rs)


def test_assemble_multi_refuses_mixed_kinds(bwrt_lib, scene07):
    w, h = 16, 9
    gs = A.shard_contexts(bwrt_lib, scene07, w, h, 2, gpu=True)
    cs = A.shard_contexts(bwrt_lib, scene07, w, h, 2)
    try:
        arr = (C.c_void_p * 2)(gs[0].ctx.value, cs[1].ctx.value)
        assert bwrt_lib.rt_assemble_multi(arr, 2, 3, 0) == abi.RT_ERR_INVALID_ARGUMENT
        assert b"mixed" in bwrt_lib.rt_last_error(gs[0].ctx)
        assert gs[0].assembled() is None and cs[1].assembled() is None
    finally:
        close(gs, cs)


# ---- 4. gather_frame over nccl --------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_gather_frame_over_nccl_one_rank():
    """World size 1 under torch.distributed.run, one fresh child process (tests/assemble_nccl_child.py)."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
                        "--master-addr=127.0.0.1", f"--master-port={_free_port()}",
                        os.path.join(REPO, "tests", "assemble_nccl_child.py")],
                       env=env, cwd=REPO, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "assembled frame equals the accumulation" in r.stdout


# ---- 5. the CLI -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [["--denoise"], ["--denoise-var", "--frames-per-call", "1"],
                                  ["--temporal", "--keys", "LEFT*2", "--dt", "0.01"]],
                         ids=["denoise", "denoise-var", "temporal"])
def test_cli_two_contexts_write_the_same_png(tmp_path, opts):
    files = []
    for gpus in (1, 2):
        png = tmp_path / f"out{gpus}.png"
        r = subprocess.run([CLI, "--scene", "07", "--width", "64", "--height", "36", "--frames", "4", "--gpus",
                            str(gpus), "--out", str(png)] + opts, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert ("assemble: 2 shards" in r.stdout) == (gpus == 2), r.stdout
        if opts[0] == "--denoise-var":
            assert "tracked variance of 4 batches" in r.stdout, r.stdout
        files.append(png.read_bytes())
    assert files[0] == files[1]
