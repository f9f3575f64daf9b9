"""Row shards assembled into one frame (rt_export_shard, rt_assemble,
rt_assemble_multi) on the CPU backend — no GPU needed.
tests/test_gpu_assemble.py compares the GPU kernels with this backend.

The oracle of every test is one context that rendered the whole frame: the
shards' frameSum and moments, interleaved, are its bits, so every pass that
reads the assembled frame must give its bits too.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import assemble_case as A
from bwrt import Renderer, abi, assemble_multi, scenes

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd", "bin",
                   "bwrt_render")

# (width, height, shards): an odd width with uneven shards and padding (45 = 4 * 11 + 1), full 16-byte
# rows, fewer rows than a block is tall, three shards, one pixel, and more shards than rows
SHAPES = [(67, 45, 4), (64, 36, 8), (5, 3, 2), (16, 9, 3), (1, 1, 1), (8, 3, 8)]
FILTER_SHAPES = [(67, 45, 4), (16, 9, 3)]


@pytest.fixture(scope="module")
def scene07():
    return scenes.scene_07()


@pytest.fixture(scope="module")
def cases(bwrt_lib, scene07):
    """(w, h, S) -> (the full-frame context, the S shard contexts), made once."""
    made = {}

    def get(w, h, s, scene=None):
        key = (w, h, s, scene.name if scene else "07")
        if key not in made:
            sc = scene or scene07
            made[key] = (A.full_context(bwrt_lib, sc, w, h), A.shard_contexts(bwrt_lib, sc, w, h, s))
        return made[key]

    yield get
    for full, rs in made.values():
        full.close()
        for r in rs:
            r.close()


def state_of(r, rows, w):
    """The progressive state of a context: RNG, frameSum, frame counter, moments."""
    rng, acc = r.get_state(rows, w)
    var = r.variance(rows, w, want_lum=True) if r.moments_batches >= 2 else ()
    return A.bits((rng, acc) + tuple(var)), r.frame_counter, r.moments_batches


# ---- 1. the assembled frame is the full frame ---------------------------------------------------------
@pytest.mark.parametrize("w,h,s", SHAPES)
def test_assembled_frame_equals_full_frame(cases, w, h, s):
    full, rs = cases(w, h, s)
    _, acc = full.get_state(h, w)
    for planes in (3, 5):
        g, n, j = A.gather(rs, w, h, planes)
        assert n == full.frame_counter - 1 == sum(A.CALLS) and j == full.moments_batches == len(A.CALLS)
        before = state_of(rs[0], A.rows_of(h, s, 0), w)
        rs[0].assemble(g, n, j)
        assert state_of(rs[0], A.rows_of(h, s, 0), w) == before
        assert rs[0].assembled() == (n, j if planes == 5 else 0)
        if planes == 5:
            got, mom = rs[0].get_assembled(w, h, want_moments=True)
            # M is rt_get_variance's mean luminance; M2 is checked through the filter that reads it
            assert A.same(mom[..., 0], full.variance(h, w, want_lum=True)[1])
            kw = dict(want_color=True, want_var=True, min_batches=2)
            assert A.same(rs[0].denoise_var(w, h, **kw), full.denoise_var(w, h, **kw))
        else:
            got = rs[0].get_assembled(w, h)
        assert A.same(got, acc)


# ---- 2. the filters on the assembled frame ------------------------------------------------------------
@pytest.mark.parametrize("w,h,s", FILTER_SHAPES)
def test_filters_equal_full_frame(cases, w, h, s):
    full, rs = cases(w, h, s)
    want = A.filter_outputs(full, w, h)
    A.assemble_on(rs, w, h, 5)
    got = A.filter_outputs(rs[0], w, h)
    for name in want:
        assert A.same(got[name], want[name]), name
    assert not A.same(want["var_tracked"], want["var_spatial"])  # the two sources differ on this frame
    A.assemble_on(rs, w, h, 3)
    got = A.filter_outputs(rs[0], w, h, spatial_only=True)
    for name in got:
        assert A.same(got[name], want[name]), name


@pytest.mark.parametrize("w,h,s", FILTER_SHAPES)
def test_temporal_equals_full_frame(bwrt_lib, scene07, w, h, s):
    full = [A.full_context(bwrt_lib, scene07, w, h)]
    rs = A.shard_contexts(bwrt_lib, scene07, w, h, s)
    try:
        want = A.temporal_outputs(full, w, h)
        got = A.temporal_outputs(rs, w, h, assemble=lambda: A.assemble_on(rs, w, h, 3))
        assert len(want) == 4
        for k, (a, b) in enumerate(zip(got, want)):
            assert A.same(a, b), k
        assert want[2][2].max() > sum(A.CALLS)  # the second view did reproject history
    finally:
        for r in full + rs:
            r.close()


def test_filters_on_bvh_scene(bwrt_lib):
    """The stress scene's guides come from the BVH walk."""
    w, h, s = 96, 54, 2
    scene = scenes.stress_scene()
    full = A.full_context(bwrt_lib, scene, w, h)
    rs = A.shard_contexts(bwrt_lib, scene, w, h, s)
    try:
        A.assemble_on(rs, w, h, 5)
        assert A.same(rs[0].get_assembled(w, h), full.get_state(h, w)[1])
        kw = dict(want_color=True, want_var=True, min_batches=2)
        assert A.same(rs[0].denoise_var(w, h, **kw), full.denoise_var(w, h, **kw))
        assert A.same(rs[0].denoise(w, h, want_color=True), full.denoise(w, h, want_color=True))
    finally:
        for r in [full] + rs:
            r.close()


# ---- 3. padding -----------------------------------------------------------------------------------------
def test_padding_is_zero_filled_and_never_read(cases):
    w, h, s = 67, 45, 4
    full, rs = cases(w, h, s)
    rps = -(-h // s) + 1  # one row more than needed: every block has padding
    g, n, j = A.gather(rs, w, h, 5, rows_per_shard=rps)
    for i in range(s):
        rows = A.rows_of(h, s, i)
        assert not g[i, :, rows:].view(np.uint32).any(), i  # +0.0 bits
        assert g[i, :3, :rows].any()
        g[i, :, rows:].view(np.uint32)[...] = 0x7fc00123 + i  # NaN bit patterns
    rs[0].assemble(g, n, j)
    got, mom = rs[0].get_assembled(w, h, want_moments=True)
    assert A.same(got, full.get_state(h, w)[1]) and not np.isnan(mom).any()
    kw = dict(want_color=True, want_var=True, min_batches=2)
    assert A.same(rs[0].denoise_var(w, h, **kw), full.denoise_var(w, h, **kw))


# ---- 4. currency and the error contract -------------------------------------------------------------
def test_argument_errors_leave_the_assembled_frame(cases):
    w, h, s = 16, 9, 3
    full, rs = cases(w, h, s)
    lib, r = rs[0].lib, rs[0]
    g, n, j = A.assemble_on(rs, w, h, 5)
    kept = A.bits(r.get_assembled(w, h, want_moments=True))
    rps = g.shape[2]
    gp = g.ctypes.data
    blk = np.empty((5, rps, w), np.float32)
    bad = abi.RT_ERR_INVALID_ARGUMENT
    calls = [
        lambda: lib.rt_assemble(None, gp, s, rps, 5, n, j),
        lambda: lib.rt_assemble(r.ctx, None, s, rps, 5, n, j),
        lambda: lib.rt_assemble(r.ctx, gp, s, rps, 4, n, j),
        lambda: lib.rt_assemble(r.ctx, gp, 0, rps, 5, n, j),
        lambda: lib.rt_assemble(r.ctx, gp, s, rps - 1, 5, n, j),  # 3 * 2 < 9
        lambda: lib.rt_assemble(r.ctx, gp, s, rps, 5, 0, j),
        lambda: lib.rt_export_shard(r.ctx, rps, 5, None, None, None),
        lambda: lib.rt_export_shard(r.ctx, rps, 4, blk.ctypes.data, None, None),
        lambda: lib.rt_export_shard(r.ctx, A.rows_of(h, s, 0) - 1, 3, blk.ctypes.data, None, None),
    ]
    for k, call in enumerate(calls):
        assert call() == bad, k
        assert r.assembled() == (n, j), k
    assert lib.rt_export_shard_device(r.ctx, rps, 3, blk.ctypes.data, None, None, None) == abi.RT_ERR_UNSUPPORTED
    assert lib.rt_assemble_device(r.ctx, gp, s, rps, 5, n, j, None) == abi.RT_ERR_UNSUPPORTED  # CPU context
    assert A.bits(r.get_assembled(w, h, want_moments=True)) == kept
    # contexts without a scene / a frame shape / a frame
    with Renderer.cpu(1, lib=lib) as e:
        assert lib.rt_assemble(e.ctx, gp, s, rps, 5, n, j) == abi.RT_ERR_NO_SCENE
        e.set_scene(scenes.scene_07())
        assert lib.rt_assemble(e.ctx, gp, s, rps, 5, n, j) == bad and b"frame shape" in lib.rt_last_error(e.ctx)
        e.init_rand(w, h, 0, s)
        assert lib.rt_export_shard(e.ctx, rps, 3, blk.ctypes.data, None, None) == bad  # nothing accumulated
        assert lib.rt_assembled(e.ctx, None, None) == 0
        assert lib.rt_get_assembled(e.ctx, blk.ctypes.data, None) == bad
        assert e.last_assemble_ms() == -1.0
        assert lib.rt_assemble(e.ctx, gp, s, rps, 5, n, j) == abi.RT_OK  # a frame shape is enough
        assert e.assembled() == (n, j) and e.last_assemble_ms() >= 0.0
        assert A.same(e.get_assembled(w, h), full.get_state(h, w)[1])


def test_moments_and_nonuniform_refusals(bwrt_lib, scene07):
    w, h = 16, 9
    blk = np.empty((5, h, w), np.float32)
    lib = bwrt_lib
    with Renderer.cpu(0, lib=lib) as r:
        r.set_scene(scene07)
        A.accumulate(r, w, h)  # moments off
        assert lib.rt_export_shard(r.ctx, h, 5, blk.ctypes.data, None, None) == abi.RT_ERR_INVALID_ARGUMENT
        assert lib.rt_export_shard(r.ctx, h, 3, blk.ctypes.data, None, None) == abi.RT_OK
        r.set_moments(True)  # on in mid-accumulation: not live
        r.render(w, h, 1, A.BOUNCES)
        assert lib.rt_export_shard(r.ctx, h, 5, blk.ctypes.data, None, None) == abi.RT_ERR_INVALID_ARGUMENT
        A.accumulate(r, w, h)
        assert lib.rt_export_shard(r.ctx, h, 5, blk.ctypes.data, None, None) == abi.RT_OK
        r.reset_accumulation()  # the moments describe the last accumulation, not frame counter 1
        assert lib.rt_export_shard(r.ctx, h, 5, blk.ctypes.data, None, None) == abi.RT_ERR_INVALID_ARGUMENT
        A.accumulate(r, w, h)
        r.render_adaptive(w, h, A.BOUNCES, samples=1, min_frames=100)  # non-uniform
        for planes in (3, 5):
            assert lib.rt_export_shard(r.ctx, h, planes, blk.ctypes.data, None, None) == abi.RT_ERR_UNSUPPORTED
        arr = (C.c_void_p * 1)(r.ctx.value)
        assert lib.rt_assemble_multi(arr, 1, 3, 0) == abi.RT_ERR_UNSUPPORTED


def test_currency(bwrt_lib, scene07):
    w, h, s = 16, 9, 3
    lib = bwrt_lib
    full = A.full_context(lib, scene07, w, h)
    rs = A.shard_contexts(lib, scene07, w, h, s)
    r = rs[0]
    dn, dv, tp = r.denoise_params(), r.denoise_var_params(), r.temporal_params()
    passes = [lambda: lib.rt_denoise(r.ctx, C.byref(dn), None, None),
              lambda: lib.rt_denoise_var(r.ctx, C.byref(dv), None, None, None),
              lambda: lib.rt_temporal(r.ctx, C.byref(tp), None, None, None, None)]

    def refused(stale):
        for call in passes:
            assert call() == abi.RT_ERR_UNSUPPORTED
            err = lib.rt_last_error(r.ctx)
            assert b"row shard" in err and (b"stale" in err) == stale, err
        assert r.assembled() is None

    try:
        refused(stale=False)  # never assembled: as before
        want = A.filter_outputs(full, w, h)
        A.assemble_on(rs, w, h, 5)
        assert A.same(A.filter_outputs(r, w, h), want)
        # a snapshot: the shard's own accumulation may restart and move on
        before = state_of(r, 3, w)
        r.reset_accumulation()
        assert r.assembled() == (7, 3) and A.same(A.filter_outputs(r, w, h), want)
        twin = A.shard_contexts(lib, scene07, w, h, s)[0]
        for x in (r, twin):
            x.render(w, h, 2, A.BOUNCES, first_frame=8, row_offset=0, row_stride=s)  # continues the seven frames
            x.render(w, h, 1, A.BOUNCES, row_offset=0, row_stride=s)
        assert state_of(r, 3, w) == state_of(twin, 3, w) != before  # as a context that never assembled
        twin.close()
        assert r.assembled() == (7, 3) and A.same(A.filter_outputs(r, w, h), want)
        # drop
        r.assemble_drop()
        refused(stale=False)
        # each end of a view
        cam = r.get_camera()
        for end in (lambda: r.set_camera(cam), lambda: r.controls(["LEFT"], A.DT), lambda: r.set_scene(scene07),
                    lambda: r.render(w + 1, h, 1, A.BOUNCES, row_offset=0, row_stride=s)):
            g, n, j = A.gather(rs[1:] + rs[1:2], w, h, 3)  # (any blocks: this is about currency)
            r.init_rand(w, h, 0, s)
            r.assemble(g, n, j)
            assert r.assembled() == (n, 0)
            assert r.controls([], A.DT) == 0 and r.assembled() == (n, 0)  # no key: no movement
            end()
            refused(stale=True)
    finally:
        for x in [full] + rs:
            x.close()


def test_full_frame_context_ignores_its_assembled_frame(bwrt_lib, scene07):
    w, h = 16, 9
    with A.full_context(bwrt_lib, scene07, w, h) as r:
        want = A.filter_outputs(r, w, h)
        block, n, j = r.export_shard(h, w, 5)
        assert A.same(np.moveaxis(block[:3], 0, -1), r.get_state(h, w)[1])
        block[:] = 1.0  # nothing like its accumulation
        r.assemble(block[None], 1, 2)  # shards == 1
        assert r.assembled() == (1, 2) and (r.get_assembled(w, h) == 1.0).all()
        assert A.same(A.filter_outputs(r, w, h), want)


# ---- 5. rt_assemble_multi -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_assemble_multi(bwrt_lib, scene07, cases, n):
    w, h = 16, 9
    full, _ = cases(w, h, 3)
    _, acc = full.get_state(h, w)
    var = full.denoise_var(w, h, want_color=True, want_var=True, min_batches=2)
    rs = A.shard_contexts(bwrt_lib, scene07, w, h, n)
    try:
        for dst in sorted({0, n - 1}):
            for planes in (0, 3, 5):
                rs[dst].assemble_drop()
                assert assemble_multi(rs, planes, dst) == (7, 0 if planes == 3 else 3)
                assert A.same(rs[dst].get_assembled(w, h), acc)
                if planes != 3:
                    assert A.same(rs[dst].denoise_var(w, h, want_color=True, want_var=True, min_batches=2), var)
        # refusals touch nothing
        lib = bwrt_lib
        for r in rs:
            r.assemble_drop()

        def call(ctxs, planes=0, dst=0):
            arr = (C.c_void_p * len(ctxs))(*[r.ctx.value for r in ctxs])
            return lib.rt_assemble_multi(arr, len(ctxs), planes, dst)

        bad = abi.RT_ERR_INVALID_ARGUMENT
        assert call(rs + rs[:1]) == bad  # listed twice (and the wrong stride)
        assert call(rs, 4) == bad and call(rs, 0, n) == bad and call(rs, 0, -1) == bad
        if n > 1:
            assert call(rs[::-1]) == bad  # wrong shard offsets
            assert call(rs[:1] + rs[:1]) == bad
            rs[-1].render(w, h, 1, A.BOUNCES, row_offset=n - 1, row_stride=n)
            assert call(rs) == bad and b"frame counters" in lib.rt_last_error(rs[0].ctx)
        assert all(r.assembled() is None for r in rs)
    finally:
        for r in rs:
            r.close()


def test_assemble_multi_mixed_moments(bwrt_lib, scene07):
    """planes 0 falls back to 3 when one context's moments are not current; 5 is then refused."""
    w, h, n = 16, 9, 2
    rs = A.shard_contexts(bwrt_lib, scene07, w, h, n)
    try:
        rs[1].set_moments(False)
        assert assemble_multi(rs, 0, 0) == (7, 0)
        arr = (C.c_void_p * n)(*[r.ctx.value for r in rs])
        assert bwrt_lib.rt_assemble_multi(arr, n, 5, 0) == abi.RT_ERR_INVALID_ARGUMENT
    finally:
        for r in rs:
            r.close()


# ---- 6. thread counts -----------------------------------------------------------------------------------
def test_thread_count_invariance(bwrt_lib, scene07):
    w, h, s = 67, 45, 4
    got = []
    for threads in (1, 5):
        rs = A.shard_contexts(bwrt_lib, scene07, w, h, s, threads=threads)
        g, n, j = A.assemble_on(rs, w, h, 5)
        got.append(A.bits((g,) + rs[0].get_assembled(w, h, want_moments=True)))
        for r in rs:
            r.close()
    assert got[0] == got[1]


# ---- 7. the CLI -----------------------------------------------------------------------------------------
def test_cli_names_the_combination_and_keeps_its_refusals():
    usage = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert usage.returncode == 0 and "rt_assemble_multi" in usage.stdout
    for bad in (["--moments"], ["--adaptive", "0.1"]):
        r = subprocess.run([CLI, "--width", "16", "--height", "9", "--frames", "2", "--gpus", "2"] + bad,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--gpus" in r.stderr, (bad, r.stderr)
