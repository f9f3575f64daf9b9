"""Adaptive sampling on row shards (rt_adaptive_export_rows,
rt_render_adaptive_shard, rt_render_adaptive_multi) on the
CPU backend — no GPU needed.  tests/test_gpu_adaptive_multi.py runs the kernels
against this backend.

The oracle: S shard contexts that exchange their row sums end with,
interleaved, exactly the bits of one context that ran rt_render_adaptive on the
whole frame (tests/adaptive_multi_case.py builds both).
"""
import ctypes as C

import numpy as np
import pytest

import adaptive_multi_case as M
from bwrt import Renderer, abi, render_adaptive_multi, scenes

# (scene, width, height): two mask words per row and a width that is no
# multiple of 64; a width of exactly one word; the BVH scene, where a shard's
# list may be empty or shorter than a wave
MAIN = [("07", 67, 45), ("04_box", 64, 36), ("stress", 96, 54)]
SHARDS = (1, 2, 3, 8)
# radii 0..4 on 07: radius >= stride (4 over 2 and 3 shards), radius < stride (1
# and 2 under 8), and windows clipped at the top and bottom rows across shard
# boundaries; the other scenes take the default and the largest
RADII = {"07": (0, 1, 2, 3, 4), "04_box": (2, 4), "stress": (2, 4)}
CASES = [(n, w, h, s, r) for n, w, h in MAIN for r in RADII[n] for s in SHARDS]


# ---- ABI ------------------------------------------------------------------------------------------------
def test_abi_declares_the_entry_points(bwrt_lib):
    names = {"rt_adaptive_export_rows", "rt_adaptive_export_rows_device", "rt_render_adaptive_shard",
             "rt_render_adaptive_shard_device", "rt_render_adaptive_multi"}
    assert names <= set(abi.declared_functions())
    for n in names:
        assert hasattr(bwrt_lib, n)


# ---- guards: the equality tests below cannot pass vacuously ------------------------------------------------
@pytest.mark.parametrize("name,w,h", MAIN)
def test_guard_first_call_selects_a_proper_subset(bwrt_lib, name, w, h):
    for radius in RADII[name]:
        first = M.oracle(bwrt_lib, name, w, h, M.sequence(radius))["calls"][0]
        print(f"{name} {w}x{h} radius {radius}: first call selects {first['selected']} of {w * h}")
        assert 0 < first["selected"] < w * h, (radius, first["selected"])


def test_guard_the_vertical_window_decides_pixels(bwrt_lib):
    """Radius 2 against radius 0 on 07 at 67x45: the selected sets differ, so
    the column taps — the part that crosses shards — decide pixels."""
    w, h = 67, 45
    took = []
    for radius in (0, 2):
        o = M.oracle(bwrt_lib, "07", w, h, M.sequence(radius, ks=(3,)))
        took.append(o["final"]["n"] > sum(M.CALLS))
    differ = np.count_nonzero(took[0] != took[1])
    print(f"radius 2 against radius 0: {differ} of {w * h} pixels differ")
    assert differ > 0


# ---- the core: shards against the full frame ----------------------------------------------------------------
@pytest.mark.parametrize("name,w,h,shards,radius", CASES)
def test_shards_equal_the_full_frame(bwrt_lib, name, w, h, shards, radius):
    """Three successive calls, so the other ranks' non-uniform counts feed the
    next selection.  shards == 1 is a full-frame context on the two-phase entry
    points against rt_render_adaptive."""
    seq = M.sequence(radius)
    M.assert_same(M.run_shards(bwrt_lib, name, w, h, shards, seq), M.oracle(bwrt_lib, name, w, h, seq))


@pytest.mark.parametrize("w,h,shards", [(5, 3, 8), (5, 3, 2), (1, 1, 1), (1, 1, 3)])
def test_tiny_frames_and_ranks_beyond_the_height(bwrt_lib, w, h, shards):
    # (min_frames forces the pixels of these frames, whose moments select nothing by themselves, on the first call)
    seq = M.sequence(2, min_frames=9) if (w, h) == (5, 3) else M.sequence(1, min_frames=8)
    want = M.oracle(bwrt_lib, "07", w, h, seq)
    assert want["calls"][0]["selected"] == w * h
    M.assert_same(M.run_shards(bwrt_lib, "07", w, h, shards, seq), want)


@pytest.mark.parametrize("over,bounces,spp", [
    (dict(min_frames=9, max_frames=12), M.BOUNCES, 1),   # forced below 9, capped at 12: both clauses, cap first
    (dict(min_frames=100, max_frames=11), M.BOUNCES, 1),  # everything forced, the cap wins on the later calls
    (dict(), M.BOUNCES, 2),                               # samplesPerPixel 2
    (dict(), 0, 1),                                       # max_bounces 0
])
def test_parameters(bwrt_lib, over, bounces, spp):
    w, h = 67, 45
    seq = M.sequence(2, **over)
    want = M.oracle(bwrt_lib, "07", w, h, seq, bounces=bounces, spp=spp)
    if over:
        assert [c["selected"] for c in want["calls"]] != [want["calls"][0]["selected"]] * 3  # the clauses bite
    M.assert_same(M.run_shards(bwrt_lib, "07", w, h, 3, seq, bounces=bounces, spp=spp), want)


def multi_call(rs, w, h, p, bounces):
    rgba, st = render_adaptive_multi(rs, w, h, bounces, **p)
    return {"rgba": rgba, "selected": st["selected"], "frames_total": st["frames_total"]}


@pytest.mark.parametrize("w,h,shards", [(67, 45, 3), (67, 45, 1), (5, 3, 8)])
def test_multi_equals_the_two_phase_calls(bwrt_lib, w, h, shards):
    seq = M.sequence(2, min_frames=9 if h == 3 else 0)
    want = M.oracle(bwrt_lib, "07", w, h, seq)
    got = M.run_shards(bwrt_lib, "07", w, h, shards, seq, call=multi_call)
    for a, b in zip(got["calls"], want["calls"]):
        assert a["selected"] == b["selected"] and a["frames_total"] == b["frames_total"]
        assert M.same(a["rgba"], b["rgba"])
    for k in want["final"]:
        assert M.same(got["final"][k], want["final"][k]), k


def test_multi_refusals_touch_nothing(bwrt_lib):
    lib, w, h = bwrt_lib, 33, 17
    rs = M.contexts(lib, scenes.scene_07(), w, h, 3)
    d = rs[0].adaptive_params(samples=2, **M.DEFAULTS)

    def call(ctxs, params=d):
        arr = (C.c_void_p * len(ctxs))(*[r.ctx.value for r in ctxs])
        return lib.rt_render_adaptive_multi(arr, len(ctxs), C.byref(params) if params is not None else None, M.BOUNCES,
                                            None, None)
    before = M.bits(M.snapshot(rs, w, h))
    assert call(rs, rs[0].adaptive_params(samples=0)) == abi.RT_ERR_INVALID_ARGUMENT
    assert call([rs[0], rs[1], rs[1]]) == abi.RT_ERR_INVALID_ARGUMENT  # listed twice
    assert call([rs[1], rs[0], rs[2]]) == abi.RT_ERR_INVALID_ARGUMENT  # not shards i (mod n)
    assert call(rs[:2]) == abi.RT_ERR_INVALID_ARGUMENT                  # stride 3, two contexts
    assert call(rs, None) == abi.RT_ERR_INVALID_ARGUMENT
    with Renderer.cpu(1, lib=lib) as other:  # a context of another frame
        other.set_scene(scenes.scene_07())
        assert call([rs[0], rs[1], other]) == abi.RT_ERR_INVALID_ARGUMENT
    assert before == M.bits(M.snapshot(rs, w, h))  # nothing was touched
    rs[2].render(w, h, 1, M.BOUNCES, row_offset=2, row_stride=3)        # one more batch on one context
    assert call(rs) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"differ" in lib.rt_last_error(rs[0].ctx)
    for r in rs[:2]:
        r.render(w, h, 1, M.BOUNCES, row_offset=r is rs[1] and 1 or 0, row_stride=3)
    assert not any((r.counts(M.rows_of(h, 3, i), w)[0] != 8).any() for i, r in enumerate(rs))  # all still uniform
    assert call(rs) == abi.RT_OK
    M.close(rs)


# ---- phase 1 alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [1, 3])
def test_export_alone_leaves_the_state_untouched(bwrt_lib, shards):
    """After an export without a phase 2, a continuing uniform render,
    rt_export_shard and rt_get_counts give what a context that never exported gives."""
    lib, w, h = bwrt_lib, 67, 45
    rps = -(-h // shards) + 2  # (more padding rows than the gather needs)
    got = []
    for export in (False, True):
        rs = M.contexts(lib, scenes.scene_07(), w, h, shards)
        out = []
        for i, r in enumerate(rs):
            rows = M.rows_of(h, shards, i)
            if export:
                blk = r.adaptive_export_rows(rps, w, samples=3, **M.DEFAULTS)
                assert (blk[:, rows:].view(np.uint32) == 0).all()  # the padding rows
                assert blk[2, :rows].view(np.int32).min() >= 1 and blk[2, :rows].view(np.int32).max() <= 5
            out.append(r.counts(rows, w))
            out.append(r.export_shard(rps, w, 5))
            img, acc = r.render(w, h, 2, M.BOUNCES, row_offset=i, row_stride=shards, want_accum=True)
            out += [img, acc, r.counts(rows, w), r.variance(rows, w, want_lum=True),
                    np.array([r.frame_counter, r.moments_batches])]
        got.append(M.bits(out))
        M.close(rs)
    assert got[0] == got[1]


# ---- errors -----------------------------------------------------------------------------------------------------
def test_errors(bwrt_lib):
    lib, w, h, s = bwrt_lib, 33, 17, 3
    scene = scenes.scene_07()
    rps = -(-h // s)
    with Renderer.cpu(2, lib=lib) as r:
        block = np.zeros((3, rps, w), np.float32)
        gathered = np.zeros((s, 3, rps, w), np.float32)

        def export(ptr=block.ctypes.data, rows=rps, null_params=False, **kw):
            d = r.adaptive_params(**kw)
            return lib.rt_adaptive_export_rows(r.ctx, None if null_params else C.byref(d), rows, ptr)

        def shard(ptr=gathered.ctypes.data, shards=s, rows=rps, null_params=False, bounces=2, **kw):
            d = r.adaptive_params(**kw)
            return lib.rt_render_adaptive_shard(r.ctx, None if null_params else C.byref(d), bounces, ptr, shards, rows,
                                                None, None, None)

        def render(k=2, first=0):
            r.render(w, h, k, 2, first_frame=first, row_offset=1, row_stride=s)

        assert export() == abi.RT_ERR_NO_SCENE
        r.set_scene(scene)
        assert export() == abi.RT_ERR_INVALID_ARGUMENT  # no state
        render(first=1)
        render()
        assert export() == abi.RT_ERR_INVALID_ARGUMENT  # tracking off
        r.set_moments(True)
        render(first=1)
        assert export() == abi.RT_ERR_INVALID_ARGUMENT  # one batch
        assert b"2 batches" in lib.rt_last_error(r.ctx)
        render()
        # phase 1: rt_render_adaptive's checks minus the shard refusal
        for bad in (dict(samples=0), dict(tolerance=0.0), dict(tolerance=float("nan")), dict(lum_floor=-0.5),
                    dict(radius=-1), dict(radius=abi.RT_ADAPTIVE_MAX_RADIUS + 1)):
            assert export(**bad) == abi.RT_ERR_INVALID_ARGUMENT, bad
        assert export(ptr=None) == abi.RT_ERR_INVALID_ARGUMENT
        assert export(null_params=True) == abi.RT_ERR_INVALID_ARGUMENT
        assert export(rows=M.rows_of(h, s, 1) - 1) == abi.RT_ERR_INVALID_ARGUMENT
        d = r.adaptive_params()
        assert lib.rt_adaptive_export_rows_device(r.ctx, C.byref(d), rps, block.ctypes.data, None) == abi.RT_ERR_UNSUPPORTED
        assert lib.rt_render_adaptive_shard_device(r.ctx, C.byref(d), 2, gathered.ctypes.data, s, rps, None,
                                                   None) == abi.RT_ERR_UNSUPPORTED
        # the full-frame entry point keeps refusing a shard, with its message
        assert lib.rt_render_adaptive(r.ctx, C.byref(d), 2, None, None, None) == abi.RT_ERR_UNSUPPORTED
        assert b"row shard" in lib.rt_last_error(r.ctx)
        # phase 2 without a current phase 1
        assert shard() == abi.RT_ERR_INVALID_ARGUMENT  # none was made
        assert b"rt_adaptive_export_rows" in lib.rt_last_error(r.ctx)
        assert export(radius=1) == abi.RT_OK
        assert shard(radius=2) == abi.RT_ERR_INVALID_ARGUMENT  # made with another radius
        assert export(radius=2) == abi.RT_OK
        # with a current one: the arguments
        assert shard(ptr=None) == abi.RT_ERR_INVALID_ARGUMENT
        assert shard(null_params=True) == abi.RT_ERR_INVALID_ARGUMENT
        assert shard(shards=s + 1) == abi.RT_ERR_INVALID_ARGUMENT
        assert shard(shards=1, rows=h) == abi.RT_ERR_INVALID_ARGUMENT
        assert shard(rows=rps - 1) == abi.RT_ERR_INVALID_ARGUMENT  # rows_per_shard * shards < height
        assert shard(bounces=abi.RT_MAX_BOUNCES + 1) == abi.RT_ERR_UNSUPPORTED
        assert (r.counts(M.rows_of(h, s, 1), w)[0] == 4).all()  # no refusal changed anything: still uniform
        # what ends a phase 1: a render, a reset, a camera call, a scene call, an adaptive call
        enders = {"render": render, "reset": r.reset_accumulation, "camera": lambda: r.set_camera(scene.camera),
                  "controls": lambda: r.controls(["LEFT"], 0.05), "scene": lambda: r.set_scene(scene)}
        for name, end in enders.items():
            assert export() == abi.RT_OK
            end()
            assert shard() == abi.RT_ERR_INVALID_ARGUMENT, name
            if name != "render":
                assert export() == abi.RT_ERR_INVALID_ARGUMENT and b"render first" in lib.rt_last_error(r.ctx)
                render(first=1)
                render()
        assert export() == abi.RT_OK and shard() == abi.RT_OK
        assert shard() == abi.RT_ERR_INVALID_ARGUMENT  # the call consumed it: the counts moved
        assert export() == abi.RT_OK and shard() == abi.RT_OK


# ---- the non-uniform state on a shard context and its ends ---------------------------------------------------------
def test_non_uniform_state_on_a_shard(bwrt_lib):
    lib, w, h, s, mb = bwrt_lib, 33, 17, 2, 2
    scene = scenes.scene_07()
    rows, rps = M.rows_of(h, s, 1), -(-h // s)
    with Renderer.cpu(2, lib=lib) as r:
        def go_non_uniform():
            r.set_scene(scene)
            r.init_rand(w, h, 1, s)
            r.set_moments(True)
            for i in range(4):
                r.render(w, h, 2, mb, first_frame=1 if i == 0 else 0, row_offset=1, row_stride=s)
            g = np.zeros((s, 3, rps, w), np.float32)
            g[1] = r.adaptive_export_rows(rps, w, samples=2, min_frames=100)
            _, st = r.render_adaptive_shard(g, rows, w, mb, samples=2, min_frames=100)
            assert st["selected"] == rows * w and st["frames_total"] == rows * w * 10
        params = r.params(w, h, 1, mb, row_offset=1, row_stride=s)
        go_non_uniform()
        assert r.frame_counter == 9 and r.moments_batches == 4  # the uniform base, not advanced
        for first in (0, 9, 2):
            params.first_frame = first
            assert lib.rt_render_ex(r.ctx, C.byref(params), None, None) == abi.RT_ERR_UNSUPPORTED, first
            assert b"non-uniform" in lib.rt_last_error(r.ctx)
        blk = np.zeros((5, rps, w), np.float32)
        assert lib.rt_export_shard(r.ctx, rps, 3, blk.ctypes.data, None, None) == abi.RT_ERR_UNSUPPORTED
        arr = (C.c_void_p * 1)(r.ctx.value)
        assert lib.rt_render_multi(arr, 1, w, h, 1, None) == abi.RT_ERR_UNSUPPORTED
        # what keeps working
        r.get_state(rows, w)
        assert np.isfinite(r.variance(rows, w)).all()
        n, j = r.counts(rows, w)
        assert (n == 10).all() and (j == 5).all()
        # the ends: a render of frame 1, rt_set_scene, rt_init_rand, rt_set_state, rt_set_moments(0), a reset
        r.render(w, h, 2, mb, first_frame=1, row_offset=1, row_stride=s)
        assert (r.counts(rows, w)[0] == 2).all()
        assert lib.rt_export_shard(r.ctx, rps, 3, blk.ctypes.data, None, None) == abi.RT_OK
        go_non_uniform()
        r.set_scene(scene)
        assert r.frame_counter == 1 and (r.counts(rows, w)[0] == 0).all()
        go_non_uniform()
        r.init_rand(w, h, 1, s)
        assert (r.counts(rows, w)[0] == 0).all()
        go_non_uniform()
        rng, acc = r.get_state(rows, w)
        r.set_state(rng, acc, 9)
        assert (r.counts(rows, w)[0] == 8).all()
        go_non_uniform()
        r.set_moments(False)
        assert (r.counts(rows, w)[0] == 8).all()
        go_non_uniform()
        r.reset_accumulation()
        r.render(w, h, 1, mb, row_offset=1, row_stride=s)
        assert (r.counts(rows, w)[0] == 1).all()


# ---- thread-count invariance ---------------------------------------------------------------------------------------
def test_thread_count_invariance(bwrt_lib):
    w, h, seq = 67, 45, M.sequence(2)
    got = [M.run_shards(bwrt_lib, "07", w, h, 3, seq, threads=t) for t in (1, 5)]
    M.assert_same(got[0], got[1])
    M.assert_same(got[0], M.oracle(bwrt_lib, "07", w, h, seq))
