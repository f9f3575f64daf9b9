"""Counted assembled frames (rt_export_shard_adaptive, rt_assemble_adaptive,
rt_assemble_adaptive_multi, rt_get_assembled_counts) on
the CPU backend — no GPU needed.  tests/test_gpu_assemble_adaptive.py compares
the GPU kernels with this backend.

The oracle of every test is one full-frame context that ran the same
rt_render_adaptive calls with rt_set_adaptive_filters on: the shard contexts'
frameSum, moments and counts, interleaved, are its bits, so every pass that
reads the counted assembled frame must give its bits too.
"""
import ctypes as C

import numpy as np
import pytest

import adaptive_multi_case as M
import assemble_adaptive_case as K
import assemble_case as A
from bwrt import Renderer, abi, assemble_adaptive_multi, render_adaptive_multi, scenes

# (scene, width, height, shards, adaptive calls): 07 at an odd width with uneven shards, after one call and
# after three (the later selections read the other ranks' counts); full 16-byte rows; the BVH scene's guides
MAIN = [("07", 67, 45, s, k) for k in (1, 3) for s in (1, 2, 3, 8)] + [("04_box", 64, 36, 8, 1), ("stress", 96, 54, 8, 1)]
# contexts beyond the height (their blocks are NaN-filled by hand) and one pixel
TINY = [("07", 5, 3, 2, 1), ("07", 5, 3, 8, 1), ("07", 1, 1, 1, 1)]
FILTER = [("07", 67, 45, 3, 1), ("07", 67, 45, 8, 3), ("04_box", 64, 36, 8, 1), ("stress", 96, 54, 8, 1)]


@pytest.fixture(scope="module")
def cases(bwrt_lib):
    """(scene, w, h, shards, calls) -> (the oracle context, the shard contexts), made once."""
    made = {}

    def get(name, w, h, s, k):
        key = (name, w, h, s, k)
        if key not in made:
            seq = K.sequence(w, h, k)
            made[key] = (K.full_after(bwrt_lib, name, w, h, seq), K.shards_after(bwrt_lib, name, w, h, s, seq))
        return made[key]

    yield get
    for full, rs in made.values():
        M.close([full] + rs)


def call_multi(lib, ctxs, planes=0, dst=0):
    arr = (C.c_void_p * len(ctxs))(*[r.ctx.value for r in ctxs])
    return lib.rt_assemble_adaptive_multi(arr, len(ctxs), planes, dst)


def test_abi_declares_the_entry_points(bwrt_lib):
    names = {"rt_export_shard_adaptive", "rt_export_shard_adaptive_device", "rt_assemble_adaptive",
             "rt_assemble_adaptive_device", "rt_assemble_adaptive_multi", "rt_get_assembled_counts"}
    assert names <= set(abi.declared_functions())
    for n in names:
        assert hasattr(bwrt_lib, n)


# ---- 1. the assembled planes are the full frame's ----------------------------------------------------------
@pytest.mark.parametrize("name,w,h,s,k", MAIN + TINY)
def test_assembled_planes_equal_full_frame(cases, name, w, h, s, k):
    full, rs = cases(name, w, h, s, k)
    want = K.frame_of(full, w, h)
    if (name, w, h, s, k) in MAIN:  # the guard: a path that ignored the counts could not pass
        print(f"{name} {w}x{h} after {k} calls: n_p values {np.unique(want['n'])}")
        assert len(np.unique(want["n"])) >= 2
    for planes in (4, 7):
        own = K.shard_state(rs[0], K.rows_of(h, s, 0), w)
        g, n, j = K.gather(rs, w, h, planes)
        assert (n, j) == K.BASE == (full.frame_counter - 1, full.moments_batches)
        rs[0].assemble_adaptive(g, n, j)
        assert K.shard_state(rs[0], K.rows_of(h, s, 0), w) == own
        assert rs[0].assembled() == (n, j if planes == 7 else 0)
        got = K.assembled_of(rs[0], w, h, planes)
        for key in got:
            if key == "j" and planes == 4:
                assert not got["j"].any()  # no moments: no batch is tracked
            else:
                assert K.same(got[key], want[key]), (planes, key)
        if planes == 7:  # M2 through the filter that reads it: every pixel tracked (J_p >= 3)
            kw = dict(want_color=True, want_var=True, min_batches=2)
            assert K.same(rs[0].denoise_var(w, h, **kw), full.denoise_var(w, h, **kw))


# ---- 2. the filters on the counted assembled frame ---------------------------------------------------------
@pytest.mark.parametrize("name,w,h,s,k", FILTER)
def test_filters_equal_full_frame(cases, name, w, h, s, k):
    full, rs = cases(name, w, h, s, k)
    j = full.counts(h, w)[1]
    mixed = K.mixed_min_batches(j)  # (asserts that tracked and spatial pixels both occur)
    assert len(np.unique(full.counts(h, w)[0])) >= 2
    want = K.filter_outputs(full, w, h, mixed)
    assert not K.same(want["var_mixed"], want["var_spatial"])  # the choice shows in the output
    for planes in (7, 4):
        K.assemble_on(rs, w, h, planes)
        got = K.filter_outputs(rs[0], w, h, mixed, planes)
        exp = K.expected(want, planes)
        for name_ in got:
            assert K.same(got[name_], exp[name_]), (planes, name_)


def test_counts_decide_the_filters(cases):
    """The guard of section 2 on the oracle alone: the filters' outputs on the
    non-uniform frame differ from those on the same frameSum read with one count."""
    name, w, h, s, k = FILTER[0]
    full, rs = cases(name, w, h, s, k)
    K.assemble_on(rs, w, h, 7)
    counted = rs[0].denoise(w, h, iterations=1, want_color=True)
    g = K.gather(rs, w, h, 7)[0]
    rs[0].assemble(np.ascontiguousarray(g[:, :5]), *K.BASE)  # the same planes as an uncounted frame of 7 frames
    assert not K.same(rs[0].denoise(w, h, iterations=1, want_color=True), counted)
    K.assemble_on(rs, w, h, 7)
    assert K.same(rs[0].denoise(w, h, iterations=1, want_color=True), counted)


@pytest.mark.parametrize("s", [3, 8])
def test_temporal_equals_full_frame(bwrt_lib, s):
    name, w, h = "07", 67, 45
    (p,) = K.sequence(w, h, 1)
    for planes in (7, 4):
        full = M.contexts(bwrt_lib, M.scene_of(name), w, h, 1)
        rs = M.contexts(bwrt_lib, M.scene_of(name), w, h, s)
        try:
            for r in full + rs:
                r.set_adaptive_filters(True)
            want = K.temporal_outputs(full, w, h, p)
            got = K.temporal_outputs(rs, w, h, p, assemble=lambda: K.assemble_on(rs, w, h, planes))
            assert len(want) == 4
            for i, (a, b) in enumerate(zip(got, want)):
                assert K.same(a, b), (planes, i)
            assert len(np.unique(full[0].counts(h, w)[0])) >= 2
            assert want[2][2].max() > K.BASE[0]  # the second view did reproject history
            assert len(np.unique(want[0][2])) >= 2  # per-pixel lengths: the counts reached the blend
        finally:
            M.close(full + rs)


# ---- 3. a uniform accumulation through the counted path ----------------------------------------------------
def test_uniform_state_through_the_counted_path(bwrt_lib):
    w, h, s = 67, 45, 4
    scene = scenes.scene_07()
    rs = A.shard_contexts(bwrt_lib, scene, w, h, s)
    twin = A.shard_contexts(bwrt_lib, scene, w, h, s)[1]
    try:
        for r in rs:
            r.set_adaptive_filters(True)
        for counted, plain in ((7, 5), (4, 3)):
            A.assemble_on(rs, w, h, plain)
            want = A.filter_outputs(rs[0], w, h, spatial_only=plain == 3)
            want_t = rs[0].temporal(w, h, want_color=True, want_length=True)
            plain_frame = A.bits(rs[0].get_assembled(w, h, want_moments=plain == 5))
            g, n, j = K.assemble_on(rs, w, h, counted)
            assert (n, j) == K.BASE
            assert A.bits(rs[0].get_assembled(w, h, want_moments=counted == 7)) == plain_frame
            cn, cj = rs[0].assembled_counts(w, h)
            assert (cn == n).all() and (cj == (j if counted == 7 else 0)).all()
            got = A.filter_outputs(rs[0], w, h, spatial_only=plain == 3)
            for name in want:
                assert A.same(got[name], want[name]), (counted, name)
            rs[0].temporal_reset()
            assert A.same(rs[0].temporal(w, h, want_color=True, want_length=True), want_t)
            rs[0].temporal_reset()
        # the exporting context goes on as one that never exported
        for x in (rs[1], twin):
            x.render(w, h, 2, A.BOUNCES, row_offset=1, row_stride=s)
        rows = K.rows_of(h, s, 1)
        assert K.shard_state(rs[1], rows, w) == K.shard_state(twin, rows, w)
        assert A.same(rs[1].export_shard(rows, w, 5), twin.export_shard(rows, w, 5))
    finally:
        M.close(rs + [twin])


# ---- 4. the switch, and which frame a context has ---------------------------------------------------------
def test_switch_and_replacement(cases):
    name, w, h, s, k = FILTER[0]
    full, rs = cases(name, w, h, s, k)
    lib, r = rs[0].lib, rs[0]
    dn, dv, tp = r.denoise_params(), r.denoise_var_params(), r.temporal_params()
    passes = [lambda: lib.rt_denoise(r.ctx, C.byref(dn), None, None),
              lambda: lib.rt_denoise_var(r.ctx, C.byref(dv), None, None, None),
              lambda: lib.rt_temporal(r.ctx, C.byref(tp), None, None, None, None)]
    g7, n, j = K.gather(rs, w, h, 7)
    plain = np.ascontiguousarray(g7[:, :5])
    try:
        # an uncounted frame is served whatever the switch says and although the shard itself is non-uniform
        r.assemble(plain, n, j)
        served = A.filter_outputs(r, w, h)
        r.set_adaptive_filters(False)
        assert A.same(A.filter_outputs(r, w, h), served)
        bad = abi.RT_ERR_INVALID_ARGUMENT
        assert lib.rt_get_assembled_counts(r.ctx, None, None) == bad and b"no counts" in lib.rt_last_error(r.ctx)
        # a counted one replaces it and is refused with the switch off
        r.assemble_adaptive(g7, n, j)
        assert lib.rt_get_assembled_counts(r.ctx, None, None) == abi.RT_OK
        for call in passes:
            assert call() == abi.RT_ERR_UNSUPPORTED and b"non-uniform" in lib.rt_last_error(r.ctx)
        # rt_assemble replaces the counted frame: served again, and the counts are gone
        r.assemble(plain, n, j)
        assert A.same(A.filter_outputs(r, w, h), served)
        assert lib.rt_get_assembled_counts(r.ctx, None, None) == bad
        # and the reverse, with the switch on
        r.set_adaptive_filters(True)
        r.assemble_adaptive(g7, n, j)
        mixed = K.mixed_min_batches(full.counts(h, w)[1])
        assert K.same(K.filter_outputs(r, w, h, mixed), K.filter_outputs(full, w, h, mixed))
        r.temporal_reset()
    finally:
        r.set_adaptive_filters(True)
        r.temporal_reset()


# ---- 5. the invariants around the calls ------------------------------------------------------------------
def test_argument_errors_leave_the_assembled_frame(cases):
    name, w, h, s, k = FILTER[0]
    full, rs = cases(name, w, h, s, k)
    lib, r = rs[0].lib, rs[0]
    g, n, j = K.assemble_on(rs, w, h, 7)
    kept = A.bits((r.get_assembled(w, h, want_moments=True), r.assembled_counts(w, h)))
    own = K.shard_state(r, K.rows_of(h, s, 0), w)
    rps = g.shape[2]
    gp = g.ctypes.data
    blk = np.empty((7, rps, w), np.float32)
    bp = blk.ctypes.data
    bad = abi.RT_ERR_INVALID_ARGUMENT
    calls = [
        lambda: lib.rt_assemble_adaptive(None, gp, s, rps, 7, n, j),
        lambda: lib.rt_assemble_adaptive(r.ctx, None, s, rps, 7, n, j),
        lambda: lib.rt_assemble_adaptive(r.ctx, gp, s, rps, 5, n, j),
        lambda: lib.rt_assemble_adaptive(r.ctx, gp, s, rps, 3, n, j),
        lambda: lib.rt_assemble_adaptive(r.ctx, gp, s, rps, 6, n, j),
        lambda: lib.rt_assemble_adaptive(r.ctx, gp, 0, rps, 7, n, j),
        lambda: lib.rt_assemble_adaptive(r.ctx, gp, s, rps - 1, 7, n, j),  # 3 * 14 < 45
        lambda: lib.rt_assemble_adaptive(r.ctx, gp, s, rps, 7, 0, j),
        lambda: lib.rt_assemble(r.ctx, gp, s, rps, 7, n, j),  # the uncounted call takes no counted block
        lambda: lib.rt_export_shard_adaptive(None, rps, 7, bp, None, None),
        lambda: lib.rt_export_shard_adaptive(r.ctx, rps, 7, None, None, None),
        lambda: lib.rt_export_shard_adaptive(r.ctx, rps, 5, bp, None, None),
        lambda: lib.rt_export_shard_adaptive(r.ctx, rps, 3, bp, None, None),
        lambda: lib.rt_export_shard_adaptive(r.ctx, K.rows_of(h, s, 0) - 1, 4, bp, None, None),
    ]
    for i, call in enumerate(calls):
        assert call() == bad, i
        assert r.assembled() == (n, j), i
    assert lib.rt_export_shard_adaptive_device(r.ctx, rps, 4, bp, None, None, None) == abi.RT_ERR_UNSUPPORTED
    assert lib.rt_assemble_adaptive_device(r.ctx, gp, s, rps, 7, n, j, None) == abi.RT_ERR_UNSUPPORTED  # CPU context
    assert lib.rt_get_assembled_counts(None, None, None) == bad
    # the existing entry points keep refusing the non-uniform accumulation
    for planes in (3, 5):
        assert lib.rt_export_shard(r.ctx, rps, planes, bp, None, None) == abi.RT_ERR_UNSUPPORTED
    arr = (C.c_void_p * s)(*[x.ctx.value for x in rs])
    assert lib.rt_assemble_multi(arr, s, 0, 0) == abi.RT_ERR_UNSUPPORTED
    assert A.bits((r.get_assembled(w, h, want_moments=True), r.assembled_counts(w, h))) == kept
    assert K.shard_state(r, K.rows_of(h, s, 0), w) == own
    # contexts without a scene / a frame shape / a frame / current moments
    with Renderer.cpu(1, lib=lib) as e:
        assert lib.rt_assemble_adaptive(e.ctx, gp, s, rps, 7, n, j) == abi.RT_ERR_NO_SCENE
        e.set_scene(M.scene_of(name))
        assert lib.rt_assemble_adaptive(e.ctx, gp, s, rps, 7, n, j) == bad and b"frame shape" in lib.rt_last_error(e.ctx)
        e.init_rand(w, h, 0, s)
        assert lib.rt_export_shard_adaptive(e.ctx, rps, 4, bp, None, None) == bad  # nothing accumulated
        assert lib.rt_get_assembled_counts(e.ctx, None, None) == bad  # none made
        e.render(w, h, 2, A.BOUNCES, row_offset=0, row_stride=s)  # moments off
        assert lib.rt_export_shard_adaptive(e.ctx, rps, 7, bp, None, None) == bad
        assert lib.rt_export_shard_adaptive(e.ctx, rps, 4, bp, None, None) == abi.RT_OK
        assert lib.rt_assemble_adaptive(e.ctx, gp, s, rps, 7, n, j) == abi.RT_OK  # a frame shape is enough
        e.set_adaptive_filters(True)
        assert e.assembled() == (n, j) and e.last_assemble_ms() >= 0.0
        assert K.same(K.assembled_of(e, w, h, 7), K.frame_of(full, w, h))


def test_padding_is_zero_filled_and_never_read(cases):
    name, w, h, s, k = FILTER[0]
    full, rs = cases(name, w, h, s, k)
    rps = -(-h // s) + 1  # one row more than needed: every block has padding
    for planes in (4, 7):
        g, n, j = K.gather(rs, w, h, planes, rows_per_shard=rps)
        for i in range(s):
            rows = K.rows_of(h, s, i)
            assert not g[i, :, rows:].view(np.uint32).any(), i  # zero words, the count planes' too
            assert g[i, -1, :rows].view(np.uint32).all()  # (the last plane: n_p or J_p, never 0)
            g[i, :, rows:].view(np.uint32)[...] = 0x7fc00123 + i  # NaN bit patterns
        rs[0].assemble_adaptive(g, n, j)
        want = K.frame_of(full, w, h)
        got = K.assembled_of(rs[0], w, h, planes)
        for key in got:
            if not (key == "j" and planes == 4):
                assert K.same(got[key], want[key]), (planes, key)


def test_copies_keep_every_bit(bwrt_lib):
    """NaN payloads in the float planes and arbitrary integers in the count planes pass an assembly unchanged."""
    w, h, s = 8, 5, 2
    rps = 3
    with Renderer.cpu(1, lib=bwrt_lib) as e:
        e.set_scene(scenes.scene_07())
        e.init_rand(w, h, 1, s)
        rng = np.random.default_rng(7)
        g = rng.integers(0, 1 << 32, (s, 7, rps, w), dtype=np.uint64).astype(np.uint32)
        g[0, 0, 0, 0], g[1, 3, 1, 2], g[0, 5, 0, 1], g[1, 6, 0, 3] = 0x7fc00abc, 0xffc12345, 0x7fa00001, 0x00000001
        e.assemble_adaptive(g.view(np.float32), 1, 1)
        acc, mom = e.get_assembled(w, h, want_moments=True)
        n, j = e.assembled_counts(w, h)
        for y in range(h):
            blk = g[y % s, :, y // s]
            assert np.array_equal(acc[y].view(np.uint32), blk[:3].T)
            assert np.array_equal(mom[y].view(np.uint32), blk[3:5].T)
            assert np.array_equal(n[y], blk[5]) and np.array_equal(j[y], blk[6])


def test_currency_and_drop(bwrt_lib):
    name, w, h, s = "07", 16, 9, 3
    lib = bwrt_lib
    seq = M.sequence(2, ks=(3,), min_frames=8)  # (every pixel forced: the frame is small)
    rs = K.shards_after(lib, name, w, h, s, seq)
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
        refused(stale=False)  # never assembled
        g, n, j = K.assemble_on(rs, w, h, 7)
        want = A.bits([r.denoise(w, h, want_color=True), r.denoise_var(w, h, want_color=True, want_var=True)])

        def served():
            return A.bits([r.denoise(w, h, want_color=True), r.denoise_var(w, h, want_color=True, want_var=True)])

        # a snapshot: the shard's own accumulation may restart and move on
        r.reset_accumulation()
        assert r.assembled() == (n, j) and served() == want
        r.render(w, h, 2, A.BOUNCES, first_frame=1, row_offset=0, row_stride=s)
        assert r.assembled() == (n, j) and served() == want
        r.assemble_drop()
        refused(stale=False)
        cam = r.get_camera()
        for end in (lambda: r.set_camera(cam), lambda: r.controls(["LEFT"], A.DT),
                    lambda: r.set_scene(M.scene_of(name)),
                    lambda: r.render(w + 1, h, 1, A.BOUNCES, row_offset=0, row_stride=s)):
            r.init_rand(w, h, 0, s)
            r.assemble_adaptive(g, n, j)
            assert r.assembled() == (n, j)
            assert r.controls([], A.DT) == 0 and r.assembled() == (n, j)  # no key: no movement
            end()
            refused(stale=True)
    finally:
        M.close(rs)


# ---- 6. rt_assemble_adaptive_multi -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 8])
def test_assemble_adaptive_multi(bwrt_lib, n):
    name, w, h = "07", 33, 17
    lib = bwrt_lib
    seq = M.sequence(2, ks=(3, 1))
    full = K.full_after(lib, name, w, h, seq)
    rs = M.contexts(lib, M.scene_of(name), w, h, n)
    try:
        for p in seq:
            render_adaptive_multi(rs, w, h, M.BOUNCES, **p)
        for r in rs:
            r.set_adaptive_filters(True)
        want = K.frame_of(full, w, h)
        assert len(np.unique(want["n"])) >= 2
        mixed = K.mixed_min_batches(want["j"])
        outs = K.filter_outputs(full, w, h, mixed)
        for dst in sorted({0, n - 1}):
            for planes in (0, 7, 4):
                rs[dst].assemble_drop()
                own = [K.shard_state(r, K.rows_of(h, n, i), w) for i, r in enumerate(rs)]
                assert assemble_adaptive_multi(rs, planes, dst) == (K.BASE[0], 0 if planes == 4 else K.BASE[1])
                assert [K.shard_state(r, K.rows_of(h, n, i), w) for i, r in enumerate(rs)] == own
                p = planes or 7
                got = K.assembled_of(rs[dst], w, h, p)
                for key in got:
                    if not (key == "j" and p == 4):
                        assert K.same(got[key], want[key]), (dst, planes, key)
                if n > 1:  # (a context with offset 0 and stride 1 reads its own accumulation)
                    got = K.filter_outputs(rs[dst], w, h, mixed, p)
                    exp = K.expected(outs, p)
                    for key in got:
                        assert K.same(got[key], exp[key]), (dst, planes, key)
        # refusals touch nothing
        for r in rs:
            r.assemble_drop()
        bad = abi.RT_ERR_INVALID_ARGUMENT
        assert call_multi(lib, rs + rs[:1]) == bad  # listed twice (and the wrong stride)
        assert call_multi(lib, rs, 3) == bad and call_multi(lib, rs, 5) == bad
        assert call_multi(lib, rs, 0, n) == bad and call_multi(lib, rs, 0, -1) == bad
        assert lib.rt_assemble_adaptive_multi(None, n, 0, 0) == bad
        if n > 1:
            assert call_multi(lib, rs[::-1]) == bad  # wrong shard offsets
            rs[-1].reset_accumulation()
            rs[-1].render(w, h, 1, A.BOUNCES, row_offset=n - 1, row_stride=n)
            assert call_multi(lib, rs) == bad and b"frame counters" in lib.rt_last_error(rs[0].ctx)
        assert all(r.assembled() is None for r in rs)
    finally:
        M.close([full] + rs)


def test_assemble_adaptive_multi_mixed_states(bwrt_lib):
    """Some contexts uniform and some not; planes 0 in both outcomes."""
    name, w, h, n = "07", 33, 17, 3
    lib = bwrt_lib
    rs = M.contexts(lib, M.scene_of(name), w, h, n)
    try:
        for r in rs:
            r.set_adaptive_filters(True)
        # context 1 alone becomes non-uniform: the three-shard blocks of one export, its phase 2 only
        p = M.sequence(2, ks=(2,), min_frames=8)[0]
        g = M.export_all(rs, w, h, p)
        rs[1].render_adaptive_shard(g, K.rows_of(h, n, 1), w, M.BOUNCES, **p)
        assert assemble_adaptive_multi(rs, 0, 0) == K.BASE  # every context's moments current: 7 planes
        cn, cj = rs[0].assembled_counts(w, h)
        assert (cn[1::n] == 9).all() and (cj[1::n] == 4).all()
        for i in (0, 2):
            assert (cn[i::n] == 7).all() and (cj[i::n] == 3).all()
        acc, mom = rs[0].get_assembled(w, h, want_moments=True)
        for i, r in enumerate(rs):
            rows = K.rows_of(h, n, i)
            assert K.same(acc[i::n], r.get_state(rows, w)[1]) and K.same(mom[i::n, :, 0], r.variance(rows, w, True)[1])
        # the filters take the mixture: not what one count for all pixels gives
        counted = rs[0].denoise(w, h, iterations=1, want_color=True)
        rs[0].assemble(np.ascontiguousarray(K.gather(rs, w, h, 7)[0][:, :5]), *K.BASE)
        assert not K.same(rs[0].denoise(w, h, iterations=1, want_color=True), counted)
        # one context's moments not current: 0 falls back to 4, and 7 is refused
        rs[2].set_moments(False)
        rs[0].assemble_drop()
        assert call_multi(lib, rs, 7) == abi.RT_ERR_INVALID_ARGUMENT and rs[0].assembled() is None
        assert assemble_adaptive_multi(rs, 0, 0) == (K.BASE[0], 0)
        assert lib.rt_get_assembled(rs[0].ctx, None, acc.ctypes.data) == abi.RT_ERR_INVALID_ARGUMENT  # no moments
        cn2, cj2 = rs[0].assembled_counts(w, h)
        assert K.same(cn2, cn) and not cj2.any()
    finally:
        M.close(rs)


# ---- 7. thread counts --------------------------------------------------------------------------------------
def test_thread_count_invariance(bwrt_lib):
    name, w, h, s = "07", 67, 45, 4
    seq = K.sequence(w, h, 1)
    got = []
    for threads in (1, 5):
        rs = K.shards_after(bwrt_lib, name, w, h, s, seq, threads=threads)
        g, n, j = K.assemble_on(rs, w, h, 7)
        got.append(A.bits((g, rs[0].get_assembled(w, h, want_moments=True), rs[0].assembled_counts(w, h))))
        M.close(rs)
    assert got[0] == got[1]


# ---- 8. the four plane counts are one layout -----------------------------------------------------------------
@pytest.mark.parametrize("w,h,s", K.LAYOUT_SHAPES)
def test_plane_counts_are_one_layout(bwrt_lib, w, h, s):
    """Blocks of 3, 5, 4 and 7 planes of the same contexts hold the same words
    in the planes they share, and assemble to the same frame (K.one_layout)."""
    blocks = K.one_layout(bwrt_lib, w, h, s)
    assert set(blocks) == {("uniform", p) for p in (3, 5, 4, 7)} | {("adaptive", p) for p in (4, 7)}
