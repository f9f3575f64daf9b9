"""What the tests of counted assembled frames share
(tests/test_assemble_adaptive.py on the CPU backend,
tests/test_gpu_assemble_adaptive.py on the GPU).

The oracle is one full-frame context that ran the same rt_render_adaptive
sequence with rt_set_adaptive_filters on.  The shard contexts of
tests/adaptive_multi_case.py end with its counts, frameSum and moments,
interleaved (tests/test_adaptive_multi.py), so after a counted assembly the
root shard context's passes must give the oracle's bits.
"""
import numpy as np

import adaptive_multi_case as M
import assemble_case as A
from assemble_case import bits, rows_of, same, same_values  # noqa: F401  (the comparisons)

BOUNCES = M.BOUNCES
BASE = (sum(M.CALLS), len(M.CALLS))  # the uniform base: seven frames, three batches
BIG = 1 << 20                        # a min_batches above every J_p


def sequence(w, h, calls=1):
    """`calls` adaptive calls; the tiny frames, whose moments select nothing
    by themselves, are forced as in tests/test_adaptive_multi.py."""
    if (w, h) == (5, 3):
        return M.sequence(2, min_frames=9)[:calls]
    if (w, h) == (1, 1):
        return M.sequence(1, min_frames=8)[:calls]
    return M.sequence(2)[:calls]


def shards_after(lib, name, w, h, shards, seq, gpu=False, threads=0):
    """`shards` contexts accumulated as 2 + 2 + 3 frames with the moments on,
    then the adaptive calls of `seq`, the filter switch on."""
    rs = M.contexts(lib, M.scene_of(name), w, h, shards, gpu, threads)
    for p in seq:
        M.two_phase(rs, w, h, p)
    for r in rs:
        r.set_adaptive_filters(True)
    return rs


def full_after(lib, name, w, h, seq, gpu=False):
    """The oracle: one full-frame context after the same calls."""
    (r,) = M.contexts(lib, M.scene_of(name), w, h, 1, gpu)
    for p in seq:
        M.full_call(r, w, h, p)
    r.set_adaptive_filters(True)
    return r


def gather(rs, w, h, planes, rows_per_shard=None, fill=np.nan):
    """(gathered, frames, batches): every context's counted block; the blocks
    of contexts without rows are made by hand (`fill`: assembly never reads them)."""
    shards = len(rs)
    rps = rows_per_shard or -(-h // shards)
    g = np.full((shards, planes, rps, w), fill, np.float32)
    base = set()
    for i, r in enumerate(rs):
        if i < h:
            g[i], n, j = r.export_shard_adaptive(rps, w, planes)
            base.add((n, j))
    assert len(base) == 1, base
    n, j = base.pop()
    return g, n, j


def assemble_on(rs, w, h, planes, dst=0):
    g, n, j = gather(rs, w, h, planes)
    rs[dst].assemble_adaptive(g, n, j)
    return g, n, j


def frame_of(r, w, h):
    """The oracle's frame: frameSum, per-pixel counts and the mean luminance M
    (rt_get_variance's; M2 is checked through the filter that reads it)."""
    n, j = r.counts(h, w)
    return {"accum": r.get_state(h, w)[1], "n": n, "j": j, "lum": r.variance(h, w, want_lum=True)[1]}


def assembled_of(r, w, h, planes):
    n, j = r.assembled_counts(w, h)
    if planes == 7:
        acc, mom = r.get_assembled(w, h, want_moments=True)
        return {"accum": acc, "n": n, "j": j, "lum": mom[..., 0]}
    return {"accum": r.get_assembled(w, h), "n": n, "j": j}


def mixed_min_batches(j):
    """A min_batches that splits the frame's J_p: both kinds of pixel occur."""
    mb = int(j.max())
    assert mb >= 2 and (j >= mb).any() and (j < mb).any(), np.unique(j)
    return mb


def filter_outputs(r, w, h, mixed, planes=7):
    """rt_denoise at 0, 1 and 5 levels (RGBA, colour); rt_denoise_var (RGBA,
    colour, variance) with min_batches `mixed` and above every J_p.  A 4-plane
    frame has no moments: whatever min_batches says, it must give the oracle's
    all-spatial output, which the comparison maps both names to."""
    out = {f"denoise{it}": r.denoise(w, h, iterations=it, want_color=True) for it in (0, 1, 5)}
    kw = dict(want_color=True, want_var=True)
    out["var_mixed"] = r.denoise_var(w, h, min_batches=mixed, **kw)
    out["var_spatial"] = r.denoise_var(w, h, min_batches=BIG, **kw)
    if planes == 4:
        out["var_two"] = r.denoise_var(w, h, min_batches=2, **kw)
    return out


def expected(want, planes):
    """The oracle's outputs as a frame of `planes` planes must give them."""
    if planes == 7:
        return want
    exp = dict(want, var_mixed=want["var_spatial"], var_two=want["var_spatial"])
    return exp


def temporal_outputs(rs, w, h, params, assemble=None, dst=0):
    """Two views: (the contexts come accumulated) adaptive call, counted
    assembly, temporal without and with its filter; LEFT on every context, the
    ranks re-accumulate, adaptive call, assembly, temporal twice.  Each
    (RGBA, colour, length).  One context: rt_render_adaptive on the full frame."""
    out = []
    for view in range(2):
        if view:
            for i, r in enumerate(rs):
                r.controls(["LEFT"], A.DT)
                if i < h:
                    A.accumulate(r, w, h, i if len(rs) > 1 else 0, len(rs), restart=False)
        if assemble:
            M.two_phase(rs, w, h, params)
        else:
            M.full_call(rs[0], w, h, params)
        if assemble:
            assemble()
        for dn in (None, {"iterations": 2}):
            out.append(rs[dst].temporal(w, h, denoise=dn, want_color=True, want_length=True))
    return out


def shard_state(r, rows, w):
    """Everything a shard context holds of its own accumulation."""
    rng, acc = r.get_state(rows, w)
    var = r.variance(rows, w, want_lum=True) if r.moments_batches >= 2 else ()
    return bits((rng, acc, r.counts(rows, w)) + tuple(var)), r.frame_counter, r.moments_batches


# ---- the four plane counts are one layout ---------------------------------------------
# (width, height, shards): the 4-byte form; the 16-byte form; contexts beyond the height
LAYOUT_SHAPES = [(67, 45, 3), (64, 36, 8), (5, 3, 8)]
LAYOUT_CALLS = (2, 2, 2, 2)  # 4 x 2 tracked frames: n = 8, J = 4


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _layout_blocks(rs, w, h, rps, plane_counts):
    """planes -> (gathered, frames, batches) of the contexts' blocks with one
    padding row at least; the blocks of contexts without rows are zero."""
    out = {}
    for planes in plane_counts:
        g = np.zeros((len(rs), planes, rps, w), np.float32)
        base = set()
        for i, r in enumerate(rs[:h]):
            export = r.export_shard_adaptive if planes in (4, 7) else r.export_shard
            g[i], n, j = export(rps, w, planes)
            base.add((n, j))
            assert not _words(g[i, :, rows_of(h, len(rs), i):]).any(), (planes, i)  # padding rows are zero
        assert len(base) == 1, base
        out[planes] = (g, *base.pop())
    return out


def _layout_assembled(r, blocks, w, h):
    """planes -> what rs[0] holds after assembling that block: sum, and mom / (n, j) where the block has them"""
    got = {}
    for planes, (g, n, j) in blocks.items():
        (r.assemble_adaptive if planes in (4, 7) else r.assemble)(g, n, j)
        moments = planes in (5, 7)
        frame = r.get_assembled(w, h, want_moments=moments)
        got[planes] = {"sum": frame[0] if moments else frame}
        if moments:
            got[planes]["mom"] = frame[1]
        if planes in (4, 7):
            got[planes]["n"], got[planes]["j"] = r.assembled_counts(w, h)
    return got


def one_layout(lib, w, h, shards, gpu=False):
    """The blocks of 3, 5, 4 and 7 planes of one set of shard contexts agree
    word for word where they hold the same planes, and so do their assembled
    frames: in the uniform state for all four, after one adaptive call for 4
    and 7 (3 and 5 refuse).  Returns {(state, planes): gathered blocks}."""
    from bwrt import abi
    rs = []
    for i in range(shards):
        r = A.new(lib, gpu)
        r.set_scene(M.scene_of("07"))
        r.set_moments(True)
        if i < h:
            A.accumulate(r, w, h, i, shards, calls=LAYOUT_CALLS)
        rs.append(r)
    rps = -(-h // shards) + 1
    n, J = sum(LAYOUT_CALLS), len(LAYOUT_CALLS)
    kept = {}
    try:
        # uniform, current moments: all four
        blocks = _layout_blocks(rs, w, h, rps, (3, 5, 4, 7))
        u = {p: _words(b[0]) for p, b in blocks.items()}
        assert [(b[1], b[2]) for b in blocks.values()] == [(n, J)] * 4
        for p in (5, 4, 7):
            assert np.array_equal(u[p][:, :3], u[3]), p
        assert np.array_equal(u[5][:, 3:5], u[7][:, 3:5])
        assert np.array_equal(u[4][:, 3], u[7][:, 5])
        for i in range(min(shards, h)):
            rows = rows_of(h, shards, i)
            assert (u[4][i, 3, :rows] == n).all() and (u[7][i, 6, :rows] == J).all(), i
        got = _layout_assembled(rs[0], blocks, w, h)
        for p in (5, 4, 7):
            assert same(got[p]["sum"], got[3]["sum"]), p
        assert same(got[5]["mom"], got[7]["mom"])
        assert (got[4]["n"] == n).all() and not got[4]["j"].any()
        assert (got[7]["n"] == n).all() and (got[7]["j"] == J).all()
        kept.update({("uniform", p): b[0] for p, b in blocks.items()})
        # after one adaptive call: 4 and 7 only
        M.two_phase(rs, w, h, sequence(w, h)[0])
        scratch = np.empty((5, rps, w), np.float32)
        for r in rs[:h]:
            for p in (3, 5):
                assert r.lib.rt_export_shard(r.ctx, rps, p, scratch.ctypes.data, None, None) == abi.RT_ERR_UNSUPPORTED
                assert b"non-uniform" in r.lib.rt_last_error(r.ctx)
        blocks = _layout_blocks(rs, w, h, rps, (4, 7))
        u = {p: _words(b[0]) for p, b in blocks.items()}
        assert np.array_equal(u[4][:, :3], u[7][:, :3]) and np.array_equal(u[4][:, 3], u[7][:, 5])
        got = _layout_assembled(rs[0], blocks, w, h)
        assert same(got[4]["sum"], got[7]["sum"]) and same(got[4]["n"], got[7]["n"]) and not got[4]["j"].any()
        for i, r in enumerate(rs[:h]):
            cn, cj = r.counts(rows_of(h, shards, i), w)
            assert same(got[7]["n"][i::shards], cn) and same(got[7]["j"][i::shards], cj), i
        print(f"{w}x{h}, {shards} shards: n_p after the adaptive call {np.unique(got[7]['n'])}")
        kept.update({("adaptive", p): b[0] for p, b in blocks.items()})
    finally:
        M.close(rs)
    return kept
