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
