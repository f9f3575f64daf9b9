"""What the tests of adaptive sampling on row shards share
(tests/test_adaptive_multi.py on the CPU backend, tests/test_gpu_adaptive_multi.py
on the GPU): one full-frame context as the oracle, S shard contexts of the same
frame, the same sequence of adaptive calls on both, and everything the two
leave behind.

The premise: pixels are independent and the window
arithmetic is specified operation by operation, so S shard contexts that
exchange their row sums end with, interleaved, exactly the bits of one context
that ran rt_render_adaptive on the whole frame.
"""
import numpy as np

import assemble_case as AC
from assemble_case import bits, rows_of, same, same_values  # noqa: F401  (the comparisons)
from bwrt import scenes

CALLS = AC.CALLS      # the uniform start: three tracked batches, seven frames
BOUNCES = AC.BOUNCES
KS = (3, 1, 4)        # frames of the three successive adaptive calls
DEFAULTS = dict(tolerance=0.1, lum_floor=0.01, radius=2)


def sequence(radius=2, ks=KS, **over):
    """One parameter dict per adaptive call."""
    return [dict(DEFAULTS, radius=radius, samples=k, **over) for k in ks]


def scene_of(name):
    return scenes.SCENES[name]()


def contexts(lib, scene, w, h, shards, gpu=False, threads=0, spp=1):
    """`shards` contexts accumulated as CALLS with the moments on; shards == 1
    is a full-frame context (offset 0, stride 1)."""
    rs = []
    for i in range(shards):
        r = AC.new(lib, gpu, threads)
        r.set_samples_per_pixel(spp)
        r.set_scene(scene)
        r.set_moments(True)
        if i < h:
            AC.accumulate(r, w, h, i, shards)
        rs.append(r)
    return rs


def close(rs):
    for r in rs:
        r.close()


def export_all(rs, w, h, params, rows_per_shard=None, fill=np.nan):
    """Phase 1 on every context with rows: the gathered blocks.  The blocks of
    contexts beyond the height are filled with `fill` (NaN: a read of one would
    poison the test, so equality also shows that none is read)."""
    shards = len(rs)
    rps = rows_per_shard or -(-h // shards)
    g = np.full((shards, 3, rps, w), fill, np.float32)
    for i, r in enumerate(rs):
        if i < h:
            g[i] = r.adaptive_export_rows(rps, w, **params)
    return g


def two_phase(rs, w, h, params, bounces=BOUNCES):
    """One adaptive call on the shard contexts by the two-phase entry points:
    (RGBA, colour) of the full frame, the sums of selected and frames_total."""
    shards = len(rs)
    g = export_all(rs, w, h, params)
    rgba = np.empty((h, w, 4), np.uint8)
    col = np.empty((h, w, 3), np.float32)
    sel = tot = 0
    for i, r in enumerate(rs):
        if i < h:
            a, c, st = r.render_adaptive_shard(g, rows_of(h, shards, i), w, bounces, want_color=True, **params)
            rgba[i::shards], col[i::shards] = a, c
            sel += st["selected"]
            tot += st["frames_total"]
    return {"rgba": rgba, "color": col, "selected": sel, "frames_total": tot}


def full_call(r, w, h, params, bounces=BOUNCES):
    """The same call on the oracle: rt_render_adaptive on the whole frame."""
    rgba, col, st = r.render_adaptive(w, h, bounces, want_color=True, **params)
    return {"rgba": rgba, "color": col, "selected": st["selected"], "frames_total": st["frames_total"]}


def snapshot(rs, w, h, variance=True):
    """The contexts' state, interleaved into the full frame: counts
    (rt_get_counts), RNG and frameSum (rt_get_state), variance and luminance
    (rt_get_variance; not with variance=False, for an accumulation of one
    batch).  Every pixel of the frame is written: no pixel is left out."""
    s = len(rs)
    out = {"n": np.empty((h, w), np.uint32), "j": np.empty((h, w), np.uint32), "rng": np.empty((6, h, w), np.uint32),
           "accum": np.empty((h, w, 3), np.float32), "var": np.empty((h, w), np.float32),
           "lum": np.empty((h, w), np.float32)}
    covered = np.zeros(h, bool)
    for i, r in enumerate(rs):
        if i >= h:
            continue
        rows = rows_of(h, s, i)
        out["n"][i::s], out["j"][i::s] = r.counts(rows, w)
        rng, acc = r.get_state(rows, w)
        out["rng"][:, i::s], out["accum"][i::s] = rng, acc
        if variance:
            out["var"][i::s], out["lum"][i::s] = r.variance(rows, w, want_lum=True)
        covered[i::s] = True
    assert covered.all()
    if not variance:
        del out["var"], out["lum"]
    return out


_ORACLES = {}


def oracle(lib, name, w, h, seq, gpu=False, bounces=BOUNCES, spp=1):
    """The full-frame context's results of `seq`: {"calls": [per call], "final":
    snapshot}; computed once per case, shared and kept unchanged."""
    key = (gpu, name, w, h, bits([sorted(p.items()) for p in seq]), bounces, spp)
    if key not in _ORACLES:
        (r,) = contexts(lib, scene_of(name), w, h, 1, gpu, spp=spp)
        res = {"calls": [full_call(r, w, h, p, bounces) for p in seq], "final": snapshot([r], w, h)}
        r.close()
        for d in res["calls"] + [res["final"]]:
            for v in d.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _ORACLES[key] = res
    return _ORACLES[key]


def run_shards(lib, name, w, h, shards, seq, gpu=False, bounces=BOUNCES, spp=1, threads=0, call=two_phase):
    rs = contexts(lib, scene_of(name), w, h, shards, gpu, threads, spp)
    try:
        return {"calls": [call(rs, w, h, p, bounces) for p in seq], "final": snapshot(rs, w, h)}
    finally:
        close(rs)


def assert_same(got, want, eq=same):
    """Every compared quantity by name, so a failure says which one differs."""
    assert len(got["calls"]) == len(want["calls"])
    for i, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        for k in ("selected", "frames_total"):
            assert a[k] == b[k], (i, k, a[k], b[k])
        for k in ("rgba", "color"):
            assert a[k].shape == b[k].shape and eq(a[k], b[k]), (i, k)
    for k in ("n", "j", "rng", "accum", "var", "lum"):
        assert got["final"][k].shape == want["final"][k].shape and eq(got["final"][k], want["final"][k]), k
