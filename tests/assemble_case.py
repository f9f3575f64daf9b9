"""What the assembled-frame tests share (tests/test_assemble.py on the CPU
backend, tests/test_gpu_assemble.py on the GPU): one full-frame context as the
oracle, S shard contexts of the same frame, their gathered blocks, and the
outputs of every full-frame pass.

The premise (ISSUE / DESIGN.md section 17): pixels are independent, so the
shards' frameSum and moments, interleaved, are a single full-frame context's
bit for bit; a filter that reads the assembled frame must therefore give that
context's bits.
"""
import numpy as np

from bwrt import Renderer

CALLS = (2, 2, 3)  # frames per render call: three tracked batches, seven frames
BOUNCES = 4
DT = 0.01


def new(lib, gpu=False, threads=0):
    return Renderer(0, lib=lib) if gpu else Renderer.cpu(threads, lib=lib)


def accumulate(r, w, h, off=0, stride=1, calls=CALLS, restart=True):
    for i, k in enumerate(calls):
        r.render(w, h, k, BOUNCES, first_frame=1 if restart and i == 0 else 0, row_offset=off, row_stride=stride)


def full_context(lib, scene, w, h, gpu=False, moments=True):
    r = new(lib, gpu)
    r.set_scene(scene)
    r.set_moments(moments)
    accumulate(r, w, h)
    return r


def shard_contexts(lib, scene, w, h, shards, gpu=False, moments=True, threads=0):
    """`shards` contexts, context i with rows i (mod shards) accumulated;
    contexts beyond the height have a scene and nothing else."""
    rs = []
    for i in range(shards):
        r = new(lib, gpu, threads)
        r.set_scene(scene)
        r.set_moments(moments)
        if i < h:
            accumulate(r, w, h, i, shards)
        rs.append(r)
    return rs


def rows_of(h, shards, i):
    return len(range(i, h, shards))


def gather(rs, w, h, planes, rows_per_shard=None, fill=np.nan):
    """(gathered, frames, batches): every context's exported block; the blocks
    of contexts without rows are made by hand (`fill`: assembly never reads them)."""
    shards = len(rs)
    rps = rows_per_shard or -(-h // shards)
    g = np.full((shards, planes, rps, w), fill, np.float32)
    counts = set()
    for i, r in enumerate(rs):
        if i < h:
            g[i], n, j = r.export_shard(rps, w, planes)
            counts.add((n, j))
    assert len(counts) == 1, counts
    n, j = counts.pop()
    return g, n, j


def assemble_on(rs, w, h, planes, dst=0):
    g, n, j = gather(rs, w, h, planes)
    rs[dst].assemble(g, n, j)
    return g, n, j


def bits(x):
    """A result as bytes: equality is bit for bit, NaN payloads included."""
    if isinstance(x, dict):
        return tuple((k, bits(v)) for k, v in sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return tuple(bits(v) for v in x)
    return np.ascontiguousarray(x).tobytes()


def same(a, b):
    return bits(a) == bits(b)


def same_values(a, b):
    """Equal values, any NaN equal to any NaN: what a GPU context and a CPU
    context agree on (their renders give NaNs of different sign bits, e.g. on
    the 1x1 frame, whose camera rays are NaN; the copies keep whatever bits
    they are given, which `same` checks within one backend)."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_values(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_values(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def interleave(rs, w, h):
    """The full frame's frameSum from the shard contexts' own state (rt_get_state)."""
    out = np.empty((h, w, 3), np.float32)
    for i, r in enumerate(rs):
        if i < h:
            out[i::len(rs)] = r.get_state(rows_of(h, len(rs), i), w)[1]
    return out


def filter_outputs(r, w, h, spatial_only=False):
    """Every filter of the issue's list on the frame r reads: rt_denoise at 0,
    1 and 5 levels (RGBA, colour), rt_denoise_var with the tracked variance
    (min_batches 2 <= J = 3) and with the spatial estimate (min_batches 4 > J),
    each (RGBA, colour, variance).  spatial_only: the frame has no moments, so
    min_batches 2 must also give the spatial estimate."""
    out = {}
    for it in (0, 1, 5):
        out[f"denoise{it}"] = r.denoise(w, h, iterations=it, want_color=True)
    if not spatial_only:
        out["var_tracked"] = r.denoise_var(w, h, want_color=True, want_var=True, min_batches=2)
    out["var_spatial"] = r.denoise_var(w, h, want_color=True, want_var=True, min_batches=2 if spatial_only else 4)
    return out


def temporal_outputs(rs, w, h, assemble=None, dst=0):
    """The two-view sequence: (render), assemble, temporal; LEFT on every
    context; render, assemble, temporal.  Each temporal step runs without and
    with the filter (the second call of a view replaces its pending result and
    leaves the history alone), each (RGBA, colour, length)."""
    out = []
    for view in range(2):
        if view:
            for i, r in enumerate(rs):
                r.controls(["LEFT"], DT)
                if i < h:
                    accumulate(r, w, h, i if len(rs) > 1 else 0, len(rs), restart=False)
        if assemble:
            assemble()
        for dn in (None, {"iterations": 2}):
            out.append(rs[dst].temporal(w, h, denoise=dn, want_color=True, want_length=True))
    return out
