"""The device pass of csrc/rt_light.h on the MI355X, function by function:
tools/nee_probe.hip built as the two NEE kernel units are (build/neeprobe,
build/neeprobe_bvh) runs the case sets of tests/test_nee_reference.py — one
case per lane, 256-lane blocks, the table in global memory — and every device
output word must equal the word of the header's host pass in the same run; a
NaN equals any NaN.  The device words then meet the conditions of the float64
reference (tests/nee_ref.py, stated in tests/nee_cases.py) on their own.

build/neeprobe runs every set, build/neeprobe_bvh (the same header under the
BVH unit's flags) the sphere, divergent and edge-table sets.  Each (binary,
function, table) runs once and is shared, read-only.  Once a probe run ends
in anything but success — a signal, an abort, its time-out, a HIP error — no
further probe is launched in the session and the remaining tests fail without
running anything.

Behind them: renders of two scenes with one small sphere light (s2 about 1e-4
from the lit floor), GPU against the CPU twin, which carry the sphere cone of
nee_sample through the brute-force and the BVH kernels.
"""
import os
import subprocess

import numpy as np
import pytest

import nee_cases as K
import nee_ref as R
from bwrt import Renderer
from test_gpu_light_sampling import same_state
from test_light_sampling import state

pytestmark = pytest.mark.gpu

BINARIES = {"neeprobe": os.path.join(K.BUILD, "neeprobe"), "neeprobe_bvh": os.path.join(K.BUILD, "neeprobe_bvh")}
RUNS = K.SAMPLE_RUNS + K.OTHER_RUNS
BVH_RUNS = [("07", 0), ("07", 1), ("eight_lights", 0), ("eight_lights", 1), ("decade4", 0), ("decade7", 0), K.DIVERGENT_RUN,
            ("mixed", 2), ("quad_1_3", 2), ("quad_1_3", 3), ("twins", 1), ("exact_r2", 0), ("origin_quad", 2), ("underflow", 1),
            ("zero_first", 1)] + K.OTHER_RUNS[:1] + K.OTHER_RUNS[2:]
assert set(BVH_RUNS) <= set(RUNS)
PAIRS = [("neeprobe", t, f) for t, f in RUNS] + [("neeprobe_bvh", t, f) for t, f in BVH_RUNS]
# the float words of a function's output (a NaN there equals any NaN)
FLOAT_WORDS = {0: [3, 4, 5, 6], 1: [3, 4, 5, 6], 2: [3, 4, 5, 6], 3: [3, 4, 5, 6], 4: [0], 5: [0], 6: [], 7: [], 8: [0, 1, 2], 9: []}
OUT_WORDS = {0: 13, 1: 13, 2: 13, 3: 13, 4: 1, 5: 1, 6: 1, 7: 1, 8: 3, 9: 1}

_CACHE = {}
_REFS = {}
_DEAD = []


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    t = K.dump_tables(tmp_path_factory.mktemp("nee_tables"))
    t.update(K.crafted_tables())
    for v in t.values():
        v.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def probe(tables, tmp_path_factory):
    """probe(binary, table, fid) -> (table words, cases, random mask, device words, host words)"""
    d = tmp_path_factory.mktemp("neeprobe")

    def run(binary, table, fid):
        key = (binary, table, fid)
        if key not in _CACHE:
            if _DEAD:
                pytest.fail(f"no probe is launched any more: {_DEAD[0]}")
            words, cases, random = K.run_inputs(tables, table, fid)
            try:
                r, dev, host = K.run_probe([BINARIES[binary]], fid, words, cases, d)
            except subprocess.TimeoutExpired:
                _DEAD.append(f"{key} ran into its time-out")
                raise
            if r.returncode != 0:
                _DEAD.append(f"{key} ended with status {r.returncode}: {r.stderr.strip()[-200:]}")
                pytest.fail(_DEAD[0])
            assert len(dev) == len(host) == len(cases) * OUT_WORDS[fid]
            for a in (cases, dev, host):
                a.setflags(write=False)
            _CACHE[key] = (words, cases, random, dev, host)
        return _CACHE[key]
    return run


@pytest.mark.parametrize("binary,table,fid", PAIRS, ids=[f"{b}-{t}-{f}" for b, t, f in PAIRS])
def test_device_pass_equals_host_pass_and_meets_the_reference(tables, probe, binary, table, fid):
    words, cases, random, dev, host = probe(binary, table, fid)
    n = OUT_WORDS[fid]
    d, h = dev.reshape(-1, n), host.reshape(-1, n)
    same = d == h
    for col in FLOAT_WORDS[fid]:
        same[:, col] |= np.isnan(d[:, col].view(np.float32)) & np.isnan(h[:, col].view(np.float32))
    bad = np.nonzero(~same.all(1))[0]
    assert len(bad) == 0, (len(bad), bad[:8], d[bad[:8]], h[bad[:8]])
    # the reference conditions, on the device words alone
    ref = None
    if fid <= 3:
        if (table, fid) not in _REFS:
            _REFS[table, fid] = K.sample_reference(words, fid, cases)
        ref = _REFS[table, fid]
    print(K.check_run(tables, table, fid, cases, random, dev, ref))
    if table.startswith("decade") and table[6:].isdigit():
        (m, got, ideal), = K.miss_shares(ref, cases, random, dev)
        print(f"s2 <= {K.DECADES[int(table[6:])]:g}: {m} traced, wi misses {got}, the rounded reference {ideal}")
        assert got <= 2 * ideal + 2.0 * m / 65536


def test_the_divergent_set_diverges(tables, probe):
    """The mixed table under the weighted, all-shapes pick (3 sphere and 4 quad
    lights): within the waves of its run, consecutive lanes pick spheres and
    polygons, carry kind 0, 1 and 2, are reachable and not, traced and not, and
    the second weight pass leaves its loop at different lights."""
    table, fid = K.DIVERGENT_RUN
    assert (table, fid) in RUNS
    words, cases, random, dev, host = probe("neeprobe", table, fid)
    out = dev.reshape(-1, 13)
    t, _ = R.table_from_words(words)
    j, trace, kind = out[:, 0].view(np.int32), out[:, 2], cases[:, 13].view(np.int32)
    waves = (len(cases) - 4096) // 64  # the random part
    poly = (j >= t["n_sphere_lights"])[:waves * 64].reshape(waves, 64)
    assert (poly.any(1) & ~poly.all(1)).mean() > 0.95
    assert (np.array([len(np.unique(w)) for w in j[:waves * 64].reshape(waves, 64)]) >= 4).mean() > 0.95
    assert all(len(np.unique(w)) == 3 for w in kind[:waves * 64].reshape(waves, 64))
    tr = trace[:waves * 64].reshape(waves, 64)
    assert ((tr != 0).any(1) & (tr == 0).any(1)).all()


# ---- renders with a small sphere light -------------------------------------------------------

@pytest.mark.parametrize("pick", ["uniform", "weighted"])
@pytest.mark.parametrize("mb", [1, 4])
@pytest.mark.parametrize("below,bvh", [(0, False), (64, True)])
def test_small_light_renders_equal_cpu(bwrt_lib, below, bvh, mb, pick):
    """A floor under one sphere light of s2 about 1e-4 (and, with 64 small dark
    spheres below the floor, the same through the BVH kernels): 32 x 18, 3
    frames, GPU against the CPU twin, frameSum, RNG state and RGBA."""
    scene = K.small_light_scene(below)
    res = []
    for make in (lambda: Renderer(0, lib=bwrt_lib), lambda: Renderer.cpu(0, lib=bwrt_lib)):
        with make() as r:
            r.set_scene(scene)
            r.set_light_sampling(True)
            r.set_light_picking(pick)
            res.append(state(r, 32, 18, 3, mb))
            if not res[1:]:
                name = r.last_kernel_name()
    same_state(res[0], res[1])
    assert name.startswith("rt_render_nee_kernel") and ("bvh" in name) == bvh and ("weighted" in name) == (pick == "weighted"), name
    assert np.isfinite(res[0][1]).all() and res[0][1].max() > 0  # the light reaches the floor
