"""Schedule invariance of the reference-fast precision mode (DESIGN.md section
8, "Tests").

FAST has no oracle: its bits are pinned to FAST's own plainest queued
schedule, the sorted kernel in 64-lane groups with LDS records, no sky table
and no launch order (rt_render_sorted_kernel<64,fast>).  Every other schedule
of the queued kernels calls the same rt_path.h functions on the same arguments
in another order, so RGBA8, frameSum (NaN equal to NaN) and RNG state must be
identical: kernel family (pair, sorted, sorted with global records), workgroup
size, sky table, launch-order feedback, row shards, call splitting, bounce
limits, ragged sizes; and for the BVH kernels node formats, octant masks and
refill schedules.  (Class S.)  The launch policy mixes these inside one frame
(row shards) and one accumulation (a view's first launch has neither table nor
order), so a frame must not depend on them.

Other arithmetic forms of the same scene are only counted (class A; the
oracle bar of test_gpu_precision.py holds them):
  * the one-path-per-lane kernel (BWRT_KERNEL=simple) against the queued
    kernels: the same source, but under -ffp-contract=fast the compiler
    contracts its instantiation of the shading code differently (measured:
    frameSum differs on 0.2-8 % of the pixels, a byte or an RNG stream on a
    few); no launch policy mixes it with the queued kernels, so it is counted
    and not pinned;
  * the brute-force loop against the BVH;
  * the BVH kernels' compiled leaf records (the simple BVH kernel) against the
    refill kernel's vertex-form records, whose planes the device forms itself,
    contracted.
The BVH schedules are therefore pinned per kernel: the refill kernel's
variants to the refill kernel's default schedule, the simple BVH kernel's node
formats and octant masks to its default.
"""
import os

import numpy as np
import pytest

import sky_cases as S
from bwrt import Renderer, scenes
from scenegen import _random_scene, _scaled

pytestmark = pytest.mark.gpu

MB = 2  # the sky matrix's bounce limit (test_gpu_sky.py)
PRODUCT = not os.environ.get("BWRT_LIB")  # kernel families pin the product library's policy only


def _fresh(bwrt_lib, env):
    """A FAST renderer created under BWRT_* launch knobs (read at rt_create)."""
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        r = Renderer(0, lib=bwrt_lib)
    finally:
        for k in env:
            del os.environ[k]
    r.set_precision("fast")
    return r


@pytest.fixture(scope="module")
def pool(bwrt_lib):
    """Contexts by their create-time knobs, made once per module."""
    made = {}

    def get(**env):
        key = tuple(sorted(env.items()))
        if key not in made:
            made[key] = _fresh(bwrt_lib, env)
        return made[key]

    yield get
    for r in made.values():
        r.close()


SIMPLE = dict(BWRT_KERNEL="simple")
REFERENCE = dict(BWRT_SPREAD=0, BWRT_BLOCK=64, BWRT_GREC=0, BWRT_SKY=0, BWRT_ORDER=0)
REFERENCE_KERNEL = "rt_render_sorted_kernel<64,fast>"
PAIR = dict(BWRT_SPREAD=1)
SORTED_LDS = dict(BWRT_SPREAD=0, BWRT_GREC=0)
SORTED_GREC = dict(BWRT_SPREAD=0, BWRT_GREC=1)


def set_scene(r, scene, **options):
    """rt_set_scene under scene-compile options (BWRT_BVH_*: read there)."""
    for k, v in options.items():
        os.environ[k] = str(v)
    try:
        r.set_scene(scene)
    finally:
        for k in options:
            del os.environ[k]


def step(r, w, h, frames, mb, first, off=0, stride=1):
    """One render call and the full state after it."""
    img = r.render(w, h, frames, mb, first_frame=first, row_offset=off, row_stride=stride)
    rng, acc = r.get_state(len(range(off, h, stride)), w)
    return img, rng, acc


def diff(a, b):
    """Names of the parts of two states that differ."""
    return [what for x, y, what in zip(a, b, ("RGBA8", "RNG state", "frameSum"))
            if not np.array_equal(x, y, equal_nan=what == "frameSum")]


def same(a, b, what=""):
    bad = diff(a, b)
    assert not bad, f"{what}: {bad} differ; {int((a[0] != b[0]).any(-1).sum())} of {a[0].shape[0] * a[0].shape[1]} pixels"


def kernel(r, family):
    name = r.last_kernel_name()
    assert ",fast" in name, name
    if PRODUCT:
        assert name.startswith(family), (name, family)
    return name


def two_steps(r, scene, w, h, frames, more, mb, off=0, stride=1, bg=None, family=None, **options):
    """`frames` frames from a fresh seed, then a continuation of `more`."""
    set_scene(r, scene, **options)
    r.set_background(*(bg or (0.0, 0.0, 0.0)))
    r.init_rand(w, h, off, stride)
    a = step(r, w, h, frames, mb, 1, off, stride)
    if family:
        kernel(r, family)
    b = step(r, w, h, more, mb, 0, off, stride)
    if family:
        kernel(r, family)
    return a, b


_REF = {}


def count(a, b):
    """(pixels whose RGBA8 differs, whose frameSum differs, whose RNG state differs, pixels)."""
    acc = ~((a[2] == b[2]) | (np.isnan(a[2]) & np.isnan(b[2])))
    return (int((a[0] != b[0]).any(-1).sum()), int(acc.any(-1).sum()), int((a[1] != b[1]).any(0).sum()),
            a[0].shape[0] * a[0].shape[1])


def reference(pool, key, scene, w, h, frames, more, mb, off=0, stride=1, bg=None):
    """The reference schedule's FAST state of a case, computed once and shared;
    the simple kernel's distance from it is printed (class A)."""
    if key not in _REF:
        r = pool(**REFERENCE)
        _REF[key] = two_steps(r, scene, w, h, frames, more, mb, off, stride, bg, REFERENCE_KERNEL)
        assert not PRODUCT or r.last_kernel_name() == REFERENCE_KERNEL, r.last_kernel_name()
        for part in _REF[key]:
            for x in part:
                x.setflags(write=False)
        simple = two_steps(pool(**SIMPLE), scene, w, h, frames, more, mb, off, stride, bg, "rt_render_kernel<")
        print(f"\nFASTINV class A {key}: simple kernel vs reference schedule: RGBA8 / frameSum / RNG differ on "
              f"%d / %d / %d of %d pixels" % count(simple[1], _REF[key][1]))
    return _REF[key]


# ---- 1. the sky path ---------------------------------------------------------------------------------
def sorted_env(block, grec, sky, tile_w=8, tile_sq=0):
    return dict(BWRT_SPREAD=0, BWRT_BLOCK=block, BWRT_GREC=grec, BWRT_ORDER=1, BWRT_ORDER_PERIOD=2, BWRT_SKY=sky,
                BWRT_TILE=tile_w, BWRT_TILE_SQ=tile_sq)


def check_sorted(r, block, sky, grec=None):
    name = kernel(r, f"rt_render_sorted_kernel<{block}")
    assert name.endswith("+sky") == bool(sky), name
    if grec is not None and PRODUCT:
        assert ("grec" in name) == bool(grec), name


@pytest.mark.parametrize("grec", [0, 1])
@pytest.mark.parametrize("block", [64, 128, 256])
def test_sky_cases_match_the_reference_schedule(bwrt_lib, pool, block, grec):
    """test_gpu_sky.py's matrix under FAST: the sky groups' one loop over the
    draws, with the table on (BWRT_SKY=2) and off, against the reference schedule."""
    for tile in sorted({(c[6], c[7]) for c in S.ORDINARY}):
        for sky in (2, 0):
            r = _fresh(bwrt_lib, sorted_env(block, grec, sky, *tile))
            try:
                for case in [c for c in S.ORDINARY if (c[6], c[7]) == tile]:
                    cid, make, w, h, off, stride, _, _ = case
                    first, more = reference(pool, ("sky", cid), make(), w, h, S.FRAMES, 3, MB, off, stride, S.BG)
                    r.set_scene(make())
                    r.set_background(*S.BG)
                    r.init_rand(w, h, off, stride)
                    same(step(r, w, h, S.FRAMES, MB, 1, off, stride), first, f"{cid} sky {sky}")
                    check_sorted(r, block, sky, grec)
                    same(step(r, w, h, 3, MB, 0, off, stride), more, f"{cid} sky {sky} continuation")
                    check_sorted(r, block, sky, grec)
            finally:
                r.close()


def test_view_changes_between_renders(bwrt_lib, pool):
    """test_gpu_sky.py's view-change sequence under the default policy
    (BWRT_SKY=1: a view's table arrives at its second launch)."""
    w, h = 160, 90
    r = _fresh(bwrt_lib, sorted_env(256, 0, 1))
    ref = pool(**REFERENCE)
    try:
        def both(frames, has_table, new_view=True):
            for x in (r, ref):
                x.init_rand(w, h)
            same(step(r, w, h, frames, MB, 1), step(ref, w, h, frames, MB, 1), "first launch of the view")
            assert kernel(r, "rt_render_sorted_kernel<256").endswith("+sky") == (has_table and not new_view)
            kernel(ref, REFERENCE_KERNEL)
            same(step(r, w, h, 2, MB, 0), step(ref, w, h, 2, MB, 0), "second launch of the view")
            assert kernel(r, "rt_render_sorted_kernel<256").endswith("+sky") == has_table

        for x in (r, ref):
            x.set_scene(scenes.scene_07())
            x.set_background(*S.BG)
        both(4, True)
        cam = r.get_camera()
        cam.angle[0], cam.angle[1] = 0.7, 0.25
        for x in (r, ref):
            x.set_camera(cam)
        both(4, True)
        for x in (r, ref):
            x.set_scene(S.with_camera(scenes.scene_04_box(), 1.3, 0.2))
        both(4, True)
        for x in (r, ref):
            x.set_background(0.9, 0.1, 0.4)
        both(4, True, new_view=False)
        for x in (r, ref):
            x.set_scene(S.with_camera(scenes.scene_07(), pos=(0.1, 0.75, -4.0)))
        both(2, False)
    finally:
        r.close()
        ref.set_background(0.0, 0.0, 0.0)


def test_full_frame_sky_and_order_arrive_mid_accumulation(bwrt_lib):
    """1920x1080, scene 07, three launches of one frame under the default
    policy: the first has neither a sky table nor a launch order, the later ones
    both; the accumulation must not depend on that history (BWRT_SKY=0)."""
    w, h, mb = 1920, 1080, 4
    r, plain = _fresh(bwrt_lib, {}), _fresh(bwrt_lib, dict(BWRT_SKY=0))
    try:
        for x in (r, plain):
            x.set_scene(scenes.scene_07())
            x.set_background(*S.BG)
            x.init_rand(w, h)
        for i in range(3):
            same(step(r, w, h, 1, mb, 0), step(plain, w, h, 1, mb, 0), f"launch {i + 1}")
            if PRODUCT:
                assert r.last_kernel_name() == "rt_render_sorted_kernel<256,grec,fast>+order" + ("+sky" if i else "")
                assert plain.last_kernel_name() == "rt_render_sorted_kernel<256,grec,fast>+order"
    finally:
        r.close()
        plain.close()


# ---- 2. kernel families -------------------------------------------------------------------------------
def _random_case(seed):
    s = _random_scene(seed)
    if seed % 4 == 2:
        s = _scaled(s, 1e3 if seed % 8 == 2 else 1e-3)
    return s, 80, 45, 3, [0, 1, 2, 4, 6, 9][seed % 6]


EXTREME = [(3, 1e6), (5, 1e10), (7, 1e-6), (9, 1e-10), (11, 1e15), (13, 1e19)]
FAMILY_CASES = {"07": lambda: (scenes.scene_07(), 160, 90, 3, 4), "04_box": lambda: (scenes.scene_04_box(), 160, 90, 3, 4)}
FAMILY_CASES.update({f"random{s}": (lambda s=s: _random_case(s)) for s in (0, 2, 4, 6)})
FAMILY_CASES.update({f"random{s}_x{k:g}": (lambda s=s, k=k: (_scaled(_random_scene(s), k), 64, 36, 2, 4)) for s, k in EXTREME})


def families(pool, mb):
    """(context, kernel family) of every brute-force family a launch can take;
    the pair kernel has no global records, which paths deeper than 4 take."""
    out = [(pool(**SORTED_LDS), "rt_render_sorted_kernel<"), (pool(**SORTED_GREC), "rt_render_sorted_kernel<")]
    if mb <= 4:
        out.append((pool(**PAIR), "rt_render_pair_kernel<"))
    return out


@pytest.mark.parametrize("case", list(FAMILY_CASES))
def test_kernel_families_agree(pool, case):
    """Pair, sorted with LDS records and sorted with global records: the
    launch policy mixes them inside one frame (row shards) and one
    accumulation."""
    scene, w, h, spp, mb = FAMILY_CASES[case]()
    ref = reference(pool, ("family", case), scene, w, h, spp, 2, mb)
    for r, fam in families(pool, mb):
        got = two_steps(r, scene, w, h, spp, 2, mb, family=fam)
        same(got[0], ref[0], f"{case} {r.last_kernel_name()}")
        same(got[1], ref[1], f"{case} {r.last_kernel_name()} continuation")


# ---- 3. record stack depth ----------------------------------------------------------------------------
@pytest.mark.parametrize("mb", [0, 1, 2, 3, 5, 12, 32])
@pytest.mark.parametrize("name,w,h", [("07", 160, 90), ("04_box", 96, 61)])
def test_record_stack_depths(pool, name, w, h, mb):
    """LDS against global records at every workgroup size and bounce limit (the
    global split keeps levels 0-1 in LDS: its boundaries are limits 2 and 3;
    from 16 on only 64-lane groups hold the stack), 3 frames then 2 more."""
    scene = {"07": scenes.scene_07, "04_box": scenes.scene_04_box}[name]()
    ref = reference(pool, ("depth", name, mb), scene, w, h, 3, 2, mb)
    for block in (64, 128, 256):
        for grec in (0, 1):
            r = pool(BWRT_SPREAD=0, BWRT_BLOCK=block, BWRT_GREC=grec)
            got = two_steps(r, scene, w, h, 3, 2, mb, family=f"rt_render_sorted_kernel<{64 if mb >= 16 else block}")
            if PRODUCT:
                assert ("grec" in r.last_kernel_name()) == bool(grec)
            same(got[0], ref[0], f"{name} limit {mb} {r.last_kernel_name()}")
            same(got[1], ref[1], f"{name} limit {mb} {r.last_kernel_name()} continuation")
    if mb <= 4:
        got = two_steps(pool(**PAIR), scene, w, h, 3, 2, mb, family="rt_render_pair_kernel<")
        same(got[0], ref[0], f"{name} limit {mb} pair")
        same(got[1], ref[1], f"{name} limit {mb} pair continuation")


# ---- 4. shapes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,off,stride", [(1, 1, 0, 1), (63, 65, 0, 1), (100, 37, 0, 1), (333, 187, 5, 8)])
def test_ragged_shapes(pool, w, h, off, stride):
    scene = scenes.scene_07()
    ref = reference(pool, ("shape", w, h), scene, w, h, 3, 2, 4, off, stride)
    for r, fam in families(pool, 4) + [(pool(), "rt_render_")]:
        got = two_steps(r, scene, w, h, 3, 2, 4, off, stride, family=fam)
        same(got[0], ref[0], f"{w}x{h} {r.last_kernel_name()}")
        same(got[1], ref[1], f"{w}x{h} {r.last_kernel_name()} continuation")


# ---- 5. row shards ------------------------------------------------------------------------------------
def test_row_shards_match_the_full_frame(pool):
    """A multi-GPU FAST frame is row shards, each from whatever kernel the
    policy gives its size, stitched together."""
    scene, w, h, spp, mb = scenes.scene_07(), 160, 90, 4, 4
    (img, rng, acc), _ = reference(pool, ("shards",), scene, w, h, spp, 1, mb)
    r = pool()
    r.set_scene(scene)
    r.set_background(0.0, 0.0, 0.0)
    names = set()
    for stride in (1, 2, 3, 8):
        for off in range(stride):
            r.init_rand(w, h, off, stride)
            got = step(r, w, h, spp, mb, 1, off, stride)
            names.add(kernel(r, "rt_render_"))
            same(got, (img[off::stride], rng[:, off::stride], acc[off::stride]), f"rows {off} mod {stride}")
    print(f"\nFASTINV shards: kernels {sorted(names)}")


# ---- 6. call splitting --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sky", "04_box"])
def test_call_splitting(pool, case):
    """8 frames as one call, as 1 + 7, as 3 + 5 and as 8 x 1 (the sky groups run
    one loop over the draws of all frames of a call)."""
    if case == "sky":
        scene, w, h, mb, bg = S.with_camera(scenes.scene_07(), 0.5, 0.3), 160, 90, MB, S.BG
        r, fam = pool(**sorted_env(256, 0, 2)), "rt_render_sorted_kernel<256"
    else:
        scene, w, h, mb, bg = scenes.scene_04_box(), 96, 61, 5, (0.0, 0.0, 0.0)
        r, fam = pool(), "rt_render_"
    want, _ = reference(pool, ("split", case), scene, w, h, 8, 1, mb, bg=bg)
    for split in ((8,), (1, 7), (3, 5), (1,) * 8):
        r.set_scene(scene)
        r.set_background(*bg)
        r.init_rand(w, h)
        for i, n in enumerate(split):
            got = step(r, w, h, n, mb, 1 if i == 0 else 0)
            name = kernel(r, fam)
        if case == "sky":
            assert name.endswith("+sky"), name
        same(got, want, f"{case} as {split}")
    r.set_background(0.0, 0.0, 0.0)


# ---- 7. samplesPerPixel > 1 ---------------------------------------------------------------------------
def test_samples_per_pixel_3(pool):
    """set_samples_per_pixel(3): the policy gives every such launch to the
    one-path-per-lane kernel, whichever queued kernel the context would take
    otherwise; the two contexts agree (block 256 and the small-frame shape)."""
    scene, w, h, mb = scenes.scene_07(), 96, 54, 4
    out = []
    for r in (pool(**SORTED_LDS), pool(**PAIR)):
        r.set_samples_per_pixel(3)
        try:
            out.append(two_steps(r, scene, w, h, 2, 1, mb, family="rt_render_kernel<"))
        finally:
            r.set_samples_per_pixel(1)
    same(out[0][0], out[1][0], "samplesPerPixel 3")
    same(out[0][1], out[1][1], "samplesPerPixel 3 continuation")


# ---- 8. BVH schedules and pruning ---------------------------------------------------------------------
REFILL = "rt_render_bvh_refill_kernel<64"
SIMPLE_BVH = "rt_render_kernel<"
STRESS = ("stress", 96, 54, 2, 8, 0, 1)
C5_ROWS = ("c5_rows", 1920, 1080, 2, 8, 3, 135)
NODE_OPTIONS = [{}, {"BWRT_BVH_N16": 0}, {"BWRT_BVH_ORDER_MASK": 7}, {"BWRT_BVH_N16": 0, "BWRT_BVH_ORDER_MASK": 7},
                {"BWRT_BVH_ORDER_MASK": 1}]


def bvh_state(r, scene, w, h, spp, mb, off, stride, family, **options):
    set_scene(r, scene, **options)
    r.set_background(0.0, 0.0, 0.0)
    r.init_rand(w, h, off, stride)
    got = step(r, w, h, spp, mb, 1, off, stride)
    name = kernel(r, family)
    if family == SIMPLE_BVH and PRODUCT:
        assert ",bvh" in name, name
    return got


@pytest.mark.parametrize("case", [STRESS, C5_ROWS], ids=lambda c: c[0])
def test_bvh_schedules_and_node_formats(pool, case):
    """What is pruned and when never changes what an accepted hit computes:
    the refill kernel under every (BWRT_LEAF_BATCH, BWRT_REFILL) pair, node
    format and octant mask equals its default schedule, and the simple BVH
    kernel under every node format and mask equals its default."""
    cid, w, h, spp, mb, off, stride = case
    scene = scenes.stress_scene()
    refill = bvh_state(pool(), scene, w, h, spp, mb, off, stride, REFILL)
    simple = bvh_state(pool(**SIMPLE), scene, w, h, spp, mb, off, stride, SIMPLE_BVH)
    for batch, ref in ((1, 1), (64, 64), (33, 1), (1, 64), (60, 36)):
        got = bvh_state(pool(BWRT_LEAF_BATCH=batch, BWRT_REFILL=ref), scene, w, h, spp, mb, off, stride, REFILL)
        same(got, refill, f"{cid} refill schedule ({batch}, {ref})")
    for opt in NODE_OPTIONS[1:]:
        same(bvh_state(pool(), scene, w, h, spp, mb, off, stride, REFILL, **opt), refill, f"{cid} refill {opt}")
        same(bvh_state(pool(**SIMPLE), scene, w, h, spp, mb, off, stride, SIMPLE_BVH, **opt), simple, f"{cid} simple {opt}")
    # class A, counted only: other arithmetic forms of the same scene
    brute = bvh_state(pool(), scene, w, h, spp, mb, off, stride, "rt_render_", BWRT_BVH_MIN=100000000)
    print(f"\nFASTINV class A {cid} (RGBA8, frameSum, RNG, pixels): compiled vs vertex-form leaf records "
          f"{count(simple, refill)}; brute force vs simple BVH {count(brute, simple)}, vs refill {count(brute, refill)}")


def _scaled_stress(k, mb):
    return lambda: (_scaled(scenes.stress_scene(), k), 96, 54, 2, mb)


BVH_SCENES = {f"stress_x{k:g}": _scaled_stress(k, mb)
              for k, mb in [(3e4, 6), (1e-4, 6), (1.0, 6), (100.0, 1), (1e3, 6), (1e10, 3)]}
BVH_SCENES.update({f"random{s}": (lambda s=s: _random_case(s)) for s in (1, 3, 5, 7)})
BVH_SCENES.update({f"random{s}_x{k:g}": (lambda s=s, k=k: (_scaled(_random_scene(s), k), 64, 36, 2, 4)) for s, k in EXTREME})


@pytest.mark.parametrize("case", list(BVH_SCENES))
def test_bvh_scenes_across_schedules(pool, case):
    """Scaled, random and extreme-scale scenes through the BVH (BWRT_BVH_MIN=1:
    the ones EXACT renders, for parity): the refill kernel lane by lane and with
    another octant mask equals its default schedule, the simple BVH kernel with
    another mask equals its default."""
    scene, w, h, spp, mb = BVH_SCENES[case]()
    refill = bvh_state(pool(), scene, w, h, spp, mb, 0, 1, REFILL, BWRT_BVH_MIN=1)
    simple = bvh_state(pool(**SIMPLE), scene, w, h, spp, mb, 0, 1, SIMPLE_BVH, BWRT_BVH_MIN=1)
    same(bvh_state(pool(BWRT_LEAF_BATCH=1, BWRT_REFILL=1), scene, w, h, spp, mb, 0, 1, REFILL, BWRT_BVH_MIN=1), refill,
         f"{case} refill schedule (1, 1)")
    same(bvh_state(pool(), scene, w, h, spp, mb, 0, 1, REFILL, BWRT_BVH_MIN=1, BWRT_BVH_ORDER_MASK=7), refill,
         f"{case} refill mask 7")
    same(bvh_state(pool(**SIMPLE), scene, w, h, spp, mb, 0, 1, SIMPLE_BVH, BWRT_BVH_MIN=1, BWRT_BVH_ORDER_MASK=7), simple,
         f"{case} simple mask 7")
    print(f"\nFASTINV class A {case} (RGBA8, frameSum, RNG, pixels): compiled vs vertex-form leaf records "
          f"{count(simple, refill)}")


def teardown_module(module):
    _REF.clear()
