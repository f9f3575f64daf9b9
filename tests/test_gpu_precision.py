"""RT_PRECISION_REFERENCE_FAST on the GPU (rt_set_precision; DESIGN.md "The
reference-fast precision mode"): every render kernel the launch policy can
pick, against the exact oracle at the same passes.

The bar is SURVEY.md section 8(c)'s, over the RGB bytes of ALL pixels: at
least 99.5 % of the pixels with max-channel |delta| <= 1 LSB, and a mean
|delta| of at most 0.25 LSB.  Each case prints its figures (and the share of
pixels whose RNG stream left the oracle's: informational, no bar) before it
asserts.
"""
import functools
import os

import numpy as np
import pytest

import sky_cases
from bwrt import Renderer, scenes
from scenegen import guard_scene

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

WITHIN_1LSB_MIN = 0.995
MEAN_ABS_MAX = 0.25

SCENES = {"07": scenes.scene_07, "04_box": scenes.scene_04_box, "stress": scenes.stress_scene,
          "07_yaw_pitch": lambda: sky_cases.with_camera(scenes.scene_07(), 0.5, 0.3),
          "guard": guard_scene}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def _oracle_state(name, w, h, spp, mb, off, stride, split=None, background=(0.0, 0.0, 0.0)):
    """The exact reference of a case, computed once and shared (read-only);
    `split`: the frames of each render call, the oracle continuing alongside."""
    import oracle as O
    O.build()
    st = O.OracleState(w, h, off, stride)
    for i, n in enumerate(split or (spp,)):
        O.render(_scene(name), st, n, mb, first_frame=1 if i == 0 else None, background=background)
    return st


def _fresh(bwrt_lib, monkeypatch, env):
    """A renderer created under BWRT_* launch knobs (read at rt_create)."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return Renderer(0, lib=bwrt_lib)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _stats(img, st):
    d = np.abs(img[..., :3].astype(np.int32) - st.rgba[..., :3].astype(np.int32))
    return float((d.max(-1) <= 1).mean()), float(d.mean())


# (id, scene, w, h, spp, bounces, row_offset, row_stride, knobs, kernel family the knobs / shape pin)
CASES = [
    # smallest frame whose policy choice is the pair kernel with a full chain
    ("pair_policy", "07", 320, 180, 8, 4, 0, 1, {}, "rt_render_pair_kernel<"),
    ("sorted_lds_records", "07", 320, 180, 8, 4, 0, 1, {"BWRT_SPREAD": 0}, "rt_render_sorted_kernel<"),
    # the headline's kernel shape
    ("sorted_global_records", "07", 320, 180, 8, 4, 0, 1, {"BWRT_SPREAD": 0, "BWRT_GREC": 1}, "rt_render_sorted_kernel<"),
    # partial groups, the seeding of a shard
    ("ragged_shard", "07", 333, 187, 4, 4, 5, 8, {}, None),
    # polygon_test with nv = 4
    ("quads", "04_box", 320, 180, 4, 5, 0, 1, {}, None),
    ("simple_kernel", "07", 160, 90, 8, 4, 0, 1, {"BWRT_KERNEL": "simple"}, "rt_render_kernel<"),
    ("bvh_refill", "stress", 96, 54, 2, 8, 0, 1, {}, "rt_render_bvh_refill_kernel<"),
    # the shape the mode is quoted on, switched on the way bench.py can: the create-time knob
    ("headline_frame", "07", 1920, 1080, 8, 4, 0, 1, {"BWRT_PRECISION": "fast"}, None),
    # the sorted kernel with a sky table and (where the policy gives one) a launch order, which a view's
    # first launch never has: 8 frames as 3 + 5 under a non-black background
    ("sky_order_second_launch", "07_yaw_pitch", 320, 180, 8, 4, 0, 1,
     {"BWRT_SPREAD": 0, "BWRT_SKY": 1, "BWRT_ORDER_PERIOD": 2}, "rt_render_sorted_kernel<"),
    # the box's shared edges (exact ties in EXACT) through the BVH
    ("bvh_forced_box", "04_box", 320, 180, 4, 5, 0, 1, {}, "rt_render_bvh_refill_kernel<"),
    # the scene on which the isnan(g) guard decides half the pixels (scenegen.guard_scene): the fast
    # twins must keep the guard, so no pixel of the frame may be non-finite: the policy's kernel, the
    # sorted kernel with global records, the simple kernel and the BVH refill kernel
    ("isnan_guard", "guard", 160, 90, 3, 4, 0, 1, {}, None),
    ("isnan_guard_sorted", "guard", 160, 90, 3, 4, 0, 1, {"BWRT_SPREAD": 0, "BWRT_GREC": 1}, "rt_render_sorted_kernel<"),
    ("isnan_guard_simple", "guard", 160, 90, 3, 4, 0, 1, {"BWRT_KERNEL": "simple"}, "rt_render_kernel<"),
    ("isnan_guard_bvh", "guard", 160, 90, 3, 4, 0, 1, {}, "rt_render_bvh_refill_kernel<"),
]
# what a case needs beyond its launch knobs: the frames of each render call, the background, the
# scene-compile options (read at rt_set_scene) and the end of the last launch's kernel name
EXTRA = {
    "sky_order_second_launch": {"split": (3, 5), "background": sky_cases.BG, "ends": "+sky"},
    "bvh_forced_box": {"scene_env": {"BWRT_BVH_MIN": 1}},
    "isnan_guard": {"finite": True},
    "isnan_guard_sorted": {"finite": True},
    "isnan_guard_simple": {"finite": True},
    "isnan_guard_bvh": {"finite": True, "scene_env": {"BWRT_BVH_MIN": 1}},
}


@pytest.mark.parametrize("cid,name,w,h,spp,mb,off,stride,env,family", CASES, ids=[c[0] for c in CASES])
def test_fast_within_tolerance(bwrt_lib, monkeypatch, cid, name, w, h, spp, mb, off, stride, env, family):
    extra = EXTRA.get(cid, {})
    split, background = extra.get("split"), extra.get("background", (0.0, 0.0, 0.0))
    assert sum(split or (spp,)) == spp
    st = _oracle_state(name, w, h, spp, mb, off, stride, split, background)
    r = _fresh(bwrt_lib, monkeypatch, env)
    try:
        if "BWRT_PRECISION" not in env:
            assert r.precision == "exact"
            r.set_precision("fast")
        assert r.precision == "fast"
        for k, v in extra.get("scene_env", {}).items():
            monkeypatch.setenv(k, str(v))
        r.set_scene(_scene(name))
        for k in extra.get("scene_env", {}):
            monkeypatch.delenv(k)
        r.set_background(*background)
        r.init_rand(w, h, off, stride)
        for i, n in enumerate(split or (spp,)):
            img = r.render(w, h, n, mb, first_frame=1 if i == 0 else 0, row_offset=off, row_stride=stride)
        kernel = r.last_kernel_name()
        rng, acc = r.get_state(st.rows, st.width)
    finally:
        r.close()
    assert img.shape == st.rgba.shape
    if extra.get("finite"):
        bad = int((~np.isfinite(acc)).any(-1).sum())
        print(f"\nFASTSTAT {cid}: non-finite pixels {bad} (exact oracle: {int((~np.isfinite(st.accum)).any(-1).sum())})")
        assert bad == 0, bad
    within, mean = _stats(img, st)
    desync = float((rng != st.rng).any(0).mean())
    print(f"\nFASTSTAT {cid}: kernel {kernel} within_1lsb {within * 100:.4f} % mean_abs {mean:.5f} LSB "
          f"rng_desync {desync * 100:.4f} % of {img.shape[0] * img.shape[1]} pixels")
    assert ",fast" in kernel, kernel
    if family and not os.environ.get("BWRT_LIB"):
        assert kernel.startswith(family), kernel
        assert ("grec" in kernel) == (env.get("BWRT_GREC") == 1), kernel
        assert kernel.endswith(extra.get("ends", "")), kernel
    assert (img[..., 3] == 255).all()
    assert within >= WITHIN_1LSB_MIN, (within, mean)
    assert mean <= MEAN_ABS_MAX, (within, mean)


def test_fast_mode_is_real(bwrt_lib, monkeypatch):
    """FAST's frameSum is not bit-identical to EXACT's from the same seeds
    (contraction alone changes the accumulators of most pixels)."""
    _, name, w, h, spp, mb, off, stride, env, _ = CASES[0]
    r = _fresh(bwrt_lib, monkeypatch, env)
    try:
        r.set_scene(_scene(name))
        r.init_rand(w, h)
        _, acc_exact = r.render(w, h, spp, mb, first_frame=1, want_accum=True)
        assert ",fast" not in r.last_kernel_name()
        r.set_precision("fast")
        r.init_rand(w, h)
        _, acc_fast = r.render(w, h, spp, mb, first_frame=1, want_accum=True)
        assert ",fast" in r.last_kernel_name()
    finally:
        r.close()
    assert np.array_equal(acc_exact, _oracle_state(name, w, h, spp, mb, off, stride).accum, equal_nan=True)
    changed = float((acc_fast != acc_exact).any(-1).mean())
    print(f"\nFASTSTAT mode_is_real: frameSum differs on {changed * 100:.2f} % of the pixels")
    assert changed > 0.0


def test_switching_back_leaves_no_residue(bwrt_lib, monkeypatch):
    """FAST, then EXACT on the same context: RGBA, frameSum and RNG are
    bit-exact with the oracle again, through an exact kernel."""
    w, h, spp, mb = 320, 180, 4, 4
    st = _oracle_state("07", w, h, spp, mb, 0, 1)
    r = _fresh(bwrt_lib, monkeypatch, {})
    try:
        r.set_scene(_scene("07"))
        r.set_precision("fast")
        r.init_rand(w, h)
        r.render(w, h, spp, mb, first_frame=1)
        assert ",fast" in r.last_kernel_name()
        frame = r.frame_counter
        r.set_precision("exact")
        assert r.frame_counter == frame  # the switch itself resets nothing
        r.init_rand(w, h)
        img, acc = r.render(w, h, spp, mb, first_frame=1, want_accum=True)
        assert "fast" not in r.last_kernel_name(), r.last_kernel_name()
        rng, acc_state = r.get_state(h, w)
    finally:
        r.close()
    assert np.array_equal(img, st.rgba)
    assert np.array_equal(acc, st.accum, equal_nan=True)
    assert np.array_equal(acc_state, st.accum, equal_nan=True)
    assert np.array_equal(rng, st.rng)


def test_fast_converges_to_reference_png(bwrt_lib, monkeypatch):
    """Real-CUDA pin under FAST (test_gpu_parity.test_converges_to_reference_png's
    procedure): 2 x 512 frames of the 07 scene at 1920x1080, maxBounces 5, vs
    Renders/07_specular_BRDF.png: 16x16 block-mean MAE <= 1.5 LSB."""
    g = np.load(os.path.join(GOLDEN, "07_png_blocks16.npz"))
    r = _fresh(bwrt_lib, monkeypatch, {})
    try:
        r.set_precision("fast")
        r.set_scene(_scene("07"))
        r.init_rand(1920, 1080)
        r.render(1920, 1080, 512, 5, first_frame=1)
        img = r.render(1920, 1080, 512, 5)
        assert ",fast" in r.last_kernel_name()
    finally:
        r.close()
    top = img[::-1, :, :3]
    dx, dy, ph, pw, b = (int(g[k]) for k in ("dx", "dy", "png_h", "png_w", "block"))
    crop = top[dy:dy + ph, dx:dx + pw]
    hh, ww = ph // b * b, pw // b * b
    blocks = crop[:hh, :ww].astype(np.float64).reshape(hh // b, b, ww // b, b, 3).mean((1, 3))
    mae = np.abs(blocks - g["blocks"]).mean()
    print(f"\nFASTSTAT png_pin: block-mean MAE {mae:.4f} LSB")
    assert mae <= 1.5, mae
