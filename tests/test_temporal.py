"""Temporal reprojection of the accumulated radiance across camera moves
(rt_temporal) on the CPU backend — no GPU needed.  The GPU kernel computes the
same bits (tests/test_gpu_temporal.py compares it with this backend).

The float64 reference is tests/temporal_ref.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import temporal_ref as T
from bwrt import Renderer, abi, scenes
from bwrt.abi import Camera
from test_denoise import FILTER_BOUND

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwidman-raytracer_amd", "bin",
                   "bwrt_render")

# max |colour - float64 reference| / (1 + |reference|) over the unmarked pixels,
# measured on the CPU backend over the cases of test_against_float64 (3 frames
# per view, 4 bounces, moves A -> B -> C), per scene: float32 rounding of the
# hit points, of the history camera's rotation and of the projection moves the
# bilinear weights by ~1e-5 of a pixel, times the difference between
# neighbouring pixels of a 3-frame history (the 04_box frame has its emitter in
# view: a wider range than scene 07's).  Asserted at 8x: room for another
# compiler's float64 libm, while one wrong tap moves a pixel by ~1e-1.
MEASURED = {"07": 1.97e-5, "04_box": 1.73e-4}
LENGTH_BOUND = 1e-5  # relative
MARKED_CAP = 0.02    # of the pixels of each case: a condition on the moves


def cam(px, py, pz, yaw, pitch, fov):
    return Camera(scenes.vec(px, py, pz), (C.c_float * 2)(yaw, pitch), fov)


def moved(c, dx=0.0, dy=0.0, dz=0.0, dyaw=0.0, dpitch=0.0):
    return cam(c.position.x + dx, c.position.y + dy, c.position.z + dz, c.angle[0] + dyaw, c.angle[1] + dpitch,
               c.fov)


# View A is off the scene camera's axes, and no move leaves a screen coordinate
# on the pixel grid (a pure yaw keeps the centre row, a pure x translation every
# row: the reference would mark them all as within rounding of floor's step).
VIEW_A = dict(dx=0.1, dy=0.2, dz=0.3, dyaw=0.05, dpitch=-0.08)
MOVES = {
    "yaw": dict(dyaw=0.037, dpitch=0.011),
    "sideways": dict(dx=0.5, dy=0.07),  # uncovers the floor and the sky behind the pyramid and the spheres
    "dolly": dict(dz=-0.4, dx=0.03),
}
SECOND = dict(dx=-0.2, dy=0.05, dz=-0.1, dyaw=-0.02, dpitch=0.013)
FRAMES, BOUNCES = 3, 4


def view_a(scene):
    return moved(scene.camera, **VIEW_A)


@pytest.fixture(scope="module")
def cpu(bwrt_lib):
    r = Renderer.cpu(0, lib=bwrt_lib)
    yield r
    r.close()


def view(r, camera, w, h, frames=FRAMES, denoise=None, **tp):
    """One view: set the camera (a new view), render `frames`, one temporal
    call.  Returns a dict of everything the reference needs."""
    r.set_camera(camera)
    img, acc = r.render(w, h, frames, BOUNCES, want_accum=True)
    rgba, col, ln = r.temporal(w, h, denoise=denoise, want_color=True, want_length=True, **tp)
    return {"camera": T.camera_copy(camera), "img": img, "acc": acc, "n": frames, "rgba": rgba, "color": col,
            "length": ln}


def reference(r, w, h, cur, hist, **tp):
    """temporal_ref for the view `cur` (the context's current one)."""
    t = r.temporal_params(**tp)
    aov = r.render_aov(w, h)
    ref = T.temporal_ref(cur["acc"], cur["n"], cur["camera"], aov, hist, t.max_history, t.normal_cos_min,
                         t.plane_tol)
    return aov, ref


def assert_no_history(v):
    inv = np.float32(1) / np.float32(v["n"])
    assert np.array_equal(v["color"], inv * v["acc"], equal_nan=True)
    assert np.all(v["length"] == v["n"])
    assert np.array_equal(v["rgba"], v["img"])


def test_abi_declares_the_entry_points(bwrt_lib):
    assert {"rt_temporal", "rt_temporal_device", "rt_temporal_reset", "rt_temporal_params_default",
            "rt_last_temporal_ms"} <= set(abi.declared_functions())
    t = bwrt_lib.rt_temporal_params_default()
    assert t.max_history > 0 and -1 <= t.normal_cos_min <= 1 and t.plane_tol > 0


# ---- 1. no history ------------------------------------------------------------
@pytest.mark.parametrize("name,w,h", [("07", 67, 45), ("07", 333, 187), ("04_box", 64, 36), ("stress", 96, 54)])
def test_no_history(bwrt_lib, name, w, h):
    scene = scenes.SCENES[name]()
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        assert r.last_temporal_ms() == -1.0
        r.set_scene(scene)
        a = view_a(scene)
        assert_no_history(view(r, a, w, h, 2))
        assert r.last_temporal_ms() >= 0.0
        b = view(r, moved(a, **MOVES["dolly"]), w, h, 2)
        assert (b["length"] > 2).any()  # a history now
        r.temporal_reset()
        assert_no_history(view(r, a, w, h, 2))
        view(r, moved(a, **MOVES["dolly"]), w, h, 2)
        r.set_scene(scene)  # primitive ids change meaning
        assert_no_history(view(r, a, w, h, 2))
        view(r, moved(a, **MOVES["dolly"]), w, h, 2)
        assert_no_history(view(r, a, w + 1, h, 2))  # another frame shape
        view(r, moved(a, **MOVES["dolly"]), w + 1, h, 2)
        r.render(w, h, 1, BOUNCES)  # a shape change and back with no temporal call in between
        assert_no_history(view(r, a, w + 1, h, 2))


# ---- 2. the float64 reference ---------------------------------------------------
@pytest.mark.parametrize("name,w,h,move", [("07", 67, 45, "yaw"), ("07", 67, 45, "sideways"), ("07", 67, 45, "dolly"),
                                           ("04_box", 64, 36, "sideways")])
def test_against_float64(cpu, name, w, h, move):
    scene = scenes.SCENES[name]()
    cpu.set_scene(scene)
    ca = view_a(scene)
    va = view(cpu, ca, w, h)
    hist = T.history(ca, w, h, cpu.render_aov(w, h), va["color"], va["length"])
    cur = ca
    for step, kw in (("A->B", MOVES[move]), ("B->C", SECOND)):
        cur = moved(cur, **kw)
        v = view(cpu, cur, w, h)
        aov, ref = reference(cpu, w, h, v, hist)
        keep = ~ref["marked"]
        err = T.rel_err(v["color"], ref["color"], keep)
        lerr = float(np.max(np.abs(v["length"][keep] - ref["length"][keep]) / ref["length"][keep]))
        print(f"{name} {move} {step}: marked {ref['marked'].mean():.4f}, max |d| / (1 + |ref|) = {err:.3e}, "
              f"length {lerr:.2e}, reprojected {ref['reprojected'].mean():.3f}")
        assert ref["marked"].mean() <= MARKED_CAP
        assert ref["reprojected"].mean() > 0.5
        assert lerr <= LENGTH_BOUND
        assert err <= 8 * MEASURED[name]
        if step == "B->C":  # the history carried reprojected lengths
            assert v["length"].max() > 2 * FRAMES
        hist = T.history(cur, w, h, aov, v["color"], v["length"])


# ---- 3. disocclusion and off-screen ---------------------------------------------
def test_turning_around_leaves_nothing_to_reproject(cpu):
    scene = scenes.scene_07()
    cpu.set_scene(scene)
    w, h = 67, 45
    a = view_a(scene)
    view(cpu, a, w, h)
    assert_no_history(view(cpu, moved(a, dyaw=float(np.pi)), w, h))


def test_disoccluded_pixels_start_over(cpu):
    scene = scenes.scene_07()
    cpu.set_scene(scene)
    w, h = 67, 45
    ca = view_a(scene)
    va = view(cpu, ca, w, h)
    hist = T.history(ca, w, h, cpu.render_aov(w, h), va["color"], va["length"])
    v = view(cpu, moved(ca, **MOVES["sideways"]), w, h)
    aov, ref = reference(cpu, w, h, v, hist)
    uncovered = (aov["prim"] >= 0) & (ref["same"] == 0) & ~ref["marked"]
    assert uncovered.sum() >= 20
    assert np.all(v["length"][uncovered] == FRAMES)
    assert np.array_equal(v["color"][uncovered], (np.float32(1) / np.float32(FRAMES)) * v["acc"][uncovered])
    assert np.all(v["length"][aov["prim"] < 0] == FRAMES)  # misses are never reprojected


# ---- 4. accumulation, 5. max_history --------------------------------------------
def test_lengths_add_up_in_an_unmoved_view(cpu):
    scene = scenes.scene_07()
    cpu.set_scene(scene)
    w, h = 67, 45
    ca = view_a(scene)
    n1, n2, n3 = 2, 3, 2
    va = view(cpu, ca, w, h, n1, max_history=8.0)
    hist = T.history(ca, w, h, cpu.render_aov(w, h), va["color"], va["length"])
    vb = view(cpu, ca, w, h, n2, max_history=8.0)  # the same camera: accumulation restarts, a new view
    assert cpu.frame_counter == n2 + 1
    aov, ref = reference(cpu, w, h, vb, hist, max_history=8.0)
    full = ref["taps"] == 4
    full[[0, -1], :] = full[:, [0, -1]] = False
    assert full.mean() > 0.4
    assert np.max(np.abs(vb["length"][full] - (n1 + n2))) <= 1e-3
    vc = view(cpu, ca, w, h, n3, max_history=8.0)
    assert np.max(np.abs(vc["length"][full] - (n1 + n2 + n3))) <= 1e-3


def test_max_history_caps_the_length(cpu):
    scene = scenes.scene_07()
    cpu.set_scene(scene)
    w, h = 67, 45
    ca = view_a(scene)
    view(cpu, ca, w, h, 4, max_history=2.0)
    cur = ca
    for kw in (MOVES["yaw"], SECOND):
        cur = moved(cur, **kw)
        v = view(cpu, cur, w, h, 3, max_history=2.0)
        assert v["length"].max() == 2.0 + 3
        assert v["length"].min() == 3.0


# ---- 6. special values -------------------------------------------------------------
def plant(r, w, h, frames, pixels, values):
    rng, acc = r.get_state(h, w)
    for p, v in zip(pixels, values):
        acc[p] = v
    r.set_state(rng, acc, frames + 1)
    return acc


def special_sequence(r, w, h, history_values, current_values):
    """View A with non-finite frameSum pixels (the history), a yaw, view B with
    others.  Returns (history, view B's dict, the two pixel lists)."""
    scene = scenes.scene_07()
    r.set_scene(scene)
    r.init_rand(w, h)  # the same samples in every sequence
    ca = view_a(scene)
    cb = moved(ca, **MOVES["yaw"])
    r.set_camera(ca)
    r.render(w, h, FRAMES, BOUNCES)
    aov_a = r.render_aov(w, h)
    hit = np.argwhere((aov_a["prim"][3:-3, 3:-3] >= 0)) + 3
    hist_px = [tuple(hit[len(hit) // 4]), tuple(hit[len(hit) // 2]), tuple(hit[3 * len(hit) // 4])]
    acc_a = plant(r, w, h, FRAMES, hist_px, history_values)
    _, col, ln = r.temporal(w, h, want_color=True, want_length=True)
    for p in hist_px:  # a non-finite pixel passes through unchanged
        assert np.array_equal(col[p], (np.float32(1) / np.float32(FRAMES)) * acc_a[p], equal_nan=True)
    hist = T.history(ca, w, h, aov_a, col, ln)
    r.set_camera(cb)
    r.render(w, h, FRAMES, BOUNCES)
    aov_b = r.render_aov(w, h)
    hit = np.argwhere((aov_b["prim"][3:-3, 3:-3] >= 0)) + 3
    cur_px = [tuple(hit[len(hit) // 3]), tuple(hit[2 * len(hit) // 3]), tuple(hit[len(hit) // 5])]
    acc_b = plant(r, w, h, FRAMES, cur_px, current_values)
    rgba, col, ln = r.temporal(w, h, want_color=True, want_length=True)
    vb = {"camera": cb, "acc": acc_b, "n": FRAMES, "rgba": rgba, "color": col, "length": ln}
    return hist, vb, hist_px, cur_px


def test_special_values(cpu):
    w, h = 67, 45
    nan, inf = np.nan, np.inf
    hist, vb, hist_px, cur_px = special_sequence(cpu, w, h, (nan, inf, -inf), (inf, -inf, nan))
    aov, ref = reference(cpu, w, h, vb, hist)
    inv = np.float32(1) / np.float32(FRAMES)
    for p in cur_px:  # planted in the current frame: unchanged, no history
        assert np.array_equal(vb["color"][p], inv * vb["acc"][p], equal_nan=True)
        assert vb["length"][p] == FRAMES
    others = np.ones((h, w), bool)
    for p in cur_px:
        others[p] = False
    assert np.isfinite(vb["color"][others]).all() and np.isfinite(vb["length"]).all()
    # the history's bad pixels are invalid taps (rule 5), nothing else: the reference drops them ...
    assert T.rel_err(vb["color"], ref["color"], ~ref["marked"]) <= 8 * MEASURED["07"]
    clean = dict(hist, color=np.where(np.isfinite(hist["color"]), hist["color"], 0.0))
    _, ref_clean = reference(cpu, w, h, vb, clean)
    assert (ref_clean["taps"] > ref["taps"]).sum() >= 3  # pixels that did lose such a tap
    # ... and which non-finite value they hold makes no difference to any other pixel
    hist2, vb2, hist_px2, cur_px2 = special_sequence(cpu, w, h, (-inf, nan, inf), (inf, -inf, nan))
    assert hist_px2 == hist_px and cur_px2 == cur_px
    assert np.array_equal(vb2["color"], vb["color"], equal_nan=True)
    assert np.array_equal(vb2["length"], vb["length"]) and np.array_equal(vb2["rgba"], vb["rgba"])


# ---- 7. state neutrality -------------------------------------------------------------
def test_state_is_untouched(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 64, 36
    out = []
    for with_temporal in (True, False):
        with Renderer.cpu(0, lib=bwrt_lib) as r:
            r.set_scene(scene)
            t = (lambda: r.temporal(w, h)) if with_temporal else (lambda: None)
            r.render(w, h, 2, BOUNCES, first_frame=1)
            t()
            r.render(w, h, 1, BOUNCES)
            r.set_camera(moved(scene.camera, **MOVES["yaw"]))
            r.render(w, h, 2, BOUNCES)
            t()
            t()
            img = r.render(w, h, 1, BOUNCES)
            out.append((img, r.frame_counter) + r.get_state(h, w))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] == 4
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3], equal_nan=True)


def test_repeated_calls_and_pending(bwrt_lib):
    """Two calls in one view give the same bits; a call in the same view after
    more frames replaces the pending result and leaves the history alone: the
    third view sees the same history either way."""
    scene = scenes.scene_07()
    w, h = 67, 45
    ca = view_a(scene)
    cb, cc = moved(ca, **MOVES["yaw"]), moved(ca, **MOVES["dolly"])
    res = []
    for split in (True, False):
        with Renderer.cpu(0, lib=bwrt_lib) as r:
            r.set_scene(scene)
            view(r, ca, w, h, 2)
            r.set_camera(cb)
            if split:
                r.render(w, h, 2, BOUNCES)
                t1 = r.temporal(w, h, want_color=True, want_length=True)
                t1b = r.temporal(w, h, want_color=True, want_length=True)
                assert all(np.array_equal(x, y) for x, y in zip(t1, t1b))
                r.render(w, h, 2, BOUNCES)
            else:
                r.render(w, h, 4, BOUNCES)
            t2 = r.temporal(w, h, want_color=True, want_length=True)
            if split:
                assert not np.array_equal(t1[1], t2[1])
                assert t2[2].max() == 2 + 4  # view A's 2 frames plus this view's 4, not t1's 4 on top
            vc = view(r, cc, w, h, 2)
            res.append((t2, vc))
    for x, y in zip(res[0][0], res[1][0]):
        assert np.array_equal(x, y)
    for k in ("rgba", "color", "length"):
        assert np.array_equal(res[0][1][k], res[1][1][k]), k
    assert res[0][1]["length"].max() > 2 + 4  # view C reprojects view B's pending result


# ---- 8. with the spatial filter ----------------------------------------------------------
def test_filter_runs_over_the_temporal_colour(cpu):
    scene = scenes.scene_07()
    cpu.set_scene(scene)
    w, h = 67, 45
    ca = view_a(scene)
    view(cpu, ca, w, h)
    cb = moved(ca, **MOVES["yaw"])
    plain = view(cpu, cb, w, h)
    assert (plain["length"] > FRAMES).any()
    zero = cpu.temporal(w, h, denoise={"iterations": 0}, want_color=True, want_length=True)
    assert np.array_equal(zero[0], plain["rgba"]) and np.array_equal(zero[1], plain["color"])
    assert np.array_equal(zero[2], plain["length"])
    aov = cpu.render_aov(w, h)
    P = R.hit_points(cb, w, h, aov["depth"], aov["prim"])
    for it in (1, 5):
        rgba, col, ln = cpu.temporal(w, h, denoise={"iterations": it}, want_color=True, want_length=True)
        d = cpu.denoise_params(iterations=it)
        ref = R.denoise_ref(plain["color"], 1, aov["normal"], P, aov["prim"], it, d.sigma_color, d.sigma_normal,
                            d.sigma_plane)
        assert R.rel_err(col, ref) <= FILTER_BOUND
        assert int(np.abs(rgba.astype(np.int32) - R.tone_map(ref).astype(np.int32)).max()) <= 1
        assert np.array_equal(ln, plain["length"])  # the stored history is the unfiltered one
        assert not np.array_equal(col, plain["color"])
    # ... so a third view reprojects the unfiltered colour of the (filtered) last call
    hist = T.history(cb, w, h, aov, plain["color"], plain["length"])
    vc = view(cpu, moved(cb, **SECOND), w, h)
    _, ref = reference(cpu, w, h, vc, hist)
    assert T.rel_err(vc["color"], ref["color"], ~ref["marked"]) <= 8 * MEASURED["07"]


# ---- 9. errors -------------------------------------------------------------------------------
def test_errors(bwrt_lib):
    lib = bwrt_lib
    with Renderer.cpu(1, lib=lib) as r:
        t = lib.rt_temporal_params_default()
        d = lib.rt_denoise_params_default()
        call = lambda p, dn=None: lib.rt_temporal(r.ctx, C.byref(p), dn, None, None, None)  # noqa: E731
        assert lib.rt_temporal(r.ctx, None, None, None, None, None) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(t) == abi.RT_ERR_NO_SCENE
        r.set_scene(scenes.scene_07())
        assert call(t) == abi.RT_ERR_INVALID_ARGUMENT  # nothing accumulated (frame counter 1)
        assert b"no frame" in lib.rt_last_error(r.ctx)
        r.render(16, 9, 1, 2, first_frame=1)
        assert call(t) == abi.RT_OK
        assert call(t, C.byref(d)) == abi.RT_OK
        nan = float("nan")
        for field, value in (("max_history", 0.0), ("max_history", -1.0), ("max_history", nan),
                             ("plane_tol", 0.0), ("plane_tol", -0.5), ("plane_tol", nan),
                             ("normal_cos_min", 1.5), ("normal_cos_min", -1.5), ("normal_cos_min", nan)):
            bad = lib.rt_temporal_params_default()
            setattr(bad, field, value)
            assert call(bad) == abi.RT_ERR_INVALID_ARGUMENT, (field, value)
        for field, value in (("iterations", -1), ("iterations", abi.RT_DENOISE_MAX_ITERATIONS + 1),
                             ("sigma_color", 0.0), ("sigma_plane", nan)):
            bad = lib.rt_denoise_params_default()
            setattr(bad, field, value)
            assert call(t, C.byref(bad)) == abi.RT_ERR_INVALID_ARGUMENT, (field, value)
        for field, value in (("normal_cos_min", -1.0), ("normal_cos_min", 1.0), ("max_history", float("inf"))):
            ok = lib.rt_temporal_params_default()
            setattr(ok, field, value)
            assert call(ok) == abi.RT_OK, (field, value)
        assert lib.rt_temporal_device(r.ctx, C.byref(t), None, None, None) == abi.RT_ERR_UNSUPPORTED  # CPU context
        r.reset_accumulation()
        assert call(t) == abi.RT_ERR_INVALID_ARGUMENT
        r.render(16, 9, 1, 2, first_frame=1, row_offset=1, row_stride=2)  # the state is now a row shard
        assert call(t) == abi.RT_ERR_UNSUPPORTED
        assert lib.rt_temporal_reset(r.ctx) == abi.RT_OK
    assert lib.rt_temporal_reset(None) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_last_temporal_ms(None) == -1.0


# ---- 10. quality -------------------------------------------------------------------------------
def test_quality_of_the_defaults(bwrt_lib):
    """The condition for shipping the defaults (tools/temporal_sweep.py's case):
    scene 07, 160x90, 4 frames at view A, a small move, 4 frames at view B;
    against a 1024-frame render of view B the temporal frame beats the raw one,
    and temporal + denoise beats denoise alone."""
    w, h = 160, 90
    scene = scenes.scene_07()
    ca = view_a(scene)
    cb = moved(ca, **MOVES["yaw"])
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_scene(scene)
        r.set_camera(cb)
        truth = r.render(w, h, 1024, BOUNCES, first_frame=1).astype(np.int32)
    with Renderer.cpu(0, lib=bwrt_lib) as r:  # fresh RNG streams, as the sweep
        r.set_scene(scene)
        view(r, ca, w, h, 4)
        r.set_camera(cb)
        raw = r.render(w, h, 4, BOUNCES)
        tem = r.temporal(w, h)
        den = r.denoise(w, h)
        both = r.temporal(w, h, denoise={})
    e = {k: np.abs(v[..., :3] - truth[..., :3]).mean() for k, v in
         (("raw", raw), ("temporal", tem), ("denoise", den), ("temporal+denoise", both))}
    print(", ".join(f"{k} {v:.3f}" for k, v in e.items()),
          f"; temporal / raw {e['temporal'] / e['raw']:.3f}, both / denoise {e['temporal+denoise'] / e['denoise']:.3f}")
    assert e["temporal"] < e["raw"]
    assert e["temporal+denoise"] < e["denoise"]


# ---- 11. the CLI ----------------------------------------------------------------------------------
def read_ppm(path, w, h):
    data = path.read_bytes()
    return np.frombuffer(data[len(data) - w * h * 3:], np.uint8).reshape(h, w, 3)


@pytest.mark.parametrize("denoise", [False, True])
def test_cli_equals_the_python_path(bwrt_lib, tmp_path, denoise):
    w, h, frames, mb, dt = 64, 36, 7, 3, 0.02
    keys = [["LEFT"], ["LEFT"], [], [], ["W", "RIGHT"], [], []]
    out = tmp_path / "t.ppm"
    cmd = [CLI, "--cpu", "2", "--width", str(w), "--height", str(h), "--frames", str(frames), "--max-bounces",
           str(mb), "--temporal", "--keys", "LEFT*2,*2,W+RIGHT*1,*2", "--dt", str(dt), "--max-history", "16",
           "--out", str(out)] + (["--denoise", "3"] if denoise else [])
    res = subprocess.run(cmd, check=True, capture_output=True, text=True)
    assert "temporal:" in res.stdout and ("denoise: 3 levels" in res.stdout) == denoise
    with Renderer.cpu(2, lib=bwrt_lib) as r:
        r.set_scene(scenes.scene_07())
        r.set_max_bounces(mb)
        for i, k in enumerate(keys):
            raw = r.render_simple(w, h, 1)
            last = i == frames - 1
            rgba = r.temporal(w, h, max_history=16.0, denoise={"iterations": 3} if denoise and last else None)
            r.controls(k, dt)
    assert np.array_equal(read_ppm(out, w, h), rgba[::-1, :, :3])  # the file's first row is the top
    assert not np.array_equal(rgba, raw)
