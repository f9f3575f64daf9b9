"""Temporal reprojection of the luminance moments across camera moves
(rt_temporal_var) on the CPU backend — no GPU needed.  The
GPU kernels compute the same bits (tests/test_gpu_temporal_var.py compares them
with this backend).

The float64 reference is tests/temporal_var_ref.py.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import assemble_case as A
import denoise_ref as R
import denoise_var_ref as V
import temporal_ref as T
import temporal_var_ref as TV
from bwrt import Renderer, abi, scenes
from test_denoise_var import SKY, dim_scene
from test_temporal import BOUNCES, CLI, MARKED_CAP, MOVES, SECOND, moved, plant, read_ppm, view_a

# the camera path of tools/temporal_sweep.py's and tools/temporal_var_sweep.py's walk
WALK = [MOVES["yaw"], dict(dx=0.15, dy=0.02), dict(dz=-0.15, dx=0.01), MOVES["yaw"], dict(dx=-0.1, dyaw=-0.03),
        dict(dz=-0.1), dict(dyaw=0.025, dpitch=-0.01)]

# test_moments_against_float64: max |value - float64 reference| / (eps + |reference|) over the unmarked pixels,
# eps the median of the reference over the pixels with dof > 0; (s2, variance of the mean) per scene, the largest
# over the moves, the two steps and both tracking modes, measured on the CPU backend.  Float32 rounding of the hit
# points moves the bilinear weights by ~1e-5 of a pixel, and with them l_h by ~1e-5 of the difference between
# neighbouring history pixels; `between` takes twice that times |l_c - l_h| (~0.5 on a 3-frame view), against a
# median s2 of ~1e-2 on scene 07.  A wrong tap or weight moves s2 by the value itself.  Asserted at 8x.
MEASURED = {"07": (8.50e-4, 8.48e-4), "04_box": (4.93e-4, 4.93e-4)}
DOF_BOUND = 1e-5  # relative: the bound of the length in test_temporal.py

# test_filter_against_float64 (levels 1..6, sigma_lum 4, min_batches 4): the metrics of test_denoise_var.py's
# float64 test, (colour, variance) per case, the largest over the levels, measured on the CPU backend ("special":
# test_special_values' frame, 3 levels, min_batches 2).  The variance of "walk" and "special" is that of a few
# pixels of the light sphere at the frame's left edge that take the SPATIAL estimate: rt_denoise_var.h's
# s2 / s0 - m1 m1 cancels squared luminances of an emitter in float32 (the same stage on the same colours through
# rt_denoise_var differs from float64 by 6e-3 of this metric there); where the spatial pixels are floor and sky
# ("uncover") it is 6e-6.  Asserted at 8x.
FILTER_MEASURED = {"walk": (6.76e-6, 1.30e-3), "uncover": (1.05e-6, 6.39e-6), "special": (2.75e-6, 2.00e-3)}
# test_special_values, the unfiltered variance of view B against the reference without the planted taps
SPECIAL_MEASURED = 8.80e-5
SIGMA, MIN_BATCHES = 4.0, 4

# test_scale_invariance: max |16 dim - bright| / (mean(bright) + |bright|) of the filtered colours of the walk's
# last view, default parameters, measured on the CPU backend: every stage scales exactly by powers of two but the
# 1e-10 floor of the sigma pass (test_denoise_var.py measured 1.26e-7 for the still camera; rt_temporal + rt_denoise
# with its fixed default sigma_color: 2.5).  Asserted at 8x.
SCALE_MEASURED = 9.44e-8


def tv(r, w, h, dv=None, **tp):
    """(rgba, colour, length, moments) of one call."""
    return r.temporal_var(w, h, denoise_var=dv, want_color=True, want_length=True, want_moments=True, **tp)


def path(scene, moves):
    cams = [view_a(scene)]
    for m in moves:
        cams.append(moved(cams[-1], **m))
    return cams


def render_view(r, camera, w, h, calls):
    """A new view: `calls` frames per render call (tracked: one batch each).  Returns (rgba, frameSum)."""
    r.set_camera(camera)
    for k in calls:
        out = r.render(w, h, k, BOUNCES, want_accum=True)
    return out


def own_moments(r, w, h, n):
    """(s2_c, dof_c) of the context's frame: the tracked moments when current."""
    j = r.moments_batches
    if j < 2:
        return 0.0, 0
    return r.variance(h, w).astype(np.float64) * n, j - 1


@pytest.fixture(scope="module")
def cpu(bwrt_lib):
    r = Renderer.cpu(0, lib=bwrt_lib)
    yield r
    r.set_background(0, 0, 0)
    r.close()


# ---- 1. ABI -----------------------------------------------------------------------------------
def test_abi_declares_the_entry_points(bwrt_lib):
    names = {"rt_temporal_var", "rt_temporal_var_device", "rt_last_temporal_var_ms"}
    assert names <= set(abi.declared_functions())
    header = open(abi.HEADER_PATH).read()
    for n in names:
        assert hasattr(bwrt_lib, n) and f" {n}(" in header
    assert bwrt_lib.rt_last_temporal_var_ms(None) == -1.0


# ---- 2. the colour path is rt_temporal's --------------------------------------------------------
@pytest.mark.parametrize("name,w,h", [("07", 67, 45), ("04_box", 64, 36)])
def test_colour_path_equals_rt_temporal(bwrt_lib, name, w, h):
    scene = scenes.SCENES[name]()
    cams = path(scene, [MOVES["yaw"], MOVES["sideways"], MOVES["dolly"], SECOND])
    plain = lambda r: r.temporal(w, h, want_color=True, want_length=True)  # noqa: E731
    var = lambda r: tv(r, w, h)[:3]  # noqa: E731
    # per view: which call each context makes; the last two alternate on ONE context (mixed history sets)
    plans = [[plain] * 5, [var] * 5, [plain, var, plain, var, plain], [var, plain, var, var, plain]]
    res = []
    for plan in plans:
        with Renderer.cpu(0, lib=bwrt_lib) as r:
            r.set_scene(scene)
            out = []
            for cam, call in zip(cams, plan):
                render_view(r, cam, w, h, (3,))
                out.append(call(r))
            res.append(out)
    assert res[0][-1][2].max() > 3 * 3  # lengths did chain through the views
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert A.same(a, b)


# ---- 3. the moments against float64 ---------------------------------------------------------------
@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("name,w,h,move", [("07", 67, 45, "yaw"), ("07", 67, 45, "sideways"), ("07", 67, 45, "dolly"),
                                           ("04_box", 64, 36, "sideways")])
def test_moments_against_float64(cpu, name, w, h, move, tracked):
    scene = scenes.SCENES[name]()
    cpu.set_scene(scene)
    cpu.set_background(*SKY)
    cpu.set_moments(tracked)
    cpu.init_rand(w, h)  # the same samples whatever ran before: MEASURED is of these
    cpu.temporal_reset()
    t = cpu.temporal_params()
    hist = None
    for step, cam in zip(("A", "A->B", "B->C"), path(scene, [MOVES[move], SECOND])):
        _, acc = render_view(cpu, cam, w, h, (2, 1) if tracked else (3,))
        assert cpu.moments_batches == (2 if tracked else 0)
        s2_c, dof_c = own_moments(cpu, w, h, 3)
        rgba, col, ln, mom = tv(cpu, w, h)
        aov = cpu.render_aov(w, h)
        ref = TV.temporal_var_ref(acc, 3, cam, aov, hist, s2_c, dof_c, t.max_history, t.normal_cos_min, t.plane_tol)
        keep = ~ref["marked"]
        pos = ref["dof"] > 0
        dof = mom[..., 1]
        if hist is None:  # no history: s2_c, dof_c
            assert (dof == dof_c).all()
            if not tracked:
                assert not mom.any()
        derr = float(np.max(np.abs(dof - ref["dof"])[keep & pos] / ref["dof"][keep & pos])) if pos.any() else 0.0
        assert np.array_equal(dof[keep & ~pos], ref["dof"][keep & ~pos])
        e_s2 = V.rel_err(mom[..., 0].astype(np.float64) * ln, ref["s2"], float(np.median(ref["s2"][pos])) if pos.any() else 0.0, keep)
        e_var = V.rel_err(mom[..., 0], ref["var"], float(np.median(ref["var"][pos])) if pos.any() else 0.0, keep)
        print(f"{name} {move} tracked={tracked} {step}: marked {ref['marked'].mean():.4f}, s2 {e_s2:.3e}, "
              f"variance {e_var:.3e}, dof {derr:.2e}")
        assert ref["marked"].mean() <= MARKED_CAP
        assert derr <= DOF_BOUND
        assert e_s2 <= 8 * MEASURED[name][0]
        assert e_var <= 8 * MEASURED[name][1]
        if hist is not None:
            assert ref["reprojected"].mean() > 0.5
            assert np.median(ref["var"][pos]) > 0
        hist = TV.history(cam, w, h, aov, col, ln, mom)
    cpu.set_moments(False)


# ---- 4. degrees of freedom add up ---------------------------------------------------------------
def unmoved_views(r, w, h, calls_per_view, **tp):
    """The same camera set again for every view; returns the interior four-tap
    pixels and every view's (length, moments)."""
    scene = scenes.scene_07()
    r.set_scene(scene)
    r.temporal_reset()
    ca = view_a(scene)
    out, full = [], None
    for i, calls in enumerate(calls_per_view):
        _, acc = render_view(r, ca, w, h, calls)
        if i == 1:
            t = r.temporal_params(**tp)
            ref = T.temporal_ref(acc, sum(calls), ca, r.render_aov(w, h), hist, t.max_history, t.normal_cos_min,
                                 t.plane_tol)
            full = ref["taps"] == 4
            full[[0, -1], :] = full[:, [0, -1]] = False
            assert full.mean() > 0.4
        _, col, ln, mom = tv(r, w, h, **tp)
        if i == 0:
            hist = T.history(ca, w, h, r.render_aov(w, h), col, ln)
        out.append((ln, mom))
    return full, out


def test_degrees_of_freedom_add_up(cpu):
    w, h = 67, 45
    cpu.set_moments(False)
    full, out = unmoved_views(cpu, w, h, [(2,), (3,), (2,)], max_history=8.0)
    for v, (ln, mom) in enumerate(out):  # V - 1 between-view terms
        assert np.max(np.abs(mom[..., 1][full] - v)) <= 1e-3
    assert np.max(np.abs(out[2][0][full] - 7)) <= 1e-3
    cpu.set_moments(True)
    full, out = unmoved_views(cpu, w, h, [(1, 1), (2, 1), (1, 1)], max_history=8.0)
    for v, (ln, mom) in enumerate(out):  # plus every view's J - 1 = 1
        assert np.max(np.abs(mom[..., 1][full] - (v + (v + 1)))) <= 1e-3
    # a capped history keeps no more degrees of freedom than frames: views of three batches bring dof_c = 2 each,
    # and the third view's history would hold 5 of them
    full, out = unmoved_views(cpu, w, h, [(1, 1, 1)] * 3, max_history=2.0)
    for v, (ln, mom) in enumerate(out):
        dof_h = mom[..., 1] - 2 - 1
        assert dof_h.max() <= 2 + 1e-3
        if v:
            assert np.max(np.abs(dof_h[full] - 2)) <= 1e-3 and np.max(np.abs(ln[full] - (2 + 3))) <= 1e-3
    cpu.set_moments(False)


# ---- 5. the estimator is a variance of the mean -------------------------------------------------------
@pytest.mark.parametrize("tracked", [False, True])
def test_estimator_is_a_variance_of_the_mean(bwrt_lib, tracked):
    w, h, reps, views = 48, 27, 64, 4
    scene = scenes.scene_07()
    ca = view_a(scene)
    lums, vars_ = [], []
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_scene(scene)
        r.set_moments(tracked)
        for _ in range(reps):  # the RNG streams continue: replicates are independent
            r.temporal_reset()
            for _ in range(views):
                render_view(r, ca, w, h, (1, 1) if tracked else (2,))
                _, col, ln, mom = tv(r, w, h, max_history=64.0)
            lums.append(V.lum(col.astype(np.float64)))
            vars_.append(mom[..., 0].astype(np.float64))
        prim = r.render_aov(w, h)["prim"]
    inner = np.zeros((h, w), bool)
    inner[1:-1, 1:-1] = True
    inner &= prim >= 0
    assert (np.abs(ln[inner] - 2 * views) < 1e-2).mean() > 0.9  # the views did add up
    ratio = np.mean(vars_, 0)[inner].sum() / np.var(lums, 0, ddof=1)[inner].sum()
    print(f"tracked={tracked}: sum of mean estimates / sum of empirical variances = {ratio:.3f} over {inner.sum()} pixels")
    assert 0.5 < ratio < 2


# ---- 6. the filter against float64 ---------------------------------------------------------------
CASES = {"walk": WALK, "uncover": WALK[:5] + [MOVES["sideways"]]}


@pytest.fixture(scope="module", params=list(CASES))
def last_view(request, bwrt_lib):
    """The last view of a camera path on scene 07 under the sky, 2 frames per
    view, tracking off: (case, renderer, camera, aov, unfiltered results)."""
    scene = scenes.scene_07()
    w, h = 67, 45
    r = Renderer.cpu(0, lib=bwrt_lib)
    r.set_scene(scene)
    r.set_background(*SKY)
    for cam in path(scene, CASES[request.param]):
        img, _ = render_view(r, cam, w, h, (2,))
        plain = tv(r, w, h)
    yield request.param, r, cam, w, h, img, r.render_aov(w, h), plain
    r.close()


@pytest.mark.parametrize("iterations", range(1, 7))
def test_filter_against_float64(last_view, iterations):
    case, r, cam, w, h, img, aov, (rgba0, col0, ln0, mom0) = last_view
    dv = dict(iterations=iterations, sigma_lum=SIGMA, min_batches=MIN_BATCHES)
    rgba, col, ln, mom = tv(r, w, h, dv)
    d = r.denoise_var_params(**dv)
    rc, rv, marked, temporal, v0 = TV.filter_ref(col0, mom0[..., 0], mom0[..., 1], cam, aov, iterations, d.sigma_lum,
                                                 d.sigma_normal, d.sigma_plane, d.min_batches)
    hit = aov["prim"] >= 0
    share = temporal[hit].mean()
    eps = float(np.median(v0))
    keep = ~marked
    e_c = V.rel_err(col, rc, 1.0, keep[..., None])
    e_v = V.rel_err(mom[..., 0], rv, eps, keep)
    print(f"{case} {iterations}: colour {e_c:.3e}, variance {e_v:.3e} (eps_v {eps:.3e}), marked {marked.mean():.4f}, "
          f"temporal source on {share:.3f} of the hit pixels")
    assert eps > 0 and marked.mean() <= MARKED_CAP
    if case == "uncover":  # both sources in one frame
        assert 0.05 <= share <= 0.95
    else:
        assert share > 0.5
    assert e_c <= 8 * FILTER_MEASURED[case][0]
    assert e_v <= 8 * FILTER_MEASURED[case][1]
    # the stored history is the unfiltered one
    assert np.array_equal(ln, ln0) and np.array_equal(mom[..., 1], mom0[..., 1])
    assert A.same(tv(r, w, h), (rgba0, col0, ln0, mom0))
    assert not np.array_equal(col, col0)
    ok = np.abs(rgba.astype(np.int32) - R.tone_map(rc).astype(np.int32)).max(-1) <= 1
    assert ok[keep].all()


def test_zero_iterations_is_the_unfiltered_call(last_view):
    case, r, cam, w, h, img, aov, plain = last_view
    assert A.same(tv(r, w, h, {"iterations": 0}), plain)


# ---- 7. scale invariance ---------------------------------------------------------------------------
def test_scale_invariance(bwrt_lib):
    w, h = 67, 45
    out = {}
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        for name, factor in (("bright", 1.0), ("dim", 0.0625)):
            scene = dim_scene(factor)
            r.set_scene(scene)
            r.init_rand(w, h)  # the same RNG streams for both
            accs = []
            for cam in path(scene, WALK):
                accs.append(render_view(r, cam, w, h, (2,))[1])
                tv(r, w, h)
            col = tv(r, w, h, {})[1]
            r.temporal_reset()
            for cam in path(scene, WALK):  # the fixed-sigma filter behind rt_temporal on the same frames
                render_view(r, cam, w, h, (2,))
                fixed = r.temporal(w, h, denoise={}, want_color=True)[1]
            out[name] = accs, col, fixed
    (accs_b, col_b, fix_b), (accs_d, col_d, fix_d) = out["bright"], out["dim"]
    for a_b, a_d in zip(accs_b, accs_d):
        assert np.array_equal(np.float32(16) * a_d, a_b) and a_b.any()
    s = float(col_b.mean())
    err = lambda d, b: float(np.max(np.abs(16.0 * d.astype(np.float64) - b) / (s + np.abs(b))))  # noqa: E731
    e_var, e_fix = err(col_d, col_b), err(fix_d, fix_b)
    print(f"rt_temporal_var + levels {e_var:.3e}; rt_temporal + rt_denoise with the default sigma_color {e_fix:.3e}")
    assert e_var <= 8 * SCALE_MEASURED


# ---- 8. special values -------------------------------------------------------------------------------
def special_sequence(r, w, h, history_values, current_values, dv):
    """test_temporal.py's: view A with non-finite frameSum pixels (the history),
    a yaw, view B with others."""
    scene = scenes.scene_07()
    r.set_scene(scene)
    r.set_background(*SKY)
    r.init_rand(w, h)
    ca = view_a(scene)
    cb = moved(ca, **MOVES["yaw"])
    r.set_camera(ca)
    r.render(w, h, 3, BOUNCES)
    aov_a = r.render_aov(w, h)
    hit = np.argwhere((aov_a["prim"][3:-3, 3:-3] >= 0)) + 3
    hist_px = [tuple(hit[len(hit) // 4]), tuple(hit[len(hit) // 2]), tuple(hit[3 * len(hit) // 4])]
    acc_a = plant(r, w, h, 3, hist_px, history_values)
    _, col, ln, mom = tv(r, w, h)
    for p in hist_px:  # a non-finite pixel passes through unchanged
        assert np.array_equal(col[p], (np.float32(1) / np.float32(3)) * acc_a[p], equal_nan=True)
    assert not mom.any()
    hist = TV.history(ca, w, h, aov_a, col, ln, mom)
    r.set_camera(cb)
    r.render(w, h, 3, BOUNCES)
    aov_b = r.render_aov(w, h)
    hit = np.argwhere((aov_b["prim"][3:-3, 3:-3] >= 0)) + 3
    cur_px = [tuple(hit[len(hit) // 3]), tuple(hit[2 * len(hit) // 3]), tuple(hit[len(hit) // 5])]
    acc_b = plant(r, w, h, 3, cur_px, current_values)
    return hist, cb, aov_b, acc_b, tv(r, w, h), tv(r, w, h, dv), hist_px, cur_px


def test_special_values(cpu):
    w, h = 67, 45
    nan, inf = np.nan, np.inf
    dv = dict(iterations=3, sigma_lum=SIGMA, min_batches=2)
    hist, cb, aov, acc, plain, filt, hist_px, cur_px = special_sequence(cpu, w, h, (nan, inf, inf), (inf, nan, inf), dv)
    rgba, col, ln, mom = plain
    t = cpu.temporal_params()
    ref = TV.temporal_var_ref(acc, 3, cb, aov, hist, 0.0, 0, t.max_history, t.normal_cos_min, t.plane_tol)
    inv = np.float32(1) / np.float32(3)
    others = np.ones((h, w), bool)
    for p in cur_px:  # planted in the current frame: unchanged, no history, nothing known
        assert np.array_equal(col[p], inv * acc[p], equal_nan=True)
        assert ln[p] == 3 and not mom[p].any()
        others[p] = False
    assert np.isfinite(col[others]).all() and np.isfinite(ln).all() and np.isfinite(mom).all()
    # the history's bad pixels are invalid taps, nothing else: the reference drops them
    keep = ~ref["marked"] & others
    pos = ref["dof"] > 0
    assert (ref["taps"] < 4)[pos].any()
    e_dof = float(np.max(np.abs(mom[..., 1] - ref["dof"])[keep & pos] / ref["dof"][keep & pos]))
    e_var = V.rel_err(mom[..., 0], ref["var"], float(np.median(ref["var"][pos])), keep)
    print(f"special values: variance {e_var:.3e}, dof {e_dof:.2e}, marked {ref['marked'].mean():.4f}")
    assert e_dof <= DOF_BOUND
    # the levels: the planted pixels pass through and spoil no neighbour
    frgba, fcol, fln, fmom = filt
    d = cpu.denoise_var_params(**dv)
    rc, rv, marked, temporal, v0 = TV.filter_ref(col, mom[..., 0], mom[..., 1], cb, aov, d.iterations, d.sigma_lum,
                                                 d.sigma_normal, d.sigma_plane, d.min_batches, masked=~others)
    for p in cur_px:
        assert np.array_equal(fcol[p], col[p], equal_nan=True)
    assert np.isfinite(fcol[others]).all() and np.isfinite(fmom[others]).all()
    keep = ~marked & others
    assert marked.mean() <= MARKED_CAP and temporal.any() and not temporal.all()
    e_c, e_v = V.rel_err(fcol, rc, 1.0, keep[..., None]), V.rel_err(fmom[..., 0], rv, float(np.median(v0)), keep)
    print(f"special values, 3 levels: colour {e_c:.3e}, variance {e_v:.3e}, marked {marked.mean():.4f}")
    assert e_c <= 8 * FILTER_MEASURED["special"][0]
    assert e_v <= 8 * FILTER_MEASURED["special"][1]
    assert e_var <= 8 * SPECIAL_MEASURED
    # which non-finite value a history pixel holds makes no difference to any other pixel
    again = special_sequence(cpu, w, h, (inf, nan, nan), (inf, nan, inf), dv)
    assert again[6] == hist_px and again[7] == cur_px
    assert A.same_values(again[4], plain) and A.same_values(again[5], filt)
    cpu.set_background(0, 0, 0)


def test_all_miss_frame(bwrt_lib):
    cam = scenes.Camera(scenes.vec(0, 0, 0), (C.c_float * 2)(0.0, 0.0), float(scenes.PI / np.float32(2)))
    empty = scenes.Scene(cam, [scenes.Sphere(scenes.vec(0, 0, 50), 1.0, scenes.material((1, 1, 1), 1))])  # behind
    w, h = 48, 27
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_scene(empty)
        r.set_background(0.5, 0.25, 0.125)
        for yaw in (0.0, 0.01):
            r.set_camera(scenes.Camera(scenes.vec(0, 0, 0), (C.c_float * 2)(yaw, 0.0), cam.fov))
            img = r.render(w, h, 2, 1)
            assert (r.render_aov(w, h)["prim"] < 0).all()
            for dv in (None, {}):
                rgba, col, ln, mom = tv(r, w, h, dv)
                assert np.array_equal(rgba, img) and (ln == 2).all() and not mom[..., 1].any()
                if dv is None:
                    assert not mom.any()
                else:  # the levels' variance is the spatial estimate s2 / s0 - m1 m1 of a flat frame: a few
                    # float32 roundings of the squared luminance, never a variance of the samples
                    lum2 = float(V.lum(col[0, 0].astype(np.float64))) ** 2
                    assert mom[..., 0].max() <= 8 * 2.0 ** -24 * lum2


# ---- 9. lifecycle, neutrality, errors -------------------------------------------------------------------
def test_no_history_after_a_drop(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 67, 45
    a = view_a(scene)
    b = moved(a, **MOVES["dolly"])

    def fresh(r, w, h, tracked):
        img, acc = render_view(r, a, w, h, (1, 1) if tracked else (2,))
        rgba, col, ln, mom = tv(r, w, h)
        assert np.array_equal(col, np.float32(0.5) * acc, equal_nan=True) and (ln == 2).all()
        assert np.array_equal(rgba, img)
        s2_c, dof_c = own_moments(r, w, h, 2)
        assert (mom[..., 1] == dof_c).all()
        if tracked:
            assert dof_c == 1 and np.allclose(mom[..., 0], s2_c / 2, rtol=1e-6, atol=0) and mom[..., 0].any()
        else:
            assert not mom.any()

    def second(r, w, h, tracked):
        render_view(r, b, w, h, (1, 1) if tracked else (2,))
        assert (tv(r, w, h)[3][..., 1] > (2 if tracked else 0)).any()  # a history now

    for tracked in (False, True):
        with Renderer.cpu(0, lib=bwrt_lib) as r:
            assert r.last_temporal_var_ms() == -1.0
            r.set_scene(scene)
            r.set_moments(tracked)
            fresh(r, w, h, tracked)
            assert r.last_temporal_var_ms() >= 0.0
            second(r, w, h, tracked)
            r.temporal_reset()
            fresh(r, w, h, tracked)
            second(r, w, h, tracked)
            r.set_scene(scene)
            fresh(r, w, h, tracked)
            second(r, w, h, tracked)
            fresh(r, w + 1, h, tracked)  # another frame shape
            second(r, w + 1, h, tracked)


def test_two_calls_in_one_view_are_identical(cpu):
    scene = scenes.scene_07()
    cpu.set_scene(scene)
    cpu.temporal_reset()
    w, h = 67, 45
    cams = path(scene, [MOVES["yaw"], SECOND])
    for cam in cams:
        render_view(cpu, cam, w, h, (2,))
        first = tv(cpu, w, h)
        assert A.same(tv(cpu, w, h), first)
        f1 = tv(cpu, w, h, {"iterations": 2})
        assert A.same(tv(cpu, w, h, {"iterations": 2}), f1)
        assert A.same(tv(cpu, w, h), first)
    assert first[3][..., 1].max() == 2


def neutrality_sequence(r, scene, w, h, with_calls):
    call = (lambda dv=None: tv(r, w, h, dv)) if with_calls else (lambda dv=None: None)
    r.set_scene(scene)
    r.set_moments(True)
    out = []
    r.render(w, h, 2, BOUNCES, first_frame=1)
    call()
    r.render(w, h, 1, BOUNCES)
    call({})
    out.append((r.moments_batches, r.variance(h, w)))
    r.set_camera(moved(scene.camera, **MOVES["yaw"]))
    r.render(w, h, 2, BOUNCES)
    call()
    call({"iterations": 1})
    img = r.render(w, h, 1, BOUNCES)
    call()
    out.append((img, r.frame_counter, r.moments_batches, r.variance(h, w)) + tuple(r.get_state(h, w)))
    return out


def test_neutrality(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 64, 36
    res = []
    for with_calls in (True, False):
        with Renderer.cpu(0, lib=bwrt_lib) as r:
            res.append(neutrality_sequence(r, scene, w, h, with_calls))
    assert A.same(res[0], res[1])
    assert res[0][1][1] == 4 and res[0][1][2] == 2


def test_errors(bwrt_lib):
    lib = bwrt_lib
    inv, uns = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED
    with Renderer.cpu(1, lib=lib) as r:
        t = lib.rt_temporal_params_default()
        d = lib.rt_denoise_var_params_default()
        call = lambda p=t, dv=None: lib.rt_temporal_var(r.ctx, C.byref(p), dv, None, None, None, None)  # noqa: E731
        assert lib.rt_temporal_var(None, C.byref(t), None, None, None, None, None) == inv
        assert lib.rt_temporal_var(r.ctx, None, None, None, None, None, None) == inv
        assert call() == abi.RT_ERR_NO_SCENE
        r.set_scene(scenes.scene_07())
        assert call() == inv and b"no frame" in lib.rt_last_error(r.ctx)
        r.render(16, 9, 1, 2, first_frame=1)
        assert call() == abi.RT_OK and call(t, C.byref(d)) == abi.RT_OK
        nan = float("nan")
        for field, value in (("max_history", 0.0), ("max_history", nan), ("plane_tol", -0.5), ("plane_tol", nan),
                             ("normal_cos_min", 1.5), ("normal_cos_min", nan)):
            bad = lib.rt_temporal_params_default()
            setattr(bad, field, value)
            assert call(bad) == inv, (field, value)
        for field, value in (("iterations", -1), ("iterations", abi.RT_DENOISE_MAX_ITERATIONS + 1), ("sigma_lum", 0.0),
                             ("sigma_lum", nan), ("sigma_plane", nan), ("sigma_normal", -1.0), ("min_batches", 1)):
            bad = lib.rt_denoise_var_params_default()
            setattr(bad, field, value)
            assert call(t, C.byref(bad)) == inv, (field, value)
        assert lib.rt_temporal_var_device(r.ctx, C.byref(t), None, None, None) == uns  # CPU context
        r.reset_accumulation()
        assert call() == inv
        r.render(16, 9, 1, 2, first_frame=1, row_offset=1, row_stride=2)  # a row shard, no assembled frame
        assert call() == uns
    assert lib.rt_last_temporal_var_ms(None) == -1.0


def test_non_uniform_frames_are_refused(bwrt_lib):
    lib = bwrt_lib
    w, h = 32, 18
    with Renderer.cpu(0, lib=lib) as r:
        r.set_scene(scenes.scene_07())
        r.set_moments(True)
        A.accumulate(r, w, h)
        assert r.temporal_var(w, h).shape == (h, w, 4)
        r.render_adaptive(w, h, BOUNCES, samples=1, min_frames=100)  # non-uniform
        t = r.temporal_params()
        for filters in (False, True):
            r.set_adaptive_filters(filters)
            assert lib.rt_temporal_var(r.ctx, C.byref(t), None, None, None, None, None) == abi.RT_ERR_UNSUPPORTED
            assert b"non-uniform" in lib.rt_last_error(r.ctx)
        assert r.temporal(w, h).shape == (h, w, 4)  # (rt_temporal takes it behind the switch)


def shard_outputs(rs, w, h, assemble=None):
    """assemble_case.temporal_outputs with rt_temporal_var: two views, each
    unfiltered and filtered."""
    out = []
    for v in range(2):
        if v:
            for i, r in enumerate(rs):
                r.controls(["LEFT"], A.DT)
                A.accumulate(r, w, h, i if len(rs) > 1 else 0, len(rs), restart=False)
        if assemble:
            assemble()
        for dv in (None, {"iterations": 2, "min_batches": 2}):
            out.append(tv(rs[0], w, h, dv))
    return out


@pytest.mark.parametrize("planes", [3, 5])
def test_a_shard_context_reads_its_assembled_frame(bwrt_lib, planes):
    w, h, s = 67, 45, 2
    scene = scenes.scene_07()
    full = A.full_context(bwrt_lib, scene, w, h, moments=planes == 5)
    rs = A.shard_contexts(bwrt_lib, scene, w, h, s, moments=planes == 5)
    try:
        want = shard_outputs([full], w, h)
        got = shard_outputs(rs, w, h, lambda: A.assemble_on(rs, w, h, planes))
        for a, b in zip(got, want):
            assert A.same(a, b)
        assert want[2][3][..., 1].max() == (1 + 2 * 2 if planes == 5 else 1)  # the frame's moments reached the merge
    finally:
        for r in [full] + rs:
            r.close()


# ---- 10. quality --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [1.0, 0.0625])
def test_quality_on_the_walk(bwrt_lib, factor):
    """tools/temporal_var_sweep.py's walk, bright and dim: against a 1024-frame
    render of the last view, the filtered frame beats rt_temporal's unfiltered one."""
    w, h = 160, 90
    scene = dim_scene(factor)
    cams = path(scene, WALK)
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_scene(scene)
        r.set_camera(cams[-1])
        r.render(w, h, 1024, BOUNCES, first_frame=1)
        truth = V.lum(r.get_state(h, w)[1].astype(np.float64) / 1024)
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_scene(scene)
        for cam in cams:
            render_view(r, cam, w, h, (2,))
            plain = r.temporal(w, h, want_color=True)[1]
        filtered = tv(r, w, h, {})[1]
    e = {k: float(np.abs(V.lum(c.astype(np.float64)) - truth).mean()) / factor for k, c in
         (("rt_temporal", plain), ("rt_temporal_var + levels", filtered))}
    print(f"factor {factor}: mean |luminance error| / factor: " + ", ".join(f"{k} {v:.5f}" for k, v in e.items()))
    assert e["rt_temporal_var + levels"] < e["rt_temporal"]


# ---- 11. the CLI -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [None, 3])
def test_cli_equals_the_python_path(bwrt_lib, tmp_path, levels):
    w, h, frames, mb, dt = 64, 36, 7, 3, 0.02
    keys = [["LEFT"], ["LEFT"], [], [], ["W", "RIGHT"], [], []]
    out = tmp_path / "t.ppm"
    cmd = [CLI, "--cpu", "2", "--width", str(w), "--height", str(h), "--frames", str(frames), "--max-bounces",
           str(mb), "--temporal-var"] + ([str(levels)] if levels else []) + \
          ["--keys", "LEFT*2,*2,W+RIGHT*1,*2", "--dt", str(dt), "--max-history", "16", "--sigma-lum", "8",
           "--min-batches", "3", "--out", str(out)]
    res = subprocess.run(cmd, check=True, capture_output=True, text=True)
    assert "temporal-var:" in res.stdout and "mean standard error" in res.stdout
    dv = {"iterations": levels, "sigma_lum": 8.0, "min_batches": 3} if levels else None
    with Renderer.cpu(2, lib=bwrt_lib) as r:
        r.set_scene(scenes.scene_07())
        r.set_max_bounces(mb)
        for i, k in enumerate(keys):
            raw = r.render_simple(w, h, 1)
            rgba = tv(r, w, h, dv if i == frames - 1 else None, max_history=16.0)[0]
            r.controls(k, dt)
    assert np.array_equal(read_ppm(out, w, h), rgba[::-1, :, :3])  # the file's first row is the top
    assert not np.array_equal(rgba, raw)


@pytest.mark.parametrize("other", [["--temporal"], ["--denoise", "2"], ["--denoise-var", "2"], ["--adaptive", "0.1"],
                                   ["--gpus", "2"]])
def test_cli_refuses_the_combinations(tmp_path, other):
    cmd = [CLI, "--cpu", "1", "--width", "16", "--height", "9", "--frames", "2", "--temporal-var",
           "--out", str(tmp_path / "t.ppm")] + other
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode != 0 and "--temporal-var" in res.stderr
