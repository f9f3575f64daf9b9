"""Adaptive sampling for a moving camera on the CPU
backend — no GPU needed: rt_render_adaptive_reprojected selects from the pending
planes of rt_temporal_var, rt_temporal_var_counted merges the non-uniform frame.
The GPU kernels compute the same bits (tests/test_gpu_adaptive_temporal.py
compares them with this backend).

The float64 references are tests/adaptive_ref.py (the selection) and
tests/adaptive_temporal_case.py over tests/temporal_var_ref.py (the merge).
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import adaptive_multi_case as M
import adaptive_ref as R
import adaptive_temporal_case as AT
import assemble_adaptive_case as AA
import assemble_case as A
import denoise_var_ref as V
import temporal_var_ref as TV
from adaptive_temporal_case import tv, tvc
from bwrt import Renderer, abi, scenes
from test_denoise_var import SKY, dim_scene
from test_temporal import BOUNCES, CLI, MARKED_CAP, MOVES, SECOND, read_ppm
from test_temporal_var import DOF_BOUND, MEASURED, WALK

TOL_BOX = 0.8
NAMES = {"rt_temporal_var_counted", "rt_temporal_var_counted_device", "rt_adaptive_reprojected_params_default",
         "rt_render_adaptive_reprojected", "rt_render_adaptive_reprojected_device"}

# test_moments_against_float64, measured on the CPU backend with the metric of tests/test_temporal_var.py (its
# MEASURED x 8 and DOF_BOUND are the bounds asserted): the largest over the moves and the three steps, (s2, variance
# of the mean, relative dof): scene 07 (7.52e-4, 7.49e-4, 6.2e-6), 04_box (1.98e-4, 1.98e-4, 3.1e-6); the marked
# share at most 0.0100 (profiles/adaptive_temporal/moments_f64.txt).  The per-pixel counts add no new cancellation.


# ---- 1. ABI -----------------------------------------------------------------------------------------
def test_abi_declares_the_entry_points(bwrt_lib):
    assert NAMES <= set(abi.declared_functions())
    header = open(abi.HEADER_PATH).read()
    for n in NAMES | {"rt_last_temporal_var_ms"}:  # the six symbols
        assert hasattr(bwrt_lib, n) and f" {n}(" in header
    assert "} rt_adaptive_reprojected_params;" in header
    d = bwrt_lib.rt_adaptive_reprojected_params_default()
    a = bwrt_lib.rt_adaptive_params_default()
    assert C.sizeof(abi.AdaptiveReprojectedParams) == C.sizeof(abi.AdaptiveParams) + 4
    for f in ("samples", "lum_floor", "min_frames", "max_frames"):
        assert getattr(d, f) == getattr(a, f), f
    # tools/adaptive_temporal_sweep.py's row (profiles/adaptive_temporal/sweep.txt)
    assert (d.tolerance, d.radius, d.min_dof) == (np.float32(0.4), 0, 4.0)
    for n in ("temporal_var_counted", "temporal_var_counted_device", "render_adaptive_reprojected",
              "render_adaptive_reprojected_device", "adaptive_reprojected_params"):
        assert callable(getattr(Renderer, n))


# ---- 2. select-all equals uniform -------------------------------------------------------------------
def one_view(r, cam, w, h, adaptive, dv, end_with_plain=False):
    """A view of K0 + K frames in two batches: through the loop with every
    pixel selected, or as two uniform calls.  Returns the view's last results."""
    AT.begin_view(r, cam, w, h)
    if adaptive:
        took = AT.adaptive_round(r, w, h, min_frames=1000)[3]
        assert took.all()
        n, j = r.counts(h, w)
        assert (n == AT.K0 + AT.K).all() and (j == 2).all()
    else:
        r.render(w, h, AT.K, BOUNCES)
    if end_with_plain:
        return r.temporal(w, h, want_color=True, want_length=True)
    return (tvc if adaptive else tv)(r, w, h, dv)


@pytest.mark.parametrize("levels", [0, 1, 5])
def test_select_all_equals_uniform(bwrt_lib, levels):
    scene = scenes.scene_07()
    w, h = 67, 45
    dv = {"iterations": levels, "min_batches": 2} if levels else None
    cams = AT.path(scene, [MOVES["yaw"], SECOND])
    res = []
    for adaptive in (True, False):
        with AT.new(bwrt_lib, scene) as r:
            r.set_adaptive_filters(adaptive)
            out = [one_view(r, cams[0], w, h, adaptive, dv)]           # without history
            out.append(one_view(r, cams[1], w, h, adaptive, dv))       # with one
            out.append(one_view(r, cams[2], w, h, adaptive, None, end_with_plain=True))
            out.append(one_view(r, cams[1], w, h, adaptive, dv))       # behind a history that rt_temporal wrote
            res.append(out)
    assert res[0][1][3][..., 1].max() > 2  # the moments did chain
    for a, b in zip(*res):
        assert A.same(a, b)


# ---- 3. the colour path is count-aware rt_temporal's ----------------------------------------------------
def test_colour_path_equals_counted_rt_temporal(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 67, 45
    cams = AT.path(scene, [MOVES["yaw"], MOVES["sideways"], MOVES["dolly"]])
    with AT.new(bwrt_lib, scene) as r, AT.new(bwrt_lib, scene) as twin:
        for v, cam in enumerate(cams):
            for c in (r, twin):
                AT.begin_view(c, cam, w, h)
                took = AT.adaptive_round(c, w, h)[3]
            assert 0 < took.sum() < w * h  # genuinely non-uniform
            got = tvc(r, w, h)
            plain = twin.temporal(w, h, want_color=True, want_length=True)
            assert A.same(got[:3], plain)
            # the twin's history sets then hold the same as r's: the calls alternate in any order
            assert A.same(tvc(twin, w, h), got)
        assert got[2].max() > 2 * (AT.K0 + AT.K)


# ---- 4. the moments against float64 ------------------------------------------------------------------------
# (the closed box is noisy everywhere: at the default tolerance every pixel is selected and the counts do not mix)
@pytest.mark.parametrize("name,w,h,move,tol", [("07", 67, 45, "yaw", 0.1), ("07", 67, 45, "sideways", 0.1),
                                               ("07", 67, 45, "dolly", 0.1), ("04_box", 64, 36, "sideways", TOL_BOX)])
def test_moments_against_float64(bwrt_lib, name, w, h, move, tol):
    scene = scenes.SCENES[name]()
    with AT.new(bwrt_lib, scene) as r:
        r.set_background(*SKY)
        t = r.temporal_params()
        hist = None
        for step, cam in zip(("A", "A->B", "B->C"), AT.path(scene, [MOVES[move], SECOND])):
            AT.begin_view(r, cam, w, h)
            AT.adaptive_round(r, w, h, tolerance=tol)
            s2_c, _, n, j = AT.own_moments_counted(r, w, h)
            assert len(np.unique(n)) > 1 and (j == 1).any() and (j == 2).any()  # mixed counts
            acc = r.get_state(h, w)[1]
            rgba, col, ln, mom = tvc(r, w, h)
            aov = r.render_aov(w, h)
            ref = AT.temporal_var_counted_ref(acc, n, j, s2_c, cam, aov, hist, t.max_history, t.normal_cos_min,
                                              t.plane_tol)
            keep = ~ref["marked"]
            pos = ref["dof"] > 0
            dof = mom[..., 1]
            if hist is None:
                assert np.array_equal(dof, np.where(j >= 2, j - 1, 0)) and np.array_equal(ln, n)
            derr = float(np.max(np.abs(dof - ref["dof"])[keep & pos] / ref["dof"][keep & pos]))
            assert np.array_equal(dof[keep & ~pos], ref["dof"][keep & ~pos])
            e_s2 = V.rel_err(mom[..., 0].astype(np.float64) * ln, ref["s2"], float(np.median(ref["s2"][pos])), keep)
            e_var = V.rel_err(mom[..., 0], ref["var"], float(np.median(ref["var"][pos])), keep)
            print(f"{name} {move} {step}: marked {ref['marked'].mean():.4f}, s2 {e_s2:.3e}, variance {e_var:.3e}, "
                  f"dof {derr:.2e}, counts {np.unique(n)}")
            assert ref["marked"].mean() <= min(MARKED_CAP, 0.01)  # at most 1 % of a case's pixels
            assert derr <= DOF_BOUND
            assert e_s2 <= 8 * MEASURED[name][0]
            assert e_var <= 8 * MEASURED[name][1]
            if hist is not None:
                assert ref["reprojected"].mean() > 0.5
            hist = TV.history(cam, w, h, aov, col, ln, mom)


# ---- 5. the selection against float64 -------------------------------------------------------------------------
def check_selection(r, w, h, pend, k=AT.K, **params):
    """One adaptive call against adaptive_ref.select_ref over the library's own
    pending results `pend`.  Returns (selected, fresh, taps)."""
    _, col, ln, mom = pend
    prim = r.render_aov(w, h)["prim"]
    d = r.adaptive_reprojected_params(samples=k, **{**AT.BASE, **params})
    var = np.where(mom[..., 1] > 0, mom[..., 0].astype(np.float64), np.nan)
    with np.errstate(all="ignore"):
        lum = V.lum(col.astype(np.float64))
    got = AT.adaptive_round(r, w, h, k, **params)[3]
    n_after = r.counts(h, w)[0]
    n0 = n_after - k * got
    fresh = (prim >= 0) & ~(mom[..., 1] >= d.min_dof)
    want, marginal, taps = R.select_ref(var, lum, n0, k, d.tolerance, d.lum_floor, d.radius, d.min_frames, d.max_frames)
    allowed = np.ones((h, w), bool) if d.max_frames == 0 else n0.astype(np.int64) + k <= d.max_frames
    want = want | (allowed & fresh)
    marginal = marginal & ~fresh
    assert marginal.mean() <= 0.02
    assert np.array_equal(got[~marginal], want[~marginal])
    return got, fresh, taps


@pytest.mark.parametrize("w,h", [(67, 45), (32, 18)])
@pytest.mark.parametrize("radius", [0, 2, 4])
def test_selection_against_float64(bwrt_lib, w, h, radius):
    scene = scenes.scene_07()
    cams = AT.path(scene, [MOVES["yaw"], MOVES["sideways"]])
    params = dict(tolerance=0.15, lum_floor=0.01, radius=radius)
    with AT.new(bwrt_lib, scene) as r:
        # the first view: every hit pixel is fresh, and nothing else is known: exactly they are selected
        pend = AT.begin_view(r, cams[0], w, h)
        hit = r.render_aov(w, h)["prim"] >= 0
        got, fresh, taps = check_selection(r, w, h, pend, **params)
        assert np.array_equal(fresh, hit) and np.array_equal(got, hit) and not taps.any() and 0 < hit.sum() < w * h
        # a second round in the view: dof 1 >= min_dof 1, the window decides
        got2, fresh2, taps2 = check_selection(r, w, h, tvc(r, w, h), **params)
        assert not fresh2.any() and taps2.any() and 0 < got2.sum() < w * h
        tvc(r, w, h)
        # a yaw, then a sideways move that uncovers background: fresh = the uncovered hit pixels
        for cam in cams[1:]:
            pend = AT.begin_view(r, cam, w, h)
            got, fresh, taps = check_selection(r, w, h, pend, **params)
            tvc(r, w, h)
        hit = r.render_aov(w, h)["prim"] >= 0
        assert 0 < fresh.sum() < hit.sum() and got[fresh].all() and not got.all()
        print(f"{w}x{h} radius {radius}: selected {got.mean():.3f}, fresh {fresh.mean():.3f} of hit {hit.mean():.3f}")


def test_selection_min_dof_and_cap(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 67, 45
    cams = AT.path(scene, [MOVES["sideways"]])
    with AT.new(bwrt_lib, scene) as r:
        # min_dof 0: no pixel is fresh, and in a first view nothing is known: nothing selected
        pend = AT.begin_view(r, cams[0], w, h)
        got, fresh, _ = check_selection(r, w, h, pend, min_dof=0.0)
        assert not fresh.any() and not got.any()
        assert (r.counts(h, w)[0] == AT.K0).all() and (r.counts(h, w)[1] == 1).all()
        # a large min_dof: every hit pixel, every round
        for _ in range(2):
            got, fresh, _ = check_selection(r, w, h, tvc(r, w, h), min_dof=100.0, tolerance=1e30)
            assert np.array_equal(got, r.render_aov(w, h)["prim"] >= 0)
        # the cap wins over fresh and over min_frames: n + k <= max_frames
        n = r.counts(h, w)[0]
        assert set(np.unique(n)) == {AT.K0, AT.K0 + 2 * AT.K}
        got, fresh, _ = check_selection(r, w, h, tvc(r, w, h), min_dof=100.0, min_frames=1000, max_frames=AT.K0 + AT.K)
        assert np.array_equal(got, n == AT.K0) and fresh[~got].any()
        # the second view with it
        pend = AT.begin_view(r, cams[1], w, h)
        got, fresh, _ = check_selection(r, w, h, pend, k=2, max_frames=3)
        assert not got.any() and fresh.any()


def test_selection_skips_non_finite_taps(bwrt_lib):
    """test_adaptive.py's: the small light of scene 07 with an infinite
    emittance.  Pixels that reached it hold a non-finite colour and, once they
    have two batches, a NaN s2: skipped as taps."""
    w, h = 67, 45
    scene = scenes.scene_07()
    scene.spheres[2].mat.emittance = float("inf")
    cams = AT.path(scene, [MOVES["yaw"]])
    with AT.new(bwrt_lib, scene) as r:
        for cam in cams:
            pend = AT.begin_view(r, cam, w, h, k0=4)
            for rnd in range(2):
                bad = ~np.isfinite(pend[1]).all(-1)
                known = pend[3][..., 1] > 0
                got, fresh, taps = check_selection(r, w, h, pend, radius=0 if rnd else 2, tolerance=0.15)
                pend = tvc(r, w, h)
                if rnd:  # radius 0: a window is its pixel
                    assert not taps[bad].any()
            assert 0.01 < bad.mean() < 0.95 and (bad & known).any()
            assert np.isnan(pend[3][..., 0][bad & (pend[3][..., 1] > 0)]).any()
        print(f"non-finite pixels {bad.mean():.3f}, of them with dof > 0 {(bad & known).sum()}")


# ---- 6. replay -------------------------------------------------------------------------------------------------
def uniform_from(lib, scene, cam, w, h, rng, upto):
    """frame count -> (RNG state, frameSum) of a uniform render of view `cam`
    that starts from the RNG state `rng`."""
    snaps = {}
    with Renderer.cpu(0, lib=lib) as u:
        u.set_scene(scene)
        u.set_camera(cam)
        u.init_rand(w, h)
        u.set_state(rng, np.zeros((h, w, 3), np.float32), 1)
        for f in range(1, upto + 1):
            u.render(w, h, 1, BOUNCES)
            snaps[f] = u.get_state(h, w)
    return snaps


def test_replay(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 67, 45
    cams = AT.path(scene, [MOVES["sideways"]])
    with AT.new(bwrt_lib, scene) as r:
        r.init_rand(w, h)
        for cam in cams:
            rng0 = r.get_state(h, w)[0]
            AT.begin_view(r, cam, w, h)
            for _ in range(2):
                img, col, st, took = AT.adaptive_round(r, w, h, tolerance=0.15)
                tvc(r, w, h)
            s = AT.frame_state(r, w, h)
            assert len(np.unique(s["n"])) == 3 and np.array_equal(s["j"], s["n"] - (AT.K0 - 1))
            assert st["frames_total"] == int(s["n"].sum())
            snaps = uniform_from(bwrt_lib, scene, cam, w, h, rng0, int(s["n"].max()))
            for f in np.unique(s["n"]):
                m = s["n"] == f
                rng, acc = snaps[int(f)]
                assert np.array_equal(s["rng"][:, m], rng[:, m]) and np.array_equal(s["accum"][m], acc[m]), f
            inv = (np.float32(1.0) / s["n"].astype(np.float32))[..., None]
            assert np.array_equal(col, inv * s["accum"])


def test_pending_planes_are_only_read(bwrt_lib):
    """The ABI has no readout of the pending planes but the call that writes
    them, so they are observed through the next view, whose history they are: a
    context whose adaptive call ran every stage but selected nothing (the cap)
    must give the bits of one that made no call."""
    scene = scenes.scene_07()
    w, h = 67, 45
    cams = AT.path(scene, [MOVES["yaw"]])
    res = []
    for call in (True, False):
        with AT.new(bwrt_lib, scene) as r:
            first = AT.begin_view(r, cams[0], w, h)
            if call:
                assert not AT.adaptive_round(r, w, h, min_frames=1000, max_frames=1)[3].any()
                assert A.same(tvc(r, w, h), first)  # (and the counted call on equal counts is the uniform one)
                assert not AT.adaptive_round(r, w, h, min_frames=1000, max_frames=1)[3].any()
            res.append((first, AT.begin_view(r, cams[1], w, h)))
    assert A.same(*res) and res[0][1][3][..., 1].max() == 1


# ---- 7. J_p = 1 -----------------------------------------------------------------------------------------------
def test_pixels_with_one_batch(bwrt_lib):
    scene = scenes.scene_07()
    w, h = 67, 45
    cam = AT.path(scene, [])[0]
    with AT.new(bwrt_lib, scene) as r, AT.new(bwrt_lib, scene) as twin:
        AT.begin_view(r, cam, w, h)
        took = AT.adaptive_round(r, w, h)[3]
        n, j = r.counts(h, w)  # rt_get_counts: the counts as they are
        assert np.array_equal(j, 1 + took) and np.array_equal(n, AT.K0 + AT.K * took) and 0 < took.sum() < w * h
        one = j == 1
        # the twin: the same frames as two uniform batches
        AT.begin_view(twin, cam, w, h)
        twin.render(w, h, AT.K, BOUNCES)
        # rt_get_variance: NaN (0 * inf) where J_p = 1, the twin's bits elsewhere
        var, lum = r.variance(h, w, want_lum=True)
        tvar, tlum = twin.variance(h, w, want_lum=True)
        assert np.isnan(var[one]).all() and A.same(var[~one], tvar[~one]) and A.same(lum[~one], tlum[~one])
        # rt_denoise_var's input stage (0 levels): tracked where J_p >= min_batches = 2, the spatial estimate at J_p = 1
        _, col, v0 = r.denoise_var(w, h, want_color=True, want_var=True, iterations=0, min_batches=2)
        assert A.same(v0[~one], var[~one]) and np.isfinite(v0[one]).all() and (v0[one] >= 0).all()
        _, _, vs = r.denoise_var(w, h, want_color=True, want_var=True, iterations=0, min_batches=AA.BIG)
        assert A.same(v0[one], vs[one])
        # rt_temporal_var_counted: no within-view term at J_p = 1, the twin's elsewhere (no history: s2_c, dof_c)
        got, want = tvc(r, w, h), tv(twin, w, h)
        assert not got[3][one].any() and (got[2][one] == AT.K0).all()
        for a, b in zip(got, want):
            assert A.same(a[~one], b[~one])
        # the counted export and assembly carry the 1
        block, bn, bj = r.export_shard_adaptive(h, w, 7)
        assert (bn, bj) == (AT.K0, 1)
        assert np.array_equal(block[5].view(np.uint32), n) and np.array_equal(block[6].view(np.uint32), j)
        # the selection from the tracked moments skips such taps; its entry point keeps refusing a one-batch base
        d = r.adaptive_params()
        assert r.lib.rt_render_adaptive(r.ctx, C.byref(d), BOUNCES, None, None, None) == abi.RT_ERR_INVALID_ARGUMENT
        assert b"2 batches" in r.lib.rt_last_error(r.ctx)
        assert np.array_equal(r.counts(h, w)[0], n)


# ---- 8. errors and lifecycle ------------------------------------------------------------------------------------
def test_errors_and_lifecycle(bwrt_lib):
    lib = bwrt_lib
    inv, uns = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED
    scene = scenes.scene_07()
    w, h, mb = 33, 17, 2
    cams = AT.path(scene, [MOVES["yaw"], SECOND])
    with Renderer.cpu(2, lib=lib) as r:
        def call(max_bounces=mb, **kw):
            d = r.adaptive_reprojected_params(**kw)
            return lib.rt_render_adaptive_reprojected(r.ctx, C.byref(d), max_bounces, None, None, None)

        def unchanged():
            return (r.counts(h, w)[0] == 2).all() and r.frame_counter == 3

        t = lib.rt_temporal_params_default()
        counted = lambda: lib.rt_temporal_var_counted(r.ctx, C.byref(t), None, None, None, None, None)  # noqa: E731
        assert lib.rt_render_adaptive_reprojected(None, None, mb, None, None, None) == inv
        assert call() == abi.RT_ERR_NO_SCENE and counted() == abi.RT_ERR_NO_SCENE
        r.set_scene(scene)
        r.set_camera(cams[0])
        assert call() == inv and counted() == inv
        r.render(w, h, 2, mb)
        assert call() == inv and b"tracking not live" in lib.rt_last_error(r.ctx)  # tracking off
        r.set_moments(True)
        r.set_camera(cams[0])
        r.render(w, h, 2, mb)
        assert call() == inv and b"no pending" in lib.rt_last_error(r.ctx)
        r.temporal(w, h)
        assert call() == inv and b"no moments" in lib.rt_last_error(r.ctx)  # a set rt_temporal wrote
        r.temporal_var(w, h)
        for bad in (dict(min_dof=-1.0), dict(min_dof=float("nan")), dict(samples=0), dict(tolerance=0.0),
                    dict(tolerance=float("nan")), dict(lum_floor=-0.5), dict(radius=-1),
                    dict(radius=abi.RT_ADAPTIVE_MAX_RADIUS + 1)):
            assert call(**bad) == inv, bad
        assert call(max_bounces=abi.RT_MAX_BOUNCES + 1) == uns
        assert lib.rt_render_adaptive_reprojected(r.ctx, None, mb, None, None, None) == inv
        d = r.adaptive_reprojected_params()
        assert lib.rt_render_adaptive_reprojected_device(r.ctx, C.byref(d), mb, None, None) == uns  # CPU context
        assert lib.rt_temporal_var_counted_device(r.ctx, C.byref(t), None, None, None) == uns
        # (RT_PRECISION_REFERENCE_FAST exists on GPU contexts only: tests/test_gpu_adaptive_temporal.py)
        assert unchanged()
        # a camera call: the tracking is not current, and the pending set is of an older view
        r.set_camera(cams[1])
        assert call() == inv and b"render first" in lib.rt_last_error(r.ctx)
        r.render(w, h, 2, mb)
        assert call() == inv and b"no pending" in lib.rt_last_error(r.ctx)
        assert unchanged()
        r.temporal_var(w, h)
        # the call, then what the non-uniform state refuses and takes
        assert call(samples=1) == abi.RT_OK
        n = r.counts(h, w)[0]
        assert set(np.unique(n)) == {2, 3}
        assert counted() == uns and b"non-uniform" in lib.rt_last_error(r.ctx)  # the switch is off
        for filters in (False, True):
            r.set_adaptive_filters(filters)
            assert lib.rt_temporal_var(r.ctx, C.byref(t), None, None, None, None, None) == uns
            assert b"non-uniform" in lib.rt_last_error(r.ctx)
        assert counted() == abi.RT_OK and call(samples=1) == abi.RT_OK  # repeated calls in one view
        _, col, ln, mom = tvc(r, w, h)
        assert r.last_temporal_var_ms() >= 0.0
        # a camera move ends the non-uniform state; the next view's history carries per-pixel lengths and moments
        r.set_camera(cams[2])
        r.render(w, h, 2, mb)
        assert (r.counts(h, w)[0] == 2).all() and (r.counts(h, w)[1] == 1).all()
        _, col2, ln2, mom2 = tv(r, w, h)
        aov = r.render_aov(w, h)
        hist = TV.history(cams[1], w, h, r_aov_of(lib, scene, cams[1], w, h), col, ln, mom)
        ref = TV.temporal_var_ref(r.get_state(h, w)[1], 2, cams[2], aov, hist, 0.0, 0, t.max_history, t.normal_cos_min,
                                  t.plane_tol)
        keep = ~ref["marked"] & ref["reprojected"]
        assert keep.mean() > 0.3 and len(np.unique(np.round(ln2[keep]))) > 2
        assert np.max(np.abs(ln2 - ref["length"])[keep] / ref["length"][keep]) <= 1e-5
        assert np.max(np.abs(mom2[..., 1] - ref["dof"])[keep] / ref["dof"][keep]) <= DOF_BOUND
        # a row shard
        r.render(w, h, 2, mb, first_frame=1, row_offset=1, row_stride=2)
        assert call() == uns and b"row shard" in lib.rt_last_error(r.ctx)


def r_aov_of(lib, scene, cam, w, h):
    with Renderer.cpu(1, lib=lib) as u:
        u.set_scene(scene)
        u.set_camera(cam)
        return u.render_aov(w, h)


# ---- 9. a counted assembled frame ----------------------------------------------------------------------------------
def counted_outputs(rs, w, h, params, assemble=None):
    """assemble_adaptive_case.temporal_outputs with rt_temporal_var_counted: two
    views, each unfiltered and with two levels."""
    out = []
    for view in range(2):
        if view:
            for i, r in enumerate(rs):
                r.controls(["LEFT"], A.DT)
                A.accumulate(r, w, h, i if len(rs) > 1 else 0, len(rs), restart=False)
        if assemble:
            M.two_phase(rs, w, h, params)
            assemble()
        else:
            M.full_call(rs[0], w, h, params)
        for dv in (None, {"iterations": 2, "min_batches": 2}):
            out.append(tvc(rs[0], w, h, dv))
    return out


@pytest.mark.parametrize("planes", [4, 7])
def test_a_shard_context_reads_its_counted_assembled_frame(bwrt_lib, planes):
    w, h, s = 67, 45, 2
    params = AA.sequence(w, h)[0]
    rs = AA.shards_after(bwrt_lib, "07", w, h, s, [])
    # the oracle of a 4-plane frame has the counts and no moments: tracking off behind the adaptive calls is not a
    # state the library has, so its oracle is the 7-plane one's colour, length and RGBA, and moments of the history alone
    full = AA.full_after(bwrt_lib, "07", w, h, [])
    try:
        want = counted_outputs([full], w, h, params)
        got = counted_outputs(rs, w, h, params, lambda: AA.assemble_on(rs, w, h, planes))
        n, j = rs[0].assembled_counts(w, h)
        assert len(np.unique(n)) > 1
        for i, (a, b) in enumerate(zip(got, want)):
            if planes == 7:
                assert A.same(a, b), i
            elif i % 2 == 0:  # unfiltered: the colour path does not read the moments
                assert A.same(a[:3], b[:3]), i
        if planes == 7:
            assert want[2][3][..., 1].max() > 4  # the frame's moments reached the merge
        else:
            assert not got[0][3].any() and got[2][3][..., 1].max() == 1  # no within-view term: the between term alone
        t = rs[0].lib.rt_temporal_params_default()
        rs[0].set_adaptive_filters(False)
        assert rs[0].lib.rt_temporal_var_counted(rs[0].ctx, C.byref(t), None, None, None, None, None) == \
            abi.RT_ERR_UNSUPPORTED
        assert b"non-uniform" in rs[0].lib.rt_last_error(rs[0].ctx)
    finally:
        M.close(rs + [full])


# ---- 10. the loop does something ---------------------------------------------------------------------------------------
def test_the_loop_does_something(bwrt_lib):
    """On a short walk, against a 512-frame render of every view: the loop's
    filtered frame has a lower mean luminance error than the same view's filtered
    frame before its adaptive rounds (it has more samples), and from the second
    view on the selected share lies strictly between 0 and 1.  The comparison at
    EQUAL samples is tools/adaptive_temporal_sweep.py's, which is reported in
    DESIGN.md section 22 and not asserted here."""
    w, h = 80, 45
    scene = dim_scene(1.0)
    cams = AT.path(scene, WALK[:4])
    truths = []
    with Renderer.cpu(0, lib=bwrt_lib) as u:
        u.set_scene(scene)
        for cam in cams:
            u.set_camera(cam)
            u.render(w, h, 512, BOUNCES)
            truths.append(V.lum(u.get_state(h, w)[1].astype(np.float64) / 512))
    before, after, shares = [], [], []
    with AT.new(bwrt_lib, scene) as r:
        for cam, truth in zip(cams, truths):
            AT.begin_view(r, cam, w, h)
            err = lambda c: float(np.abs(V.lum(c.astype(np.float64)) - truth).mean())  # noqa: E731
            before.append(err(tv(r, w, h, {})[1]))
            for _ in range(2):
                shares.append(float(AT.adaptive_round(r, w, h)[3].mean()))
                col = tvc(r, w, h, {})[1]
            after.append(err(col))
    print("mean |luminance error| per view before the rounds " + " ".join(f"{e:.5f}" for e in before) +
          ", after " + " ".join(f"{e:.5f}" for e in after) + "; selected shares " + " ".join(f"{s:.3f}" for s in shares))
    assert all(a < b for a, b in zip(after, before))
    assert all(0 < s < 1 for s in shares[2:])


# tools/adaptive_temporal_sweep.py (profiles/adaptive_temporal/sweep.txt): at equal mean frames per view the loop's
# error over the uniform path's is 0.961 as the mean over 4 sets of samples, seed-to-seed standard deviation 0.015 (its
# 160x90 cases; single cases 0.90 .. 1.005).  Asserted with three of those standard deviations: the margin reaches just
# past 1, so this test says "not worse than uniform at equal samples", and cannot tell the measured 4 % from a tie.
# Measured with this test's smaller frame and 512-frame truth: 0.987, standard deviation 0.020.
EQUAL_SAMPLES_BOUND = 0.961 + 3 * 0.015


def test_equal_samples_against_uniform(bwrt_lib):
    """The sweep's comparison at this suite's size, the defaults of
    rt_adaptive_reprojected_params_default(): 2 + 2 frames per view through the
    loop against 2, 3 and 4 uniform frames per view through rt_temporal_var, both
    with the default levels on the last view, the uniform error interpolated at
    the loop's mean frames; 4 sets of samples."""
    w, h, k0, k = 80, 45, 2, 2
    scene = dim_scene(1.0)
    cams = AT.path(scene, WALK)
    with Renderer.cpu(0, lib=bwrt_lib) as u:
        u.set_scene(scene)
        u.set_camera(cams[-1])
        u.render(w, h, 512, BOUNCES)
        truth = V.lum(u.get_state(h, w)[1].astype(np.float64) / 512)
    err = lambda c: float(np.abs(V.lum(c.astype(np.float64)) - truth).mean())  # noqa: E731

    def context(seed):
        r = AT.new(bwrt_lib, scene)
        r.init_rand(w, h)
        if seed:  # other samples: the RNG streams advanced
            r.render(w, h, 5 * seed, BOUNCES, first_frame=1)
        return r

    ratios = []
    for seed in range(4):
        uniform = {}
        for m in range(k0, k0 + k + 1):
            with context(seed) as r:
                for i, cam in enumerate(cams):
                    r.set_camera(cam)
                    r.render(w, h, m, BOUNCES)
                    col = tv(r, w, h, {} if i == len(cams) - 1 else None)[1]
            uniform[m] = err(col)
        shares = []
        with context(seed) as r:
            for i, cam in enumerate(cams):
                r.set_camera(cam)
                r.render(w, h, k0, BOUNCES)
                tv(r, w, h)
                shares.append(r.render_adaptive_reprojected(w, h, BOUNCES, samples=k)[1]["selected"] / (w * h))
                col = tvc(r, w, h, {} if i == len(cams) - 1 else None)[1]
        frames = k0 + k * float(np.mean(shares))
        lo = min(int(frames), k0 + k - 1)
        ratios.append(err(col) / ((lo + 1 - frames) * uniform[lo] + (frames - lo) * uniform[lo + 1]))
        assert k0 < frames < k0 + k
    print(f"loop / uniform at equal frames per seed: " + " ".join(f"{x:.3f}" for x in ratios) +
          f"; mean {np.mean(ratios):.3f}, standard deviation {np.std(ratios, ddof=1):.3f}")
    assert np.mean(ratios) <= EQUAL_SAMPLES_BOUND


# ---- 11. the CLI ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,rounds", [(None, 1), (3, 2)])
def test_cli_equals_the_python_path(bwrt_lib, tmp_path, levels, rounds):
    w, h, frames, mb, dt, tol = 64, 36, 5, 3, 0.02, 0.15
    keys = [["LEFT"], ["LEFT"], [], ["W", "RIGHT"], []]
    out = tmp_path / "t.ppm"
    cmd = [CLI, "--cpu", "2", "--width", str(w), "--height", str(h), "--frames", str(frames),
           "--max-bounces", str(mb), "--temporal-var"] + ([str(levels)] if levels else []) + \
          ["--adaptive-temporal", str(tol), "--adaptive-rounds", str(rounds), "--keys", "LEFT*2,*1,W+RIGHT*1,*1",
           "--dt", str(dt), "--max-history", "16", "--sigma-lum", "8", "--min-batches", "3", "--out", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert res.stdout.count("adaptive-temporal:") == frames * rounds
    dv = {"iterations": levels, "sigma_lum": 8.0, "min_batches": 3} if levels else None
    with Renderer.cpu(2, lib=bwrt_lib) as r:
        r.set_scene(scenes.scene_07())
        r.set_max_bounces(mb)
        r.set_moments(True)
        r.set_adaptive_filters(True)
        for i, k in enumerate(keys):
            if r.frame_counter == 1:  # a new view; an unmoved camera goes on with the rounds alone
                r.render_simple(w, h, 1)
                tv(r, w, h, None, max_history=16.0)
            for rnd in range(rounds):
                _, st = r.render_adaptive_reprojected(w, h, mb, samples=1, tolerance=tol)
                last = i == frames - 1 and rnd == rounds - 1
                rgba = tvc(r, w, h, dv if last else None, max_history=16.0)[0]
            r.controls(k, dt)
        assert 0 < st["selected"] < w * h
    assert np.array_equal(read_ppm(out, w, h), rgba[::-1, :, :3])


@pytest.mark.parametrize("args", [["--adaptive-temporal", "0.1"],
                                  ["--temporal-var", "--adaptive-temporal", "0.1", "--gpus", "2"],
                                  ["--temporal-var", "--adaptive-temporal", "0.1", "--precision", "fast"],
                                  ["--temporal-var", "--adaptive-rounds", "2"],
                                  ["--temporal-var", "--adaptive-temporal", "0.1", "--adaptive-rounds", "0"]])
def test_cli_refuses_the_combinations(tmp_path, args):
    cmd = [CLI, "--cpu", "1", "--width", "16", "--height", "9", "--frames", "2", "--out", str(tmp_path / "t.ppm")] + args
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode != 0 and "--adaptive-" in res.stderr
