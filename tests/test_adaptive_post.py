"""The denoisers and the reprojection on a non-uniform accumulation
(rt_set_adaptive_filters) on the CPU backend — no GPU
needed.  The GPU kernels compute the same bits (tests/test_gpu_adaptive_post.py
compares them with this backend).

With the switch on, rt_denoise, rt_denoise_var and rt_temporal take every
pixel's own counts {n_p, J_p}.  Three kinds of oracle: a non-uniform state whose
counts are all equal gives the uniform passes' bits; exact identities with what
rt_render_adaptive, rt_get_counts and rt_get_variance return; and the float64
references of the uniform passes given per-pixel counts
(tests/adaptive_post_ref.py), under the uniform passes' own bounds.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import adaptive_post_ref as A
import denoise_ref as R
import denoise_var_ref as V
import temporal_ref as T
from bwrt import Renderer, abi, scenes
from test_adaptive import CLI, DEFAULTS, mae, start
from test_denoise import FILTER_BOUND
from test_denoise_var import COLOR_BOUND, MAX_MARKED, SIGMA, VAR_BOUND
from test_temporal import LENGTH_BOUND, MARKED_CAP, MEASURED

W, H, MB = 67, 45, 4


@pytest.fixture(scope="module")
def replay(bwrt_lib):
    """A CPU context behind the replay sequence of scene 07 (counts 8, 12, 13,
    16; J_p 4..7), with what its last adaptive call returned."""
    scene = scenes.scene_07()
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        share, img, col = A.replay_state(r, scene, W, H, MB)
        yield r, scene, share, img, col


@pytest.fixture(scope="module")
def mixed(bwrt_lib):
    """A CPU context behind test 4's recipe: J_p = 4 where both adaptive calls
    selected the pixel, 2 where neither did."""
    scene = scenes.scene_07()
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        n, j = A.mixed_state(r, scene, W, H, MB)
        yield r, scene, n, j


# ---- 1. interface --------------------------------------------------------------------

def test_interface(bwrt_lib):
    lib = bwrt_lib
    names = {"rt_set_adaptive_filters", "rt_get_adaptive_filters"}
    assert names <= set(abi.declared_functions())
    for name in names:
        assert hasattr(lib, name)
    assert lib.rt_set_adaptive_filters(None, 1) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_get_adaptive_filters(None) == 0
    scene = scenes.scene_07()
    w, h, mb = 33, 17, 2
    with Renderer.cpu(2, lib=lib) as r:
        assert r.adaptive_filters is False  # off by default
        dn, dv, tp = r.denoise_params(), r.denoise_var_params(), r.temporal_params()
        calls = (lambda: lib.rt_denoise(r.ctx, C.byref(dn), None, None),
                 lambda: lib.rt_denoise_var(r.ctx, C.byref(dv), None, None, None),
                 lambda: lib.rt_temporal(r.ctx, C.byref(tp), None, None, None, None),
                 lambda: lib.rt_temporal(r.ctx, C.byref(tp), C.byref(dn), None, None, None))
        start(r, scene, w, h, mb)
        r.set_adaptive_filters(True)  # on a uniform accumulation: nothing to lift
        assert r.adaptive_filters is True
        uniform = A.all_passes(r, w, h, iterations=(0, 5), temporal=False)
        r.set_adaptive_filters(False)
        A.same_pass_results(A.all_passes(r, w, h, iterations=(0, 5), temporal=False), uniform)
        r.render_adaptive(w, h, mb, samples=2, **DEFAULTS)
        for call in calls:  # the contract tests/test_adaptive.py pins
            assert call() == abi.RT_ERR_UNSUPPORTED
            assert b"non-uniform" in lib.rt_last_error(r.ctx)
        r.set_adaptive_filters(True)
        for call in calls:
            assert call() == abi.RT_OK
        assert r.last_denoise_ms() >= 0 and r.last_denoise_var_ms() >= 0 and r.last_temporal_ms() >= 0
        # what the switch does not lift
        params = r.params(w, h, 1, mb)
        for first in (0, 9, 2):
            params.first_frame = first
            assert lib.rt_render_ex(r.ctx, C.byref(params), None, None) == abi.RT_ERR_UNSUPPORTED, first
        arr = (C.c_void_p * 1)(r.ctx.value)
        assert lib.rt_render_multi(arr, 1, w, h, 1, None) == abi.RT_ERR_UNSUPPORTED
        assert lib.rt_denoise_device(r.ctx, C.byref(dn), None, None) == abi.RT_ERR_UNSUPPORTED  # CPU context
        assert lib.rt_denoise_var_device(r.ctx, C.byref(dv), None, None) == abi.RT_ERR_UNSUPPORTED
        assert lib.rt_temporal_device(r.ctx, C.byref(tp), None, None, None) == abi.RT_ERR_UNSUPPORTED
        r.set_adaptive_filters(False)
        for call in calls:
            assert call() == abi.RT_ERR_UNSUPPORTED
        assert r.frame_counter == 9 and r.moments_batches == 4  # the uniform base, untouched


# ---- 2. select-all equals uniform ---------------------------------------------------------

def test_select_all_equals_uniform(bwrt_lib):
    """Two contexts with the same call boundaries; the adaptive one selects every
    pixel (min_frames 1000), so it is in the non-uniform state with all n_p = 11
    and J_p = 5: every pass gives the uniform context's bits.  min_batches 5 is
    at J (tracked), 6 above it (spatial).  Then a yaw step and the same again:
    the temporal calls of the second view have a history."""
    scene = scenes.scene_07()
    k = 3
    with Renderer.cpu(0, lib=bwrt_lib) as a, Renderer.cpu(0, lib=bwrt_lib) as u:
        A.first_view(a, scene, W, H, MB)
        A.first_view(u, scene, W, H, MB)
        for view in (0, 1):
            _, st = a.render_adaptive(W, H, MB, samples=k, min_frames=1000, **DEFAULTS)
            u.render(W, H, k, MB)
            assert st["selected"] == W * H
            assert (a.counts(H, W)[0] == 8 + k).all() and u.frame_counter == 9 + k
            assert lib_refuses_uniform_continuation(a)
            got = A.all_passes(a, W, H, min_batches=(5, 6))
            want = A.all_passes(u, W, H, min_batches=(5, 6))
            A.same_pass_results(got, want)
            assert not np.array_equal(want["dv", 5, 5][1], want["dv", 5, 6][1])  # two variance sources
            assert (want["tp"][2] > 8 + k).any() == (view == 1)  # the second view reprojects
            assert not np.array_equal(want["tp"][0], want["tp+dn"][0])
            if view == 0:
                A.second_view(a, scene, W, H, MB)
                A.second_view(u, scene, W, H, MB)


def lib_refuses_uniform_continuation(r):
    p = r.params(W, H, 1, MB)
    return r.lib.rt_render_ex(r.ctx, C.byref(p), None, None) == abi.RT_ERR_UNSUPPORTED


# ---- 3. exact identities on a genuinely non-uniform frame -----------------------------------

def test_exact_identities(replay):
    r, scene, share, img, col = replay
    print(f"first call selected {100 * share:.1f} %")
    assert 0.2 < share < 0.8
    n, j = r.counts(H, W)
    assert len(np.unique(n)) >= 3 and (j >= 4).all()
    rgba, c0 = r.denoise(W, H, iterations=0, want_color=True)
    assert np.array_equal(c0, col, equal_nan=True) and np.array_equal(rgba, img)
    rgba, c0, ln = r.temporal(W, H, want_color=True, want_length=True)  # no history
    assert np.array_equal(ln, n.astype(np.float32))
    assert np.array_equal(c0, col, equal_nan=True) and np.array_equal(rgba, img)
    rgba, c0, v0 = r.denoise_var(W, H, want_color=True, want_var=True, iterations=0, min_batches=4)
    assert np.array_equal(v0, r.variance(H, W), equal_nan=True)  # every pixel tracked
    assert np.array_equal(c0, col, equal_nan=True) and np.array_equal(rgba, img)
    # min_batches inside the range of J_p: the tracked pixels keep rt_get_variance's bits
    v6 = r.denoise_var(W, H, want_var=True, iterations=0, min_batches=6)[1]
    tracked = j >= 6
    assert 0.05 < tracked.mean() < 0.95
    assert np.array_equal(v6[tracked], r.variance(H, W)[tracked], equal_nan=True)
    assert not np.array_equal(v6[~tracked], r.variance(H, W)[~tracked])


# ---- 4, 5. float64 references ------------------------------------------------------------

@pytest.mark.parametrize("iterations", range(1, 7))
def test_mixed_variance_sources_against_float64(mixed, iterations):
    """One frame, both variance sources.  The bounds are the uniform filter's:
    the per-pixel operations are the same.  The variance bound is the spatial
    mode's: the frame holds spatial estimates, and every level mixes them into
    their neighbours."""
    r, scene, n, j = mixed
    tracked = j >= 4
    print(f"tracked {tracked.mean():.3f}, spatial {(~tracked).mean():.3f}, counts {np.unique(n)}")
    assert tracked.mean() >= 0.05 and (~tracked).mean() >= 0.05
    acc = r.get_state(H, W)[1]
    aov, P = A.guides(r, scene, W, H)
    d = r.denoise_var_params(iterations=iterations, sigma_lum=SIGMA, min_batches=4)
    rgba, col, var = r.denoise_var(W, H, want_color=True, want_var=True, iterations=iterations, sigma_lum=SIGMA,
                                   min_batches=4)
    rc, rv, marked, rt = A.denoise_var_cnt_ref(acc, n, j, r.variance(H, W), aov, P, d)
    assert np.array_equal(rt, tracked)
    v0 = r.denoise_var(W, H, want_var=True, iterations=0, min_batches=4)[1]
    assert np.array_equal(v0[tracked], r.variance(H, W)[tracked])
    eps = float(np.median(v0))
    keep = ~marked
    e_c = V.rel_err(col, rc, 1.0, keep[..., None])
    e_v = V.rel_err(var, rv, eps, keep)
    print(f"mixed {iterations}: colour {e_c:.3e}, variance {e_v:.3e} (eps_v {eps:.3e}), marked {marked.mean():.4f}")
    assert eps > 0
    assert marked.mean() <= MAX_MARKED
    assert e_c <= COLOR_BOUND
    assert e_v <= VAR_BOUND["spatial"]
    ok = np.abs(rgba.astype(np.int32) - R.tone_map(rc).astype(np.int32)).max(-1) <= 1
    assert ok[keep].all()


def test_spatial_input_stage_against_float64(mixed):
    """iterations 0: the spatial pixels' v0 over count-aware taps."""
    r, scene, n, j = mixed
    acc = r.get_state(H, W)[1]
    aov, P = A.guides(r, scene, W, H)
    d = r.denoise_var_params(iterations=0, min_batches=4)
    v0 = r.denoise_var(W, H, want_var=True, iterations=0, min_batches=4)[1]
    ref = A.denoise_var_cnt_ref(acc, n, j, r.variance(H, W), aov, P, d)[1]
    e = V.rel_err(v0, ref, float(np.median(ref)), j < 4)
    print(f"spatial v0 of the untracked pixels: {e:.3e}")
    assert e <= VAR_BOUND["spatial"]


@pytest.mark.parametrize("iterations", range(1, 7))
def test_denoise_against_float64(replay, iterations):
    r, scene, share, img, col = replay
    n = r.counts(H, W)[0]
    acc = r.get_state(H, W)[1]
    aov, P = A.guides(r, scene, W, H)
    d = r.denoise_params(iterations=iterations)
    rgba, got = r.denoise(W, H, iterations=iterations, want_color=True)
    ref = A.denoise_cnt_ref(acc, n, aov, P, d)
    err = R.rel_err(got, ref)
    print(f"rt_denoise {iterations} levels on counts {np.unique(n)}: {err:.3e}")
    assert err <= FILTER_BOUND
    assert (np.abs(rgba.astype(np.int32) - R.tone_map(ref).astype(np.int32)) <= 1).all()
    # the uniform base's count for every pixel is measurably another filter
    wrong = R.denoise_ref(acc, 8, aov["normal"], P, aov["prim"], iterations, d.sigma_color, d.sigma_normal,
                          d.sigma_plane)
    assert R.rel_err(got, wrong) > 100 * FILTER_BOUND


def test_temporal_against_float64(bwrt_lib):
    """Two views, both non-uniform when their temporal call runs: the history
    of the second carries per-pixel lengths."""
    scene = scenes.scene_07()
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        t = r.temporal_params()
        cam = A.first_view(r, scene, W, H, MB)
        hist = None
        for view in (0, 1):
            for k in (3, 1):
                r.render_adaptive(W, H, MB, samples=k, **DEFAULTS)
            n = r.counts(H, W)[0]
            assert len(np.unique(n)) >= 3
            acc = r.get_state(H, W)[1]
            rgba, col, ln = r.temporal(W, H, want_color=True, want_length=True)
            aov = r.render_aov(W, H)
            ref = A.temporal_cnt_ref(acc, n, cam, aov, hist, t)
            keep = ~ref["marked"]
            err = T.rel_err(col, ref["color"], keep)
            lerr = float(np.max(np.abs(ln[keep] - ref["length"][keep]) / ref["length"][keep]))
            print(f"view {view}: colour {err:.3e}, length {lerr:.2e}, marked {ref['marked'].mean():.4f}, "
                  f"reprojected {ref['reprojected'].mean():.3f}")
            assert ref["marked"].mean() <= MARKED_CAP
            assert lerr <= LENGTH_BOUND
            assert err <= 8 * MEASURED["07"]
            if view == 0:
                assert np.array_equal(ln, n.astype(np.float32))
                hist = T.history(cam, W, H, aov, col, ln)
                cam = A.second_view(r, scene, W, H, MB)
            else:
                assert ref["reprojected"].mean() > 0.5
                assert len(np.unique(hist["length"])) >= 3  # per-pixel history lengths
                assert (ln[ref["reprojected"] & keep] > n[ref["reprojected"] & keep]).all()


# ---- 6. non-finite pixels --------------------------------------------------------------------

def test_non_finite_pixels(bwrt_lib):
    """The infinite-emittance light of test_selection_skips_non_finite_taps: a
    pixel whose path reached it holds an infinite or NaN frameSum and non-finite
    moments.  Centres pass through, taps are skipped."""
    scene = scenes.scene_07()
    scene.spheres[2].mat.emittance = float("inf")
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        share, img, col = A.replay_state(r, scene, W, H, MB, ks=(3, 1))
        n, j = r.counts(H, W)
        bad = ~np.isfinite(col).all(-1)
        vbad = bad | ~np.isfinite(r.variance(H, W))
        print(f"non-finite colours {bad.mean():.3f}, colours or variances {vbad.mean():.3f}, counts {np.unique(n)}")
        assert 0.01 < bad.mean() < 0.95 and len(np.unique(n)) >= 2
        for it in (1, 5):
            c = r.denoise(W, H, iterations=it, want_color=True)[1]
            assert np.array_equal(c[bad], col[bad], equal_nan=True)
            assert np.isfinite(c[~bad]).all() and not np.array_equal(c[~bad], col[~bad])
            _, c, v = r.denoise_var(W, H, want_color=True, want_var=True, iterations=it, min_batches=4)
            assert np.array_equal(c[vbad], col[vbad], equal_nan=True)
            assert np.array_equal(v[vbad], r.variance(H, W)[vbad], equal_nan=True)
            assert np.isfinite(c[~vbad]).all() and np.isfinite(v[~vbad]).all()
            assert not np.array_equal(c[~vbad], col[~vbad])
        # the spatial window skips them too (min_batches above every J_p)
        v = r.denoise_var(W, H, want_var=True, iterations=0, min_batches=64)[1]
        assert np.isfinite(v).all()
        # reprojection: a non-finite history tap is skipped, a non-finite centre passes through
        r.temporal(W, H)
        A.second_view(r, scene, W, H, MB)
        r.render_adaptive(W, H, MB, want_color=True, samples=3, **DEFAULTS)
        _, col2, _ = r.render_adaptive(W, H, MB, want_color=True, samples=1, **DEFAULTS)
        _, c, ln = r.temporal(W, H, want_color=True, want_length=True)
        bad2 = ~np.isfinite(col2).all(-1)
        n2 = r.counts(H, W)[0]
        assert bad2.any() and (ln > n2).any()
        assert np.array_equal(c[bad2], col2[bad2], equal_nan=True) and np.array_equal(ln[bad2], n2[bad2])
        assert np.isfinite(c[~bad2]).all() and np.isfinite(ln).all()


# ---- 7. neutrality ----------------------------------------------------------------------------

def test_neutrality(bwrt_lib):
    scene = scenes.scene_07()
    with Renderer.cpu(0, lib=bwrt_lib) as r, Renderer.cpu(0, lib=bwrt_lib) as twin:
        _, img, _ = A.replay_state(r, scene, W, H, MB, ks=(3, 1))
        A.replay_state(twin, scene, W, H, MB, ks=(3, 1))
        before = A.snapshot(r, W, H)
        for run in (lambda: r.denoise(W, H), lambda: r.denoise(W, H, iterations=0),
                    lambda: r.denoise_var(W, H, min_batches=5), lambda: r.denoise_var(W, H, min_batches=64),
                    lambda: r.temporal(W, H), lambda: r.temporal(W, H, denoise={})):
            run()
            A.same_snapshot(A.snapshot(r, W, H), before)
        assert np.array_equal(r.denoise(W, H, iterations=0), img)  # the frame the adaptive call left
        got = r.render_adaptive(W, H, MB, want_color=True, samples=4, **DEFAULTS)
        want = twin.render_adaptive(W, H, MB, want_color=True, samples=4, **DEFAULTS)
        assert got[2]["selected"] == want[2]["selected"] and 0 < got[2]["selected"] < W * H
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)
        A.same_snapshot(A.snapshot(r, W, H), A.snapshot(twin, W, H))


# ---- 8. thread-count invariance ------------------------------------------------------------------

def test_thread_count_invariance(bwrt_lib):
    scene = scenes.scene_07()
    runs = []
    for threads in (1, 3, 8):
        with Renderer.cpu(threads, lib=bwrt_lib) as r:
            A.mixed_state(r, scene, W, H, MB)
            runs.append(A.all_passes(r, W, H, iterations=(0, 5)))
    for other in runs[1:]:
        A.same_pass_results(other, runs[0])


# ---- 9. quality ordering -----------------------------------------------------------------------

def test_quality_ordering(bwrt_lib):
    """The sequence of tests/test_adaptive.py test_quality_ordering (160x90, the
    defaults from the 4 x 2 start to a mean of 32 frames, against 2048 frames):
    the adaptive frame through rt_denoise_var is closer to the truth than the
    raw adaptive frame.  Only the ordering is asserted (the ratios:
    profiles/adaptive_post/sweep.txt)."""
    scene = scenes.scene_07()
    w, h, mb = 160, 90, 4
    with Renderer.cpu(0, lib=bwrt_lib) as r:
        r.set_scene(scene)
        truth = r.render(w, h, 2048, mb, first_frame=1)
        start(r, scene, w, h, mb)
        r.set_adaptive_filters(True)
        mean = 8.0
        while mean < 32.0:
            img, st = r.render_adaptive(w, h, mb)
            mean = st["frames_total"] / (w * h)
        den = r.denoise_var(w, h)
    e_raw, e_den = mae(img, truth), mae(den, truth)
    print(f"mean count {mean:.1f}: raw adaptive MAE {e_raw:.2f}, adaptive + rt_denoise_var {e_den:.2f}")
    assert e_den < e_raw


# ---- 10. CLI -----------------------------------------------------------------------------------

def test_cli_adaptive_filters(tmp_path):
    base = [CLI, "--cpu", "2", "--width", "64", "--height", "36", "--frames", "24", "--frames-per-call", "2",
            "--max-bounces", "3", "--adaptive", "0.1"]
    raw = tmp_path / "raw.ppm"
    subprocess.run(base + ["--out", str(raw)], check=True, capture_output=True)
    for name, extra, says in (("dv", ["--denoise-var"], "denoise-var: 5 levels, per-pixel variance source"),
                              ("dn", ["--denoise"], "denoise: 5 levels"),
                              ("tp", ["--temporal", "--keys", "*12,LEFT*2,*10"], "temporal:")):
        out = tmp_path / f"{name}.ppm"
        res = subprocess.run(base + ["--adaptive-filters", "--out", str(out)] + extra, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        assert says in res.stdout and "adaptive: mean" in res.stdout
        assert out.stat().st_size == raw.stat().st_size and out.read_bytes() != raw.read_bytes()
        res = subprocess.run(base + extra, capture_output=True, text=True)  # without the flag: as ever
        assert res.returncode == 2 and "--adaptive cannot be combined" in res.stderr
    for bad in (["--precision", "fast"], ["--gpus", "2"]):
        res = subprocess.run(base + ["--adaptive-filters"] + bad, capture_output=True, text=True)
        assert res.returncode == 2 and "--adaptive cannot be combined" in res.stderr, bad
