"""The post-render passes on a non-uniform accumulation (rt_set_adaptive_filters,
DESIGN.md section 15): the sequences that tests/test_adaptive_post.py (CPU
backend) and tests/test_gpu_adaptive_post.py (MI355X against the CPU backend)
share, and the count-aware float64 references.

The references are the uniform ones (denoise_ref, denoise_var_ref,
temporal_ref) given every pixel's own frame count: the specification changes
nothing but the count a pixel divides by, the per-pixel choice of the variance
source and the count a pixel blends with.
"""
import numpy as np

import denoise_ref as R
import denoise_var_ref as V
import temporal_ref as T
from test_adaptive import DEFAULTS, KS, start
from test_denoise_var import SIGMA, SKY
from test_temporal import MOVES, moved, view_a

ITERATIONS = (0, 1, 5, 6)


# ---- sequences ---------------------------------------------------------------------

def replay_state(r, scene, w, h, bounces, ks=KS):
    """The replay sequence of tests/test_adaptive.py with the switch on: the 4 x
    2 start (J = 4), then one adaptive call of the defaults per entry of ks.
    Returns (share the first call selected, RGBA and colour of the last call)."""
    start(r, scene, w, h, bounces)
    r.set_adaptive_filters(True)
    share = None
    for k in ks:
        img, col, st = r.render_adaptive(w, h, bounces, want_color=True, samples=k, **DEFAULTS)
        if share is None:
            share = st["selected"] / (w * h)
    return share, img, col


def mixed_state(r, scene, w, h, bounces, calls=2, sky=SKY):
    """Test 4's frame: 2 calls x 4 frames (base J = 2), then `calls` adaptive
    calls of 4 frames: a pixel selected every time reaches J_p = 2 + calls, one
    never selected stays at 2.  Scene under the sky, as the float64 comparisons
    of tests/test_denoise_var.py (the median variance is the metric's floor)."""
    r.set_scene(scene)
    r.set_background(*sky)
    r.init_rand(w, h)
    r.set_moments(True)
    r.set_adaptive_filters(True)
    r.render(w, h, 4, bounces, first_frame=1)
    r.render(w, h, 4, bounces)
    for _ in range(calls):
        r.render_adaptive(w, h, bounces, samples=4, **DEFAULTS)
    return r.counts(h, w)


def all_passes(r, w, h, iterations=ITERATIONS, min_batches=(4,), sigma_lum=SIGMA, temporal=True):
    """Every pass on the context's frame: a dict of tuples (RGBA first).  The
    temporal calls come last and in one order: they write the pending history."""
    out = {}
    for it in iterations:
        out["dn", it] = r.denoise(w, h, iterations=it, want_color=True)
        for mb in min_batches:
            out["dv", it, mb] = r.denoise_var(w, h, want_color=True, want_var=True, iterations=it, min_batches=mb,
                                              sigma_lum=sigma_lum)
    if temporal:
        out["tp"] = r.temporal(w, h, want_color=True, want_length=True)
        out["tp+dn"] = r.temporal(w, h, denoise={"iterations": 2}, want_color=True, want_length=True)
    return out


def first_view(r, scene, w, h, bounces, calls=(2, 2, 2, 2)):
    """test_temporal's view A (off the scene camera's axes) with the uniform
    start of tests/test_adaptive.py; the switch on.  Returns the camera."""
    r.set_scene(scene)
    r.init_rand(w, h)
    r.set_moments(True)
    r.set_adaptive_filters(True)
    cam = view_a(scene)
    r.set_camera(cam)
    for k in calls:
        r.render(w, h, k, bounces)
    return cam


def second_view(r, scene, w, h, bounces, calls=(2, 2, 2, 2)):
    """A yaw step: the accumulation restarts at frame 1, which ends the
    non-uniform state while the pending temporal result stays; then the uniform
    start again.  Returns the camera."""
    cam = moved(view_a(scene), **MOVES["yaw"])
    r.set_camera(cam)
    for k in calls:
        r.render(w, h, k, bounces)
    return cam


def same_pass_results(got, want):
    assert got.keys() == want.keys()
    for key in want:
        assert len(got[key]) == len(want[key])
        for i, (a, b) in enumerate(zip(got[key], want[key])):
            assert np.array_equal(a, b, equal_nan=True), (key, i)


def snapshot(r, w, h):
    """Everything a pass must leave alone: RNG state, frameSum, counts, moments, frame counter."""
    return r.get_state(h, w) + r.counts(h, w) + r.variance(h, w, want_lum=True) + (np.array(r.frame_counter),)


def same_snapshot(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y, equal_nan=True), i


# ---- float64 references -----------------------------------------------------------

def _n3(n):
    return np.asarray(n)[..., None]  # broadcasts over the colour planes where the references form 1 / n


def guides(r, scene, w, h, camera=None):
    a = r.render_aov(w, h)
    return a, R.hit_points(camera if camera is not None else scene.camera, w, h, a["depth"], a["prim"])


def denoise_cnt_ref(acc, n, aov, P, d):
    """rt_denoise with every pixel's own count: denoise_ref with inv per pixel."""
    return R.denoise_ref(acc, _n3(n), aov["normal"], P, aov["prim"], d.iterations, d.sigma_color, d.sigma_normal,
                         d.sigma_plane)


def denoise_var_cnt_ref(acc, n, j, tracked_var, aov, P, d, masked=None):
    """rt_denoise_var with the per-pixel choice: pixels with J_p >= min_batches
    take the tracked variance (float32, as rt_get_variance gives it: an input),
    the others the float64 spatial estimate over the count-aware colours.
    Returns (colour, variance, marked, tracked)."""
    f32 = np.float32
    H, W = aov["prim"].shape
    masked = np.zeros((H, W), bool) if masked is None else masked
    with np.errstate(all="ignore"):
        c = ((f32(1.0) / _n3(n).astype(f32)) * acc.astype(f32)).astype(np.float64)
        i_n = np.float64(f32(1.0) / (f32(d.sigma_normal) * f32(d.sigma_normal)))
        i_p = np.float64(f32(1.0) / (f32(d.sigma_plane) * f32(d.sigma_plane)))
        spatial = V.spatial_variance(c, aov["normal"].astype(np.float64), P.astype(np.float64), aov["prim"] < 0, i_n,
                                     i_p, np.isfinite(c).all(-1) & ~masked)
    tracked = j >= d.min_batches
    v0 = np.where(tracked, tracked_var.astype(np.float64), spatial)
    rc, rv, marked = V.denoise_var_ref(acc, _n3(n), aov["normal"], P, aov["prim"], d.iterations, d.sigma_lum,
                                       d.sigma_normal, d.sigma_plane, var0=v0, masked=masked)
    return rc, rv, marked, tracked


def temporal_cnt_ref(acc, n, camera, aov, hist, t):
    """rt_temporal with every pixel's own count: temporal_ref once per distinct
    count (a pixel's result depends on no other pixel's count), merged."""
    out = None
    for f in np.unique(n):
        ref = T.temporal_ref(acc, int(f), camera, aov, hist, t.max_history, t.normal_cos_min, t.plane_tol)
        if out is None:
            out = {k: v.copy() for k, v in ref.items()}
        m = n == f
        for k in out:
            out[k][m] = ref[k][m]
    return out
