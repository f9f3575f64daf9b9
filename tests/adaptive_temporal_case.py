"""What the tests of adaptive sampling for a moving camera share
(tests/test_adaptive_temporal.py on the CPU backend,
tests/test_gpu_adaptive_temporal.py on the GPU): the
per-view loop (render, rt_temporal_var, rt_render_adaptive_reprojected,
rt_temporal_var_counted) and the float64 reference of the count-aware merge.

The reference extends tests/temporal_var_ref.py's operator by import.  The
operator is per pixel given the history planes: pixel p's result depends on its
own {n_p, J_p} and on nothing of the other pixels' counts.  So the count-aware
reference is the uniform one evaluated once per distinct pair (n, J) of the
frame and stitched together by the pixels' own pairs.
"""
import numpy as np

import assemble_case as A
import temporal_var_ref as TV
from test_temporal import BOUNCES, MOVES, SECOND, moved, view_a  # noqa: F401

K0, K = 2, 1  # frames of a view's uniform call and of each adaptive round
# the selection of the tests, whatever rt_adaptive_reprojected_params_default() says: a window, a tolerance at which
# it decides on these frames, and fresh = "no merged view yet"
BASE = dict(tolerance=0.1, lum_floor=0.01, radius=2, min_dof=1.0)


def tv(r, w, h, dv=None, **tp):
    return r.temporal_var(w, h, denoise_var=dv, want_color=True, want_length=True, want_moments=True, **tp)


def tvc(r, w, h, dv=None, **tp):
    return r.temporal_var_counted(w, h, denoise_var=dv, want_color=True, want_length=True, want_moments=True, **tp)


def path(scene, moves):
    cams = [view_a(scene)]
    for m in moves:
        cams.append(moved(cams[-1], **m))
    return cams


def new(lib, scene, gpu=False, threads=0):
    """A context with tracking and the filter switch on."""
    r = A.new(lib, gpu, threads)
    r.set_scene(scene)
    r.set_moments(True)
    r.set_adaptive_filters(True)
    return r


def begin_view(r, cam, w, h, k0=K0, bounces=BOUNCES):
    """Steps 1 and 2 of the loop: the uniform call (one tracked batch) and
    rt_temporal_var.  Returns the pending results."""
    r.set_camera(cam)
    r.render(w, h, k0, bounces)
    return tv(r, w, h)


def adaptive_round(r, w, h, k=K, bounces=BOUNCES, **params):
    """Step 3: (rgba, colour, stats, selected set) of one reprojected-adaptive call."""
    before = r.counts(h, w)[0]
    img, col, st = r.render_adaptive_reprojected(w, h, bounces, want_color=True, samples=k, **{**BASE, **params})
    took = r.counts(h, w)[0] != before
    assert st["selected"] == int(took.sum())
    return img, col, st, took


def loop(r, cams, w, h, rounds=1, dv=None, k0=K0, k=K, bounces=BOUNCES, **params):
    """The whole loop over `cams`.  Per view: the pending results, and per round
    (selected set, the counted call's results)."""
    out = []
    for cam in cams:
        view = {"pending": begin_view(r, cam, w, h, k0, bounces), "rounds": []}
        for _ in range(rounds):
            took = adaptive_round(r, w, h, k, bounces, **params)[3]
            view["rounds"].append((took, tvc(r, w, h, dv)))
        out.append(view)
    return out


def frame_state(r, w, h):
    """Counts, frameSum and RNG state of a full-frame context."""
    n, j = r.counts(h, w)
    rng, acc = r.get_state(h, w)
    return {"n": n, "j": j, "rng": rng, "accum": acc}


def own_moments_counted(r, w, h):
    """(s2_c, dof_c) per pixel of a non-uniform frame from the library's own
    readouts: M2_p / (J_p - 1) = rt_get_variance's value times n_p where J_p >= 2,
    else 0 and 0."""
    n, j = r.counts(h, w)
    var = r.variance(h, w).astype(np.float64)
    has = j >= 2
    return np.where(has, var * n, 0.0), np.where(has, j.astype(np.float64) - 1.0, 0.0), n, j


def temporal_var_counted_ref(accum, n, j, s2_c, camera, aov, hist, max_history, normal_cos_min, plane_tol):
    """rt_temporal_var_counted without a filter in float64: temporal_var_ref per
    distinct (n_p, J_p), each pixel taking the result of its own pair.  s2_c: (H,
    W), read only where J_p >= 2."""
    out = None
    for nv, jv in sorted({(int(a), int(b)) for a, b in zip(n.ravel(), j.ravel())}):
        m = (n == nv) & (j == jv)
        dof_c = jv - 1 if jv >= 2 else 0
        ref = TV.temporal_var_ref(accum, nv, camera, aov, hist, s2_c if jv >= 2 else 0.0, dof_c, max_history,
                                  normal_cos_min, plane_tol)
        if out is None:
            out = {k: np.array(v, copy=True) for k, v in ref.items()}
        for k, v in ref.items():
            out[k][m] = v[m]
    return out
