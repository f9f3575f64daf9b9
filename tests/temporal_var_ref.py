"""Float64 numpy restatement of the moment-carrying reprojection's
specification (bwidman-raytracer_amd/csrc/
rt_temporal_var.h) for the tests.  It builds on tests/temporal_ref.py (the
projection, the taps and their acceptance tests) and tests/denoise_var_ref.py
(the spatial estimate and the levels) by import; no library.

The tap sums of the moments are linear in the history planes, like the colour's:
temporal_ref is run a second time over a history whose three "colour" channels
hold {s2, dof, luminance of the history colour} (NaN where the real history
colour is not finite, so rule 5 decides alike) and a zero frameSum.  Its output
is then (1 - a) times the tap means, a = n / (len_h + n), which gives ss / sw,
sd / sw and l_h back without restating one acceptance test.

Inputs as temporal_ref's; a history (history()) also carries the float32 {s2,
dof} planes the library returned for the previous view, or none (a view that
plain rt_temporal wrote).  The current view's within-view estimate comes in as
s2_c (H, W) and the scalar dof_c; 0 and 0 when its moments are not tracked.
"""
import numpy as np

import denoise_ref as R
import denoise_var_ref as V
import temporal_ref as T

DOF_BAND = 1e-4  # |dof_out - (min_batches - 1.5)| below which the source of v0 is a rounding decision


def history(camera, width, height, aov, color, length, moments=None):
    """temporal_ref.history plus the per-frame variance and its degrees of
    freedom: `moments` is (H, W, 2) {variance of the mean, dof} as
    Renderer.temporal_var returns it unfiltered (s2 = variance * length), or
    None for a set without a moment plane."""
    h = T.history(camera, width, height, aov, color, length)
    if moments is None:
        h["s2"] = np.zeros((height, width))
        h["dof"] = np.zeros((height, width))
    else:
        h["s2"] = np.asarray(moments[..., 0], np.float64) * h["length"]
        h["dof"] = np.asarray(moments[..., 1], np.float64)
    return h


def history_planes(camera, width, height, aov, color, length, s2, dof):
    """The same from the raw planes (tests that plant values in them)."""
    h = T.history(camera, width, height, aov, color, length)
    h["s2"] = np.asarray(s2, np.float64)
    h["dof"] = np.asarray(dof, np.float64)
    return h


def temporal_var_ref(accum, n, camera, aov, hist, s2_c, dof_c, max_history, normal_cos_min, plane_tol):
    """One rt_temporal_var call without a filter.  Returns temporal_ref's dict
    plus "s2", "dof" and "var" (H, W) float64: the per-frame variance, its
    degrees of freedom and the variance of the mean luminance (0 where dof is
    0)."""
    base = T.temporal_ref(accum, n, camera, aov, hist, max_history, normal_cos_min, plane_tol)
    H, W = aov["prim"].shape
    s2_c = np.broadcast_to(np.asarray(s2_c, np.float64), (H, W))
    s2 = s2_c.copy()
    dof = np.full((H, W), float(dof_c))
    if hist is not None:
        with np.errstate(all="ignore"):
            ok = np.isfinite(hist["s2"]) & np.isfinite(hist["dof"]) & (hist["dof"] >= 0)
            planes = np.stack([np.where(ok, hist["s2"], 0.0), np.where(ok, hist["dof"], 0.0), V.lum(hist["color"])], -1)
            planes = np.where(np.isfinite(hist["color"]).all(-1)[..., None], planes, np.nan)
            zero = np.where(np.isfinite(accum), np.float32(0), accum)  # (a non-finite pixel stays one: no history)
            lin = T.temporal_ref(zero, n, camera, aov, dict(hist, color=planes), max_history, normal_cos_min,
                                 plane_tol)
            re = base["reprojected"]
            assert np.array_equal(re, lin["reprojected"]) and np.array_equal(base["taps"], lin["taps"])
            len_h = np.where(re, base["length"] - n, 1.0)
            mean = lin["color"] * ((len_h + n) / len_h)[..., None]  # out = (1 - a) mean
            s2_h, dof_h, l_h = mean[..., 0], np.minimum(mean[..., 1], len_h), mean[..., 2]
            c_new = (np.float32(1.0) / np.float32(n) * accum.astype(np.float32)).astype(np.float64)
            l_c = V.lum(np.where(re[..., None], c_new, 0.0))
            between = len_h * n / (len_h + n) * (l_c - l_h) ** 2
            dof_m = (dof_h + dof_c) + 1.0
            s2_m = ((dof_h * s2_h + dof_c * s2_c) + between) / dof_m
            s2 = np.where(re, s2_m, s2)
            dof = np.where(re, dof_m, dof)
    with np.errstate(all="ignore"):
        var = np.where(dof > 0, s2 / base["length"], 0.0)
    return dict(base, s2=s2, dof=dof, var=var)


def input_variance(color, var, dof, min_batches, normal, P, prim, sigma_normal, sigma_plane, masked=None):
    """The input stage of the levels: (v0, temporal (H, W) bool, marked).  color,
    var, dof: the unfiltered call's results (float32: the pending state is the
    stage's input)."""
    f32 = np.float32
    H, W = prim.shape
    c = np.asarray(color, np.float64)
    dof = np.asarray(dof, np.float64)
    thr = float(f32(min_batches) - f32(1.5))
    temporal = dof >= thr
    marked = np.abs(dof - thr) < DOF_BAND
    i_n = np.float64(f32(1.0) / (f32(sigma_normal) * f32(sigma_normal)))
    i_p = np.float64(f32(1.0) / (f32(sigma_plane) * f32(sigma_plane)))
    masked = np.zeros((H, W), bool) if masked is None else masked
    with np.errstate(all="ignore"):
        usable = np.isfinite(c).all(-1) & ~masked
        spatial = V.spatial_variance(c, normal.astype(np.float64), P.astype(np.float64), prim < 0, i_n, i_p, usable)
    return np.where(temporal, np.asarray(var, np.float64), spatial), temporal, marked


def filter_ref(color, var, dof, camera, aov, iterations, sigma_lum, sigma_normal, sigma_plane, min_batches,
               masked=None):
    """The levels behind the call: (colour, variance, marked, temporal, v0),
    float64.  color, var, dof as input_variance's."""
    prim = aov["prim"]
    H, W = prim.shape
    P = R.hit_points(camera, W, H, aov["depth"], prim)
    v0, temporal, marked = input_variance(color, var, dof, min_batches, aov["normal"], P, prim, sigma_normal,
                                          sigma_plane, masked)
    c, v, m = V.denoise_var_ref(np.asarray(color, np.float32), 1, aov["normal"], P, prim, iterations, sigma_lum,
                                sigma_normal, sigma_plane, var0=v0, masked=masked)
    return c, v, m | marked, temporal, v0
