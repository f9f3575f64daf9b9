"""Float64 restatement of the adaptive selection and of the per-pixel moment
tracking (bwidman-raytracer_amd/csrc/rt_adaptive.h) for
the tests.
"""
import numpy as np

from moments_ref import lum

MARGIN = 1e-4  # |sv cf - b b| within this of b b: the float32 sums may fall on either side


def select_ref(var, M, n, k, tolerance, lum_floor, radius, min_frames=0, max_frames=0):
    """(selected, marginal): the selection of rt_adaptive.h in float64 from the
    library's own per-pixel variance of the mean `var`, mean luminance `M` and
    frame counts `n`, all (H, W).  A tap whose var or M is not finite is
    skipped.  `marginal` marks the pixels whose test lies within MARGIN of its
    threshold (and whose selection the test alone decides)."""
    var = np.asarray(var, np.float64)
    M = np.asarray(M, np.float64)
    n = np.asarray(n, np.int64)
    h, w = var.shape
    ok = np.isfinite(var) & np.isfinite(M)
    v0 = np.where(ok, var, 0.0)
    m0 = np.where(ok, M, 0.0)
    sv = np.zeros((h, w))
    sm = np.zeros((h, w))
    c = np.zeros((h, w), np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if abs(dy) >= h or abs(dx) >= w:
                continue
            ys = slice(max(0, -dy), min(h, h - dy))
            xs = slice(max(0, -dx), min(w, w - dx))
            yq = slice(max(0, dy), min(h, h + dy))
            xq = slice(max(0, dx), min(w, w + dx))
            sv[ys, xs] += v0[yq, xq]
            sm[ys, xs] += m0[yq, xq]
            c[ys, xs] += ok[yq, xq]
    b = tolerance * (sm + c * lum_floor)
    lhs, rhs = sv * c, b * b
    hot = (c > 0) & (lhs > rhs)
    allowed = np.ones((h, w), bool) if max_frames == 0 else n + k <= max_frames
    forced = n < min_frames
    selected = allowed & (forced | hot)
    # (both sides exactly 0, no light yet and no floor, is not marginal: 0 > 0 is false in any precision)
    marginal = allowed & ~forced & (c > 0) & (np.abs(lhs - rhs) <= MARGIN * rhs) & (np.maximum(lhs, rhs) > 0)
    return selected, marginal, c


def pixel_moments_ref(snapshots, ks, took):
    """Per-pixel weighted Welford in float64: `snapshots` the frameSum (H, W, 3)
    after each call, `ks` its frames, `took` a bool (H, W) per call: the pixels
    the call rendered.  Returns (var of the mean, M, n, J)."""
    shape = snapshots[0].shape[:-1]
    prev = np.zeros(snapshots[0].shape, np.float64)
    M = np.zeros(shape)
    M2 = np.zeros(shape)
    n = np.zeros(shape)
    J = np.zeros(shape)
    for a, k, t in zip(snapshots, ks, took):
        a = a.astype(np.float64)
        l = lum(a - prev) / k
        n1 = n + k
        d = l - M
        M1 = M + d * (k / n1)
        M21 = M2 + (k * d) * (l - M1)
        M = np.where(t, M1, M)
        M2 = np.where(t, M21, M2)
        n = np.where(t, n1, n)
        J = np.where(t, J + 1, J)
        prev = np.where(t[..., None], a, prev)
    return M2 / ((J - 1) * n), M, n, J
