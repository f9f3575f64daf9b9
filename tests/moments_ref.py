"""Float64 restatement of the luminance moment tracking (DESIGN.md section 11,
bwidman-raytracer_amd/csrc/rt_moments.h) for the tests.

Input: the frameSum snapshots (rows, W, 3) float32 after each tracked render
call and the frames k_j of each call.  Weighted Welford in float64 over the
batch mean luminances l_j = lum(a_j - a_{j-1}) / k_j.
"""
import numpy as np

LUM = np.array([0.2126, 0.7152, 0.0722])


def lum(c):
    return np.asarray(c, np.float64) @ LUM


def moments_ref(snapshots, ks):
    """(M, M2, n) after the batches: M the mean luminance over the n frames,
    M2 = sum_j k_j (l_j - M)^2."""
    prev = np.zeros(snapshots[0].shape, np.float64)
    M = np.zeros(snapshots[0].shape[:-1])
    M2 = np.zeros_like(M)
    n = 0
    for a, k in zip(snapshots, ks):
        a = a.astype(np.float64)
        l = lum(a - prev) / k
        n += k
        d = l - M
        M = M + d * (k / n)
        M2 = M2 + (k * d) * (l - M)
        prev = a
    return M, M2, n


def variance_ref(snapshots, ks):
    """(var, M): var = M2 / ((J - 1) n), the unbiased estimate of the variance
    of the mean luminance after n frames."""
    M, M2, n = moments_ref(snapshots, ks)
    return M2 / ((len(ks) - 1) * n), M


def rel_err(got, ref, scale):
    """max |got - ref| / (scale + |ref|)."""
    got = np.asarray(got, np.float64)
    return float(np.max(np.abs(got - ref) / (scale + np.abs(ref))))
