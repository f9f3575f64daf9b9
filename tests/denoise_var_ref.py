"""Float64 numpy restatement of the variance-guided filter's specification
(bwidman-raytracer_amd/csrc/rt_denoise_var.h) for the
tests: shifted-array taps, np.exp, no library.

Inputs are what the public interface gives: frameSum (H, W, 3) float32, the
frame count n, the feature buffers of Renderer.render_aov (the hit point P
restated from the camera, tests/denoise_ref.py) and, for the tracked mode, the
variance of rt_get_variance.  The float32 inputs of the filter (c0, the tracked
v0, the per-call constants) are formed in float32 as the specification says;
everything else is float64.

Decisions.  The library decides in float32 whether a tap counts (e >= 0, w > 0
with exp_nn's cut-off at e > 87, the finiteness tests).  The reference applies
the same rules and *marks* every pixel with a tap whose decision sits within
1e-4 relative of a threshold — e of 87, or a magnitude of the float32 maximum:
their comparison would test the rounding of a decision, not the filter.  (e >=
0 has no such band: e is a sum of non-negative terms or NaN.  A tap at the
cut-off weighs e^-87 of the centre's, so the value of a marked pixel is still
right to ~1e-38 relative and the pixels that take it as a tap need no mark;
a pixel marked for a magnitude at the float32 maximum stays marked and marks
those that count it.)  `masked` pixels (the non-finite ones a test injects) are
taken out of the tap sets of the spatial window and of the levels, as the
library's rules do; their own variance estimate stays finite and counts in the
sigma pass.
"""
import numpy as np

from denoise_ref import K

LUM = np.array([0.2126, 0.7152, 0.0722])
F32_MAX = float(np.finfo(np.float32).max)
EXP_CUT = 87.0
BAND = 1e-4


def lum(c):
    return c @ LUM


def _shift(H, W, oy, ox):
    """Slices (p, q) of the pixels p whose tap q = p + (oy, ox) is in the image."""
    yp = slice(max(0, -oy), H - max(0, oy))
    yq = slice(max(0, oy), H - max(0, -oy))
    xp = slice(max(0, -ox), W - max(0, ox))
    xq = slice(max(0, ox), W - max(0, -ox))
    return (yp, xp), (yq, xq)


def _near_overflow(x):
    return np.abs(np.abs(x) - F32_MAX) <= BAND * F32_MAX


def _geom(nrm, P, p, q, i_n, i_p):
    dn = nrm[q] - nrm[p]
    en = (dn * dn).sum(-1) * i_n
    pd = (nrm[p] * (P[q] - P[p])).sum(-1)
    return en, (pd * pd) * i_p


def spatial_variance(c, nrm, P, miss, i_n, i_p, usable):
    """v0 of the spatial mode; `usable`: finite colour and not masked."""
    H, W = miss.shape
    s0 = np.zeros((H, W))
    s1 = np.zeros((H, W))
    s2 = np.zeros((H, W))
    lq = lum(np.where(usable[..., None], c, 0.0))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            if abs(dy) >= H or abs(dx) >= W:
                continue
            p, q = _shift(H, W, dy, dx)
            en, ex = _geom(nrm, P, p, q, i_n, i_p)
            wn = np.exp(-(en + ex))
            wn = np.where((en + ex) > EXP_CUT, 0.0, wn)
            ok = (miss[q] == miss[p]) & usable[q]
            s0[p] += np.where(ok, wn, 0.0)
            s1[p] += np.where(ok, wn * lq[q], 0.0)
            s2[p] += np.where(ok, wn * (lq[q] * lq[q]), 0.0)
    pos = s0 > 0
    s0 = np.where(pos, s0, 1.0)
    m1 = s1 / s0
    return np.where(pos, np.maximum(s2 / s0 - m1 * m1, 0.0), 0.0)


def sigma_pass(v, vfin, sigma_lum):
    """rs = 1 / (sigma_lum sqrt(g) + 1e-10), g the 3x3 Gaussian of the finite v."""
    H, W = v.shape
    sv = np.zeros((H, W))
    sw = np.zeros((H, W))
    vz = np.where(vfin, v, 0.0)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if abs(dy) >= H or abs(dx) >= W:
                continue
            p, q = _shift(H, W, dy, dx)
            k = (0.5 if dy == 0 else 0.25) * (0.5 if dx == 0 else 0.25)
            sv[p] += np.where(vfin[q], k * vz[q], 0.0)
            sw[p] += np.where(vfin[q], k, 0.0)
    pos = sw > 0
    g = sv / np.where(pos, sw, 1.0)
    with np.errstate(all="ignore"):
        return np.where(pos, 1.0 / (np.float64(np.float32(sigma_lum)) * np.sqrt(g) + np.float64(np.float32(1e-10))), 0.0)


def denoise_var_ref(accum, n, normal, P, prim, iterations, sigma_lum, sigma_normal, sigma_plane, var0=None,
                    masked=None):
    """(colour (H, W, 3), variance (H, W), marked (H, W) bool), float64.
    var0: the tracked variance (float32, as rt_get_variance gives it); None:
    the spatial estimate.  masked: pixels no other pixel may take as a tap."""
    f32 = np.float32
    H, W = prim.shape
    with np.errstate(all="ignore"):
        inv = f32(1.0) / f32(n)
        c = (inv * accum.astype(f32)).astype(np.float64)
        nrm = normal.astype(np.float64)
        P = P.astype(np.float64)
        miss = prim < 0
        i_n = np.float64(f32(1.0) / (f32(sigma_normal) * f32(sigma_normal)))
        i_p = np.float64(f32(1.0) / (f32(sigma_plane) * f32(sigma_plane)))
        masked = np.zeros((H, W), bool) if masked is None else masked
        cfin = np.isfinite(c).all(-1)
        marked = _near_overflow(c).any(-1)
        if var0 is None:
            v = spatial_variance(c, nrm, P, miss, i_n, i_p, cfin & ~masked)
        else:
            v = var0.astype(np.float64)
        marked |= _near_overflow(v)
        overflow = marked.copy()
        for level in range(iterations):
            s = 1 << level
            vfin = np.isfinite(v) & ~masked
            rs = sigma_pass(v, np.isfinite(v), sigma_lum)  # (a masked pixel's own v0 is finite: it counts here)
            centre_ok = cfin & np.isfinite(v)
            lc = lum(np.where(cfin[..., None], c, 0.0))
            sum_w = np.zeros((H, W))
            sum_c = np.zeros((H, W, 3))
            sum_v = np.zeros((H, W))
            new_marked = marked.copy()
            new_overflow = overflow.copy()
            for dy in range(-2, 3):
                oy = dy * s
                if abs(oy) >= H:
                    continue
                for dx in range(-2, 3):
                    ox = dx * s
                    if abs(ox) >= W:
                        continue
                    p, q = _shift(H, W, oy, ox)
                    h = K[abs(dy)] * K[abs(dx)]
                    ec = np.abs(lc[q] - lc[p]) * rs[p]
                    en, ex = _geom(nrm, P, p, q, i_n, i_p)
                    e = (ec + en) + ex
                    # a tap with a non-finite colour has e = inf or NaN in the library: never counted
                    ok = (miss[q] == miss[p]) & vfin[q] & cfin[q] & (e >= 0) & (e <= EXP_CUT)
                    w = np.where(ok, h * np.exp(-np.where(ok, e, 0.0)), 0.0)
                    near = (miss[q] == miss[p]) & vfin[q] & cfin[q] & (np.abs(e - EXP_CUT) <= BAND * EXP_CUT)
                    new_marked[p] |= near
                    new_overflow[p] |= ok & overflow[q]
                    sum_w[p] += w
                    sum_c[p] += w[..., None] * np.where(ok[..., None], c[q], 0.0)
                    sum_v[p] += (w * w) * np.where(ok, v[q], 0.0)
            upd = centre_ok & (sum_w > 0)
            sw = np.where(upd, sum_w, 1.0)
            c = np.where(upd[..., None], sum_c / sw[..., None], c)
            v = np.where(upd, sum_v / (sw * sw), v)
            overflow = new_overflow
            marked = new_marked | overflow
            cfin = np.isfinite(c).all(-1)
    return c, v, marked


def rel_err(got, ref, eps, keep=None):
    """max |got - ref| / (eps + |ref|) over the kept entries finite in the
    reference; the other kept ones must be the same non-finite values.  An
    entry where both are exactly 0 has no error (eps may be 0)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    keep = np.ones(ref.shape, bool) if keep is None else np.broadcast_to(keep, ref.shape)
    fin = np.isfinite(ref) & keep
    bad = ~np.isfinite(ref) & keep
    assert np.array_equal(got[bad], ref[bad], equal_nan=True), "non-finite entries differ"
    d = np.abs(got[fin] - ref[fin])
    den = eps + np.abs(ref[fin])
    nz = d > 0
    assert (den[nz] > 0).all(), "a difference from an exactly zero reference"
    return float(np.max(d[nz] / den[nz])) if nz.any() else 0.0
