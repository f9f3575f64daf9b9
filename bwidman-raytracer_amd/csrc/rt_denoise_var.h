// rt_denoise_var.h — the variance-guided a-trous filter (the spatial stage of
// SVGF, Schied et al. 2017), shared by the HIP kernels (rt_denoise_var.hip,
// device pass) and the CPU backend (rt_cpu.cpp, host pass).  Like rt_denoise.h
// every function is written once and every float operation is one rounding in
// a fixed order (both passes built with -ffp-contract=off), so the two backends
// agree bit for bit.
//
// The colour buffers hold {c.xyz, v}: v is the variance of the pixel's mean
// luminance lum(c) = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z.  "finite" means
// neither NaN nor +-inf.
//
// Input stage: c0 = inv * frameSum.  Tracked (moment tracking live with at
// least min_batches batches): v0 = M2 rd, rd = 1 / ((J - 1) n).  Spatial
// (otherwise): over the 7 x 7 unit-step window around p, dy outer, dx inner,
// skipping q outside the image, of the other hit / miss class or with a
// non-finite colour channel:
//   wn = exp_nn(-(en + ex))   en, ex as rt_denoise.h forms them
//   l = lum(c_q);  s0 += wn;  s1 += wn l;  s2 += wn (l l)
// v0 = fmaxf(s2 / s0 - m1 m1, 0), m1 = s1 / s0; 0 unless s0 > 0.
//
// Sigma pass, before every level: g = the 3 x 3 unit-step Gaussian of v (1/4
// centre, 1/8 edges, 1/16 corners; dy outer, dx inner) over the in-image taps
// with finite v, divided by the sum of their weights;
//   rs = 1 / (sigma_lum sqrt(g) + 1e-10)
// (correctly rounded sqrt and division); 0 for a pixel without a finite tap.
//
// Level i, step s = 1 << i: taps and h as rt_denoise.h; a tap is skipped under
// its rules (outside, other hit / miss class) and when v_q is not finite;
//   ec = |lum(c_q) - lum(c_p)| rs(p);   e = (ec + en) + ex;
//   skip unless e >= 0;  w = h exp_nn(-e);  skip unless w > 0;
//   sum_w += w;  sum_c += w c_q;  sum_v += (w w) v_q.
// Result c' = sum_c / sum_w, v' = sum_v / (sum_w sum_w).  A centre with a
// non-finite colour channel or variance, and a pixel with sum_w not > 0, pass
// through unchanged.
#pragma once
#include "rt_denoise.h"
#include "rt_moments.h"

namespace {

RT_HD bool dv_finite(float x) { return (rt_f2i(x) & 0x7f800000) != 0x7f800000; }

RT_HD f3 dv_c0(const rt_dv_args& A, long q) {
    const long npix = (long)A.width * A.height;
    return mk(A.inv * A.accum[q], A.inv * A.accum[npix + q], A.inv * A.accum[2 * npix + q]);
}

// the geometry terms en, ex of a tap, as rt_denoise.h dn_tap
RT_HD void dv_geom(const rt_dv_args& A, f3 np, f3 Pp, f3 nq, f3 Pq, float& en, float& ex) {
    const f3 dn = sub(nq, np);
    en = dot(dn, dn) * A.in;
    const float pd = dot(np, sub(Pq, Pp));
    ex = (pd * pd) * A.ip;
}

// Input stage of pixel p = (x, y): {c0, v0}
RT_HD float4 dv_input(const rt_dv_args& A, int x, int y) {
    const long p = (long)y * A.width + x;
    const f3 c = dv_c0(A, p);
    if (A.tracked) return make_float4(c.x, c.y, c.z, A.mom[p].y * A.rd);
    const float4 ap = A.ga[p], bp = A.gb[p];
    const f3 np = mk(ap.x, ap.y, ap.z), Pp = mk(bp.x, bp.y, bp.z);
    const bool missp = rt_f2i(ap.w) < 0;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -3; dy <= 3; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= A.height) continue;
        for (int dx = -3; dx <= 3; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= A.width) continue;
            const long q = (long)qy * A.width + qx;
            const float4 aq = A.ga[q];
            if ((rt_f2i(aq.w) < 0) != missp) continue;
            const f3 cq = dv_c0(A, q);
            if (!dv_finite(cq.x) || !dv_finite(cq.y) || !dv_finite(cq.z)) continue;
            const float4 bq = A.gb[q];
            float en, ex;
            dv_geom(A, np, Pp, mk(aq.x, aq.y, aq.z), mk(bq.x, bq.y, bq.z), en, ex);
            const float wn = exp_nn(-(en + ex));
            const float l = mom_lum(cq.x, cq.y, cq.z);
            s0 = s0 + wn;
            s1 = s1 + wn * l;
            s2 = s2 + wn * (l * l);
        }
    }
    float v = 0.0f;
    if (s0 > 0.0f) {
        const float m1 = rt_div(s1, s0);
        v = fmaxf(rt_div(s2, s0) - m1 * m1, 0.0f);
    }
    return make_float4(c.x, c.y, c.z, v);
}

RT_HD void dv_store(const rt_dv_args& A, long p, float4 c) {
    A.dst[p] = c;
    if (A.last && A.rgba) A.rgba[p] = tone_map(c.x, c.y, c.z, 1u);
}

// Sigma pass of pixel (x, y): the reciprocal luminance sigma from A.src's .w
RT_HD float dv_sigma(const rt_dv_args& A, int x, int y) {
    float sv = 0.0f, sw = 0.0f;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= A.height) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= A.width) continue;
            const float v = A.src[(long)qy * A.width + qx].w;
            if (!dv_finite(v)) continue;
            const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            sv = sv + k * v;
            sw = sw + k;
        }
    }
    if (!(sw > 0.0f)) return 0.0f;
    const float g = rt_div(sv, sw);
    return rt_div(1.0f, A.sigma_lum * rt_sqrt(g) + 1e-10f);
}

// The filtered {colour, variance} of pixel (x, y).  fetch(dx, dy, qx, qy, c, a,
// b) gives the colour + variance and the two guide words of the in-image tap
// (qx, qy) = (x + dx s, y + dy s): from global memory (direct kernel, CPU) or
// from an LDS tile.
template <class Fetch>
RT_HD float4 dv_pixel(const rt_dv_args& A, int x, int y, const Fetch& fetch) {
    float4 cp, ap, bp;
    fetch(0, 0, x, y, cp, ap, bp);
    if (!dv_finite(cp.x) || !dv_finite(cp.y) || !dv_finite(cp.z) || !dv_finite(cp.w)) return cp;
    const float rs = A.rs[(long)y * A.width + x];
    const f3 np = mk(ap.x, ap.y, ap.z), Pp = mk(bp.x, bp.y, bp.z);
    const bool missp = rt_f2i(ap.w) < 0;
    const float lp = mom_lum(cp.x, cp.y, cp.z);
    float sw = 0.0f, sv = 0.0f;
    f3 sc = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * A.step;
        if (qy < 0 || qy >= A.height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * A.step;
            if (qx < 0 || qx >= A.width) continue;
            float4 cq, aq, bq;
            fetch(dx, dy, qx, qy, cq, aq, bq);
            if ((rt_f2i(aq.w) < 0) != missp) continue;
            if (!dv_finite(cq.w)) continue;
            const float ec = fabsf(mom_lum(cq.x, cq.y, cq.z) - lp) * rs;
            float en, ex;
            dv_geom(A, np, Pp, mk(aq.x, aq.y, aq.z), mk(bq.x, bq.y, bq.z), en, ex);
            const float e = (ec + en) + ex;
            if (!(e >= 0.0f)) continue;
            const float w = (dn_k(dy) * dn_k(dx)) * exp_nn(-e);
            if (!(w > 0.0f)) continue;
            sw = sw + w;
            sc.x = sc.x + w * cq.x;
            sc.y = sc.y + w * cq.y;
            sc.z = sc.z + w * cq.z;
            sv = sv + (w * w) * cq.w;
        }
    }
    if (!(sw > 0.0f)) return cp;
    return make_float4(rt_div(sc.x, sw), rt_div(sc.y, sw), rt_div(sc.z, sw), rt_div(sv, sw * sw));
}

// taps straight from the frame's buffers
struct DvGlobalFetch {
    const rt_dv_args& A;
    RT_HD void operator()(int, int, int qx, int qy, float4& c, float4& a, float4& b) const {
        const long q = (long)qy * A.width + qx;
        a = A.ga[q];
        b = A.gb[q];
        c = A.src[q];
    }
};

}  // namespace
