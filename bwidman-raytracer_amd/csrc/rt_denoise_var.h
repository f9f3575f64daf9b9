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
//   wn = exp_nn(-(en + ex))   en, ex as rt_denoise.h forms them (rt_atrous.h at_geom)
//   l = lum(c_q);  s0 += wn;  s1 += wn l;  s2 += wn (l l)
// v0 = fmaxf(s2 / s0 - m1 m1, 0), m1 = s1 / s0; 0 unless s0 > 0.
//
// Input stage in the non-uniform state (A.cnt non-null, cnt[p] = {n_p, J_p};
// rt_render_adaptive): the moments of every pixel are current for its own n_p,
// so the choice is per pixel and one frame mixes both sources.  c0_q is the
// pixel's own mean (rt_atrous.h at_c0_cnt) for the centre and for every tap of
// the window.  Tracked (J_p >= min_batches): v0 = ad_var(M2_p, n_p, J_p)
// (rt_adaptive.h, the selection's and rt_get_variance's expression).  Spatial
// (otherwise): the estimate above over the count-aware c0_q.  With all counts
// equal both are the uniform stage's values.
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
#include "rt_adaptive.h"
#include "rt_denoise.h"
#include "rt_moments.h"

namespace {

// The spatial estimate v0 of pixel p = (x, y); c0(q) is the input colour of tap q
template <class C0>
RT_HD float dv_spatial(const rt_at_frame& F, int x, int y, const C0& c0) {
    const long p = (long)y * F.width + x;
    const float4 ap = F.ga[p], bp = F.gb[p];
    const f3 np = mk(ap.x, ap.y, ap.z), Pp = mk(bp.x, bp.y, bp.z);
    const bool missp = rt_f2i(ap.w) < 0;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -3; dy <= 3; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= F.height) continue;
        for (int dx = -3; dx <= 3; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= F.width) continue;
            const long q = (long)qy * F.width + qx;
            const float4 aq = F.ga[q];
            if ((rt_f2i(aq.w) < 0) != missp) continue;
            const f3 cq = c0(q);
            if (!at_finite(cq.x) || !at_finite(cq.y) || !at_finite(cq.z)) continue;
            const float4 bq = F.gb[q];
            float en, ex;
            at_geom(F, np, Pp, mk(aq.x, aq.y, aq.z), mk(bq.x, bq.y, bq.z), en, ex);
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
    return v;
}

// Input stage of pixel p = (x, y): {c0, v0}
RT_HD float4 dv_input(const rt_dv_uniform& A, int x, int y) {
    const rt_at_frame& F = A.f;
    const long p = (long)y * F.width + x;
    const f3 c = at_c0(F, p);
    if (A.tracked) return make_float4(c.x, c.y, c.z, A.mom[p].y * A.rd);
    return make_float4(c.x, c.y, c.z, dv_spatial(F, x, y, [&](long q) { return at_c0(F, q); }));
}

// The same in the non-uniform state: the pixel's own choice between the two
// sources, every colour with its pixel's count
RT_HD float4 dv_input_cnt(const rt_dv_args& A, int x, int y) {
    const rt_at_frame& F = A.f;
    const long npix = (long)F.width * F.height, p = (long)y * F.width + x;
    const uint2 cn = A.cnt[p];
    const f3 c = at_c0(F.accum, npix, rt_div(1.0f, (float)cn.x), p);
    if (cn.y >= A.min_batches) return make_float4(c.x, c.y, c.z, ad_var(A.mom[p].y, cn.x, cn.y));
    return make_float4(c.x, c.y, c.z, dv_spatial(F, x, y, [&](long q) { return at_c0_cnt(F.accum, npix, A.cnt, q); }));
}

// Sigma pass of pixel (x, y): the reciprocal luminance sigma from src's .w
RT_HD float dv_sigma(const rt_dv_uniform& A, int x, int y) {
    const rt_at_frame& F = A.f;
    float sv = 0.0f, sw = 0.0f;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= F.height) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= F.width) continue;
            const float v = F.src[(long)qy * F.width + qx].w;
            if (!at_finite(v)) continue;
            const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            sv = sv + k * v;
            sw = sw + k;
        }
    }
    if (!(sw > 0.0f)) return 0.0f;
    const float g = rt_div(sv, sw);
    return rt_div(1.0f, A.sigma_lum * rt_sqrt(g) + 1e-10f);
}

// the centre and the sums of one pixel of a level; operator() is one tap
struct DvTap {
    const rt_at_frame& F;
    f3 np, Pp;
    float lp, rs;
    float w, v;
    f3 c;
    RT_HD void operator()(float h, float4 cq, f3 nq, f3 Pq) {
        if (!at_finite(cq.w)) return;
        const float ec = fabsf(mom_lum(cq.x, cq.y, cq.z) - lp) * rs;
        float en, ex;
        at_geom(F, np, Pp, nq, Pq, en, ex);
        const float e = (ec + en) + ex;
        if (!(e >= 0.0f)) return;
        const float wt = h * exp_nn(-e);
        if (!(wt > 0.0f)) return;
        w = w + wt;
        c.x = c.x + wt * cq.x;
        c.y = c.y + wt * cq.y;
        c.z = c.z + wt * cq.z;
        v = v + (wt * wt) * cq.w;
    }
};

// The filtered {colour, variance} of pixel (x, y) (fetch: rt_atrous.h)
template <class Fetch>
RT_HD float4 dv_pixel(const rt_dv_uniform& A, int x, int y, const Fetch& fetch) {
    float4 cp, ap, bp;
    fetch(0, 0, x, y, cp, ap, bp);
    if (!at_finite(cp.x) || !at_finite(cp.y) || !at_finite(cp.z) || !at_finite(cp.w)) return cp;
    DvTap t{A.f, mk(ap.x, ap.y, ap.z), mk(bp.x, bp.y, bp.z), mom_lum(cp.x, cp.y, cp.z),
            A.rs[(long)y * A.f.width + x], 0.0f, 0.0f, mk(0.0f, 0.0f, 0.0f)};
    at_walk(A.f, x, y, rt_f2i(ap.w) < 0, fetch, t);
    if (!(t.w > 0.0f)) return cp;
    return make_float4(rt_div(t.c.x, t.w), rt_div(t.c.y, t.w), rt_div(t.c.z, t.w), rt_div(t.v, t.w * t.w));
}

// the filter's level as rt_atrous.h takes it
struct DvFilter {
    using Args = rt_dv_uniform;
    static RT_HD float4 texel(const rt_dv_uniform& A, long q) { return A.f.src[q]; }
    template <class Fetch>
    static RT_HD void run(const rt_dv_uniform& A, int x, int y, const Fetch& fetch) {
        at_store(A.f, (long)y * A.f.width + x, dv_pixel(A, x, y, fetch));
    }
};

}  // namespace
