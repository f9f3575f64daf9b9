// rt_denoise.h — the edge-avoiding a-trous filter (Dammertz et al. 2010, with a
// plane-distance term for their position term and one exponential per tap),
// shared by the HIP filter kernels (rt_denoise.hip, device pass) and the CPU
// backend (rt_cpu.cpp, host pass).  Like rt_path.h every function is written
// once and every float operation is one rounding in a fixed order (both passes
// built with -ffp-contract=off), so the two backends agree bit for bit.
//
// One level, step s = 1 << i, for pixel p = (x, y); sums start at 0; taps
// dy = -2..2 (outer), dx = -2..2 (inner) at q = (x + dx s, y + dy s):
//   skip q outside the image; skip when exactly one of p, q is a miss;
//   h  = k[|dy|] k[|dx|],  k = {3/8, 1/4, 1/16};
//   ec = dot(c_q - c_p, c_q - c_p) ic;   en = dot(n_q - n_p, n_q - n_p) in;
//   pd = dot(n_p, P_q - P_p);            ex = (pd pd) ip;
//   e  = (ec + en) + ex;   skip unless e >= 0 (drops NaN);
//   w  = h exp_nn(-e);     skip unless w > 0 (a tap of weight 0 adds nothing
//        to finite sums, but 0 * inf would turn a neighbour of an infinite
//        pixel into NaN);
//   sum_w += w;  sum_c += w c_q.
// Result sum_c / sum_w when sum_w > 0, else c_p (a non-finite centre passes
// through unchanged).
#pragma once
#include "rt_path.h"

namespace {

template <bool FIRST>
RT_HD f3 dn_color(const rt_dn_level& L, long q) {
    if (FIRST) {
        const long npix = (long)L.width * L.height;
        return mk(L.inv * L.accum[q], L.inv * L.accum[npix + q], L.inv * L.accum[2 * npix + q]);
    }
    const float4 c = L.src[q];
    return mk(c.x, c.y, c.z);
}

struct DnSums {
    float w;
    f3 c;
};

// steps 4-10 of one tap
RT_HD void dn_tap(const rt_dn_level& L, float h, f3 cp, f3 np, f3 Pp, f3 cq, f3 nq, f3 Pq, DnSums& s) {
    const f3 dc = sub(cq, cp);
    const float ec = dot(dc, dc) * L.ic;
    const f3 dn = sub(nq, np);
    const float en = dot(dn, dn) * L.in;
    const float pd = dot(np, sub(Pq, Pp));
    const float ex = (pd * pd) * L.ip;
    const float e = (ec + en) + ex;
    if (!(e >= 0.0f)) return;
    const float w = h * exp_nn(-e);
    if (!(w > 0.0f)) return;
    s.w = s.w + w;
    s.c.x = s.c.x + w * cq.x;
    s.c.y = s.c.y + w * cq.y;
    s.c.z = s.c.z + w * cq.z;
}

RT_HD float dn_k(int o) {  // B3 spline {1/16, 1/4, 3/8, 1/4, 1/16}
    const int a = o < 0 ? -o : o;
    return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f;
}

// The filtered colour of pixel (x, y).  fetch(dx, dy, qx, qy, c, a, b) gives
// the colour and the two guide words of the in-image tap (qx, qy) = (x + dx s,
// y + dy s): from global memory (direct kernel, CPU) or from an LDS tile.
template <class Fetch>
RT_HD f3 dn_pixel(const rt_dn_level& L, int x, int y, const Fetch& fetch) {
    f3 cp;
    float4 ap, bp;
    fetch(0, 0, x, y, cp, ap, bp);
    const f3 np = mk(ap.x, ap.y, ap.z), Pp = mk(bp.x, bp.y, bp.z);
    const bool missp = rt_f2i(ap.w) < 0;
    DnSums s;
    s.w = 0.0f;
    s.c = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * L.step;
        if (qy < 0 || qy >= L.height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * L.step;
            if (qx < 0 || qx >= L.width) continue;
            f3 cq;
            float4 aq, bq;
            fetch(dx, dy, qx, qy, cq, aq, bq);
            if ((rt_f2i(aq.w) < 0) != missp) continue;
            dn_tap(L, dn_k(dy) * dn_k(dx), cp, np, Pp, cq, mk(aq.x, aq.y, aq.z), mk(bq.x, bq.y, bq.z), s);
        }
    }
    if (s.w > 0.0f) return mk(rt_div(s.c.x, s.w), rt_div(s.c.y, s.w), rt_div(s.c.z, s.w));
    return cp;
}

// taps straight from the frame's buffers
template <bool FIRST>
struct DnGlobalFetch {
    const rt_dn_level& L;
    RT_HD void operator()(int, int, int qx, int qy, f3& c, float4& a, float4& b) const {
        const long q = (long)qy * L.width + qx;
        a = L.ga[q];
        b = L.gb[q];
        c = dn_color<FIRST>(L, q);
    }
};

RT_HD void dn_store(const rt_dn_level& L, long p, f3 c) {
    L.dst[p] = make_float4(c.x, c.y, c.z, 0.0f);
    if (L.last && L.rgba) L.rgba[p] = tone_map(c.x, c.y, c.z, 1u);
}

}  // namespace
