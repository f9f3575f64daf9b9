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
//
// Level 0 of a call on the accumulation reads c_q = inv * frameSum_q; in the
// non-uniform state (L.cnt non-null) c_q = c0_q with the pixel's own count
// (rt_atrous.h).
#pragma once
#include "rt_atrous.h"

namespace {

// the centre and the sums of one pixel; operator() is steps 4-10 of one tap
struct DnTap {
    const rt_dn_uniform& L;
    f3 cp, np, Pp;
    float w;
    f3 c;
    RT_HD void operator()(float h, float4 cq, f3 nq, f3 Pq) {
        const f3 dc = sub(mk(cq.x, cq.y, cq.z), cp);
        const float ec = dot(dc, dc) * L.ic;
        float en, ex;
        at_geom(L.f, np, Pp, nq, Pq, en, ex);
        const float e = (ec + en) + ex;
        if (!(e >= 0.0f)) return;
        const float wt = h * exp_nn(-e);
        if (!(wt > 0.0f)) return;
        w = w + wt;
        c.x = c.x + wt * cq.x;
        c.y = c.y + wt * cq.y;
        c.z = c.z + wt * cq.z;
    }
};

// The filtered colour of pixel (x, y) (fetch: rt_atrous.h)
template <class Fetch>
RT_HD f3 dn_pixel(const rt_dn_uniform& L, int x, int y, const Fetch& fetch) {
    float4 cp, ap, bp;
    fetch(0, 0, x, y, cp, ap, bp);
    DnTap t{L, mk(cp.x, cp.y, cp.z), mk(ap.x, ap.y, ap.z), mk(bp.x, bp.y, bp.z), 0.0f, mk(0.0f, 0.0f, 0.0f)};
    at_walk(L.f, x, y, rt_f2i(ap.w) < 0, fetch, t);
    if (t.w > 0.0f) return mk(rt_div(t.c.x, t.w), rt_div(t.c.y, t.w), rt_div(t.c.z, t.w));
    return t.cp;
}

// the filter as rt_atrous.h takes it; FIRST: level 0 of a call without a source
// colour reads inv * frameSum
template <bool FIRST>
struct DnFilter {
    using Args = rt_dn_uniform;
    static RT_HD float4 texel(const rt_dn_uniform& L, long q) {
        if (!FIRST) return L.f.src[q];  // (.w: not read; rt_temporal's source carries the history length there)
        const f3 c = at_c0(L.f, q);
        return make_float4(c.x, c.y, c.z, 0.0f);
    }
    template <class Fetch>
    static RT_HD void run(const rt_dn_uniform& L, int x, int y, const Fetch& fetch) {
        const f3 c = dn_pixel(L, x, y, fetch);
        at_store(L.f, (long)y * L.f.width + x, make_float4(c.x, c.y, c.z, 0.0f));
    }
};

// Level 0 (and the conversion pass) in the non-uniform state: the colour of
// every pixel, centre or tap, is its own mean c0_q (rt_atrous.h at_c0_cnt);
// everything behind the colour word is DnFilter's.  The later levels read
// colour buffers: DnFilter<false> as ever.
struct DnFilterCnt {
    using Args = rt_dn_level;
    static RT_HD float4 texel(const rt_dn_level& L, long q) {
        const f3 c = at_c0_cnt(L.f.accum, (long)L.f.width * L.f.height, L.cnt, q);
        return make_float4(c.x, c.y, c.z, 0.0f);
    }
    template <class Fetch>
    static RT_HD void run(const rt_dn_level& L, int x, int y, const Fetch& fetch) {
        DnFilter<true>::run(L, x, y, fetch);
    }
};

}  // namespace
