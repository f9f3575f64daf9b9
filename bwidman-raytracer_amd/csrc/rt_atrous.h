// rt_atrous.h — what the post-render passes share: the arithmetic that the
// a-trous filters (rt_denoise.h, rt_denoise_var.h) and the temporal
// reprojection (rt_temporal.h) have in common, written once for the HIP
// kernels (device pass) and the CPU backend (rt_cpu.cpp, host pass).  Like
// rt_path.h every float operation is one rounding in a fixed order (both passes
// built with -ffp-contract=off), so the two backends agree bit for bit.
//
// The 5 x 5 walk of one level, step s, around pixel p = (x, y): taps dy = -2..2
// (outer), dx = -2..2 (inner) at q = (x + dx s, y + dy s); q outside the image
// is skipped, and so is q when exactly one of p, q is a miss; every other tap
// goes to the filter's tap body with h = k[|dy|] k[|dx|], k = {3/8, 1/4, 1/16}.
#pragma once
#include "rt_path.h"

namespace {

// neither NaN nor +-inf
RT_HD bool at_finite(float x) { return (rt_f2i(x) & 0x7f800000) != 0x7f800000; }

// c0 = inv * frameSum of pixel q (three planes of npix)
RT_HD f3 at_c0(const float* accum, long npix, float inv, long q) {
    return mk(inv * accum[q], inv * accum[npix + q], inv * accum[2 * npix + q]);
}
RT_HD f3 at_c0(const rt_at_frame& F, long q) { return at_c0(F.accum, (long)F.width * F.height, F.inv, q); }

// Non-uniform state (rt_render_adaptive; cnt[q] = {n_q, J_q}, every n_q >= 2):
// the input colour of every pass is pixel q's own mean,
//   inv_q = rt_div(1.0f, (float)n_q);   c0_q = inv_q * frameSum_q  per plane
// (rt_adaptive.h ad_resolve's colour), wherever the uniform passes read
// inv * frameSum of a centre or a tap.  With all n_q equal it is at_c0.
RT_HD float at_inv_cnt(const uint2* cnt, long q) { return rt_div(1.0f, (float)cnt[q].x); }
RT_HD f3 at_c0_cnt(const float* accum, long npix, const uint2* cnt, long q) {
    return at_c0(accum, npix, at_inv_cnt(cnt, q), q);
}

// the geometry terms of a tap: en = dot(n_q - n_p, n_q - n_p) in,
// ex = (pd pd) ip with pd = dot(n_p, P_q - P_p)
RT_HD void at_geom(const rt_at_frame& F, f3 np, f3 Pp, f3 nq, f3 Pq, float& en, float& ex) {
    const f3 dn = sub(nq, np);
    en = dot(dn, dn) * F.in;
    const float pd = dot(np, sub(Pq, Pp));
    ex = (pd * pd) * F.ip;
}

RT_HD float at_k(int o) {  // B3 spline {1/16, 1/4, 3/8, 1/4, 1/16}
    const int a = o < 0 ? -o : o;
    return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f;
}

RT_HD void at_store(const rt_at_frame& F, long p, float4 c) {
    F.dst[p] = c;
    if (F.last && F.rgba) F.rgba[p] = tone_map(c.x, c.y, c.z, 1u);
}

// A filter P is a small policy: P::Args (its argument struct, with the frame in
// .f), P::texel(A, q), the colour word of pixel q that a tap reads, and
// P::run(A, x, y, fetch), which filters pixel (x, y) and stores the result.
// fetch(dx, dy, qx, qy, c, a, b) gives the colour word and the two guide words
// of the in-image tap (qx, qy) = (x + dx s, y + dy s): straight from the
// frame's buffers (direct kernel, CPU), as here, or from an LDS tile
// (rt_atrous_tile.h).
template <class P>
struct AtGlobalFetch {
    const typename P::Args& A;
    const int width;  // A.f.width by value: the row offset qy * width then hoists out of the dx loop
    RT_HD void operator()(int, int, int qx, int qy, float4& c, float4& a, float4& b) const {
        const long q = (long)qy * width + qx;
        a = A.f.ga[q];
        b = A.f.gb[q];
        c = P::texel(A, q);
    }
};

// one pixel of a level with the taps from global memory
template <class P>
RT_HD void at_run_direct(const typename P::Args& A, int x, int y) {
    const AtGlobalFetch<P> fetch{A, A.f.width};
    P::run(A, x, y, fetch);
}

// The walk.  missp: the centre is a miss.  tap(h, c_q, n_q, P_q) is the
// filter's body for a tap of the centre's hit / miss class.
template <class Fetch, class Tap>
RT_HD void at_walk(const rt_at_frame& F, int x, int y, bool missp, const Fetch& fetch, Tap& tap) {
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * F.step;
        if (qy < 0 || qy >= F.height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * F.step;
            if (qx < 0 || qx >= F.width) continue;
            float4 cq, aq, bq;
            fetch(dx, dy, qx, qy, cq, aq, bq);
            if ((rt_f2i(aq.w) < 0) != missp) continue;
            tap(at_k(dy) * at_k(dx), cq, mk(aq.x, aq.y, aq.z), mk(bq.x, bq.y, bq.z));
        }
    }
}

}  // namespace
