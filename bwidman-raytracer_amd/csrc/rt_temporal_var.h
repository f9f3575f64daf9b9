// rt_temporal_var.h — temporal reprojection that also carries a per-pixel
// estimate of the luminance variance across a camera move (the temporal stage
// of SVGF, Schied et al. 2017, with its variance estimate), shared by the HIP
// kernels (rt_temporal_var.hip, device pass) and the CPU backend (rt_cpu.cpp,
// host pass).  Like rt_temporal.h every function is written once and every
// float operation is one rounding in a fixed order (both passes built with
// -ffp-contract=off), so the two backends agree bit for bit.
//
// State beside rt_temporal.h's {out.rgb, len} and guide copy: one float2 plane
// {s2, dof} per history set.  s2 is the pooled estimate of the PER-FRAME
// luminance variance of the pixel, dof its degrees of freedom; the variance of
// the pixel's mean luminance is s2 / len.
//
// Colour and length: c_new, the projection, the four taps, their acceptance
// tests, hist, len_h, a, out and len_out are rt_temporal.h's tp_pixel, the same
// operations in the same order (tv_pixel holds a copy of its tap loop, so
// rt_temporal's kernels keep their instructions; test_temporal_var.py pins the
// two to equal bits).
//
// Tap sums: every accepted tap q also adds ss += b s2_q, sd += b dof_q.  A tap
// whose s2_q or dof_q is not finite or whose dof_q < 0 adds 0 to both and still
// counts for colour; so does every tap of a history set that plain rt_temporal
// wrote (it has no moment plane).  Such a tap's weight STAYS in the divisor sw:
// the tap is a history sample about whose spread nothing is known, exactly like
// a tap of a plane-less set, so it lowers dof_h in proportion to its weight
// instead of handing its share of the history to the other taps' estimate.
//
// Current view: l_c = lum(c_new); tracked (the frame's moments are current, J >=
// 2 batches): dof_c = (float)(J - 1), s2_c = M2_p / dof_c; else dof_c = s2_c = 0.
// No usable history (any of tp_pixel's exits): s2_out = s2_c, dof_out = dof_c.
// With history (sw > 0):
//   s2_h = ss / sw;   dof_h = fminf(sd / sw, len_h);   l_h = lum(hist)
//   between = rt_div(len_h n, len_h + n) ((l_c - l_h) (l_c - l_h))
//   dof_out = (dof_h + dof_c) + 1
//   s2_out = rt_div((dof_h s2_h + dof_c s2_c) + between, dof_out)
// the pairwise (Chan) merge of two weighted-Welford accumulators: `between` has
// expectation sigma^2 when both means estimate the same value.
// Stored: rt_temporal.h's, and the pending {s2_out, dof_out}.
//
// Non-uniform frame (rt_temporal_var_counted; cnt[p] = {n_p, J_p}, n_p >= 1):
// section 21's operator with section 15's substitutions.  nf_p = (float)n_p,
// inv_p = rt_div(1.0f, nf_p), c_new = inv_p * frameSum_p (at_c0_cnt); wherever the
// text above writes n it is nf_p: a = rt_div(nf_p, len_h + nf_p), len_out = nf_p
// without usable history and len_h + nf_p with one, between = rt_div(len_h nf_p,
// len_h + nf_p) (dl dl).  Current view, per pixel: where the frame carries moments
// (the accumulation's tracking is current, or a 7-plane counted assembled frame;
// a 4-plane one has none) and J_p >= 2: dof_c = (float)(J_p - 1), s2_c =
// rt_div(M2_p, dof_c); else both 0.  M2_p / (J_p - 1) is the per-frame variance
// whatever n_p is (ad_var is that value over n_p).  Merge, tap sums, stored planes
// and moments_out are unchanged; colour, length and RGBA are rt_temporal's
// count-aware ones bit for bit; with all counts equal every expression is the
// uniform one.  A pixel with J_p = 1 (rt_render_adaptive_reprojected from a
// one-batch base left it unselected) brings no within-view term, like an
// untracked frame's.
//
// Input stage of the variance-guided levels behind the pass (rt_denoise_var.h's
// sigma pass and levels follow unchanged): {out.xyz, v0} per pixel, with
//   temporal (dof_out >= dof_min = (float)min_batches - 1.5f): v0 = rt_div(s2_out, len_out)
//   spatial (otherwise): dv_spatial over the pending colours.
#pragma once
#include "rt_denoise_var.h"
#include "rt_temporal.h"

namespace {

// One 8-byte load of a {float, float} pair.  The members of a float2 are used
// behind different tests, and the compiler then fetches them with one 4-byte
// load each; through a 64-bit word it is one global_load_dwordx2 (the bits are
// the floats' own: little-endian on both backends).
RT_HD float2 tv_load2(const float2* p) {
    unsigned long long u;
    __builtin_memcpy(&u, p, sizeof u);
    return make_float2(rt_i2f((int)(unsigned)(u & 0xffffffffull)), rt_i2f((int)(unsigned)(u >> 32)));
}

struct TvOut {
    f3 c;
    float len, s2, dof;
};

// The reprojected colour, length and moments of pixel p = y * width + x whose
// guide words are a, b (uniform accumulation: n = T.n frames, inv = T.inv)
RT_HD TvOut tv_pixel(const rt_tv_args& V, int x, int y, long p, float4 a, float4 b) {
    const rt_tp_uniform& T = V.t;
    const float n = T.n;
    TvOut o;
    o.c = at_c0(T.accum, (long)T.width * T.height, T.inv, p);
    o.len = n;
    o.s2 = 0.0f;
    o.dof = V.dof_c;
    if (V.tracked) o.s2 = rt_div(tv_load2(V.mom + p).y, V.dof_c);
    const int prim = rt_f2i(a.w);
    if (!T.has_history || prim < 0) return o;
    if (!(at_finite(o.c.x) && at_finite(o.c.y) && at_finite(o.c.z))) return o;
    const f3 np = mk(a.x, a.y, a.z), Pp = mk(b.x, b.y, b.z);
    const f3 w = sub(Pp, mk(T.h_cam[0], T.h_cam[1], T.h_cam[2]));
    const float vx = T.h_rot[0] * w.x + T.h_rot[3] * w.y + T.h_rot[6] * w.z;
    const float vy = T.h_rot[1] * w.x + T.h_rot[4] * w.y + T.h_rot[7] * w.z;
    const float vz = T.h_rot[2] * w.x + T.h_rot[5] * w.y + T.h_rot[8] * w.z;
    if (!(vz * T.h_screen_z > 0.0f)) return o;  // behind the history camera (or NaN)
    const float k = rt_div(T.h_screen_z, vz);
    const float fx = vx * k + (float)(T.width / 2);
    const float fy = vy * k + (float)(T.height / 2);
    if (!(at_finite(fx) && at_finite(fy))) return o;
    if (!(fx >= -1.0f && fx < (float)T.width && fy >= -1.0f && fy < (float)T.height)) return o;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float ax = fx - x0f, ay = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float tol = T.plane_tol * b.w;
    float sw = 0.0f, sl = 0.0f, ss = 0.0f, sd = 0.0f;
    f3 sc = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int qy = y0 + j;
        if (qy < 0 || qy >= T.height) continue;
        const float by = j ? ay : 1.0f - ay;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int qx = x0 + i;
            if (qx < 0 || qx >= T.width) continue;
            const float bw = (i ? ax : 1.0f - ax) * by;
            if (!(bw > 0.0f)) continue;
            const long q = (long)qy * T.width + qx;
            const float4 aq = T.h_ga[q];
            if (rt_f2i(aq.w) != prim) continue;
            if (!(dot(np, mk(aq.x, aq.y, aq.z)) >= T.normal_cos_min)) continue;
            const float4 bq = T.h_gb[q];
            if (!(fabsf(dot(np, sub(mk(bq.x, bq.y, bq.z), Pp))) <= tol)) continue;
            const float4 hq = T.h_col[q];
            if (!(at_finite(hq.x) && at_finite(hq.y) && at_finite(hq.z) && hq.w > 0.0f)) continue;
            sw = sw + bw;
            sc.x = sc.x + bw * hq.x;
            sc.y = sc.y + bw * hq.y;
            sc.z = sc.z + bw * hq.z;
            sl = sl + bw * hq.w;
            if (V.h_mom) {
                const float2 mq = tv_load2(V.h_mom + q);
                if (at_finite(mq.x) && at_finite(mq.y) && mq.y >= 0.0f) {
                    ss = ss + bw * mq.x;
                    sd = sd + bw * mq.y;
                }
            }
        }
    }
    if (!(sw > 0.0f)) return o;
    const f3 hist = mk(rt_div(sc.x, sw), rt_div(sc.y, sw), rt_div(sc.z, sw));
    const float len_h = fminf(rt_div(sl, sw), T.max_history);
    const float al = rt_div(n, len_h + n);
    const float l_c = mom_lum(o.c.x, o.c.y, o.c.z);
    o.c = mk(hist.x + al * (o.c.x - hist.x), hist.y + al * (o.c.y - hist.y), hist.z + al * (o.c.z - hist.z));
    o.len = len_h + n;
    const float s2_h = rt_div(ss, sw);
    const float dof_h = fminf(rt_div(sd, sw), len_h);
    const float dl = l_c - mom_lum(hist.x, hist.y, hist.z);
    const float between = rt_div(len_h * n, len_h + n) * (dl * dl);
    o.dof = (dof_h + V.dof_c) + 1.0f;
    o.s2 = rt_div((dof_h * s2_h + V.dof_c * o.s2) + between, o.dof);
    return o;
}

// One pixel of the pass: reproject, then store the pending history of the
// current view (colour + length, moments, the guide copy) and the RGBA
RT_HD void tv_run_pixel(const rt_tv_args& V, int x, int y) {
    const rt_tp_uniform& T = V.t;
    const long p = (long)y * T.width + x;
    const float4 a = T.ga[p], b = T.gb[p];
    const TvOut o = tv_pixel(V, x, y, p, a, b);
    T.p_col[p] = make_float4(o.c.x, o.c.y, o.c.z, o.len);
    V.p_mom[p] = make_float2(o.s2, o.dof);
    T.p_ga[p] = a;
    T.p_gb[p] = b;
    if (T.rgba) T.rgba[p] = tone_map(o.c.x, o.c.y, o.c.z, 1u);
}

// tv_pixel on a non-uniform frame: n, inv and dof_c are the pixel's own, from
// cnt[p] = {n_p, J_p} (a copy, like tv_pixel's of tp_pixel's tap loop, so the
// uniform kernel keeps its instructions; test_adaptive_temporal.py pins the two
// to equal bits on equal counts)
RT_HD TvOut tv_pixel_cnt(const rt_tv_cnt_args& V, int x, int y, long p, float4 a, float4 b) {
    const rt_tp_uniform& T = V.t;
    const uint2 cn = V.cnt[p];
    const float n = (float)cn.x, inv = rt_div(1.0f, n);
    const bool tracked = V.tracked && cn.y >= 2u;
    const float dof_c = tracked ? (float)(cn.y - 1u) : 0.0f;
    TvOut o;
    o.c = at_c0(T.accum, (long)T.width * T.height, inv, p);
    o.len = n;
    o.s2 = 0.0f;
    o.dof = dof_c;
    if (tracked) o.s2 = rt_div(tv_load2(V.mom + p).y, dof_c);
    const int prim = rt_f2i(a.w);
    if (!T.has_history || prim < 0) return o;
    if (!(at_finite(o.c.x) && at_finite(o.c.y) && at_finite(o.c.z))) return o;
    const f3 np = mk(a.x, a.y, a.z), Pp = mk(b.x, b.y, b.z);
    const f3 w = sub(Pp, mk(T.h_cam[0], T.h_cam[1], T.h_cam[2]));
    const float vx = T.h_rot[0] * w.x + T.h_rot[3] * w.y + T.h_rot[6] * w.z;
    const float vy = T.h_rot[1] * w.x + T.h_rot[4] * w.y + T.h_rot[7] * w.z;
    const float vz = T.h_rot[2] * w.x + T.h_rot[5] * w.y + T.h_rot[8] * w.z;
    if (!(vz * T.h_screen_z > 0.0f)) return o;  // behind the history camera (or NaN)
    const float k = rt_div(T.h_screen_z, vz);
    const float fx = vx * k + (float)(T.width / 2);
    const float fy = vy * k + (float)(T.height / 2);
    if (!(at_finite(fx) && at_finite(fy))) return o;
    if (!(fx >= -1.0f && fx < (float)T.width && fy >= -1.0f && fy < (float)T.height)) return o;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float ax = fx - x0f, ay = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float tol = T.plane_tol * b.w;
    float sw = 0.0f, sl = 0.0f, ss = 0.0f, sd = 0.0f;
    f3 sc = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int qy = y0 + j;
        if (qy < 0 || qy >= T.height) continue;
        const float by = j ? ay : 1.0f - ay;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int qx = x0 + i;
            if (qx < 0 || qx >= T.width) continue;
            const float bw = (i ? ax : 1.0f - ax) * by;
            if (!(bw > 0.0f)) continue;
            const long q = (long)qy * T.width + qx;
            const float4 aq = T.h_ga[q];
            if (rt_f2i(aq.w) != prim) continue;
            if (!(dot(np, mk(aq.x, aq.y, aq.z)) >= T.normal_cos_min)) continue;
            const float4 bq = T.h_gb[q];
            if (!(fabsf(dot(np, sub(mk(bq.x, bq.y, bq.z), Pp))) <= tol)) continue;
            const float4 hq = T.h_col[q];
            if (!(at_finite(hq.x) && at_finite(hq.y) && at_finite(hq.z) && hq.w > 0.0f)) continue;
            sw = sw + bw;
            sc.x = sc.x + bw * hq.x;
            sc.y = sc.y + bw * hq.y;
            sc.z = sc.z + bw * hq.z;
            sl = sl + bw * hq.w;
            if (V.h_mom) {
                const float2 mq = tv_load2(V.h_mom + q);
                if (at_finite(mq.x) && at_finite(mq.y) && mq.y >= 0.0f) {
                    ss = ss + bw * mq.x;
                    sd = sd + bw * mq.y;
                }
            }
        }
    }
    if (!(sw > 0.0f)) return o;
    const f3 hist = mk(rt_div(sc.x, sw), rt_div(sc.y, sw), rt_div(sc.z, sw));
    const float len_h = fminf(rt_div(sl, sw), T.max_history);
    const float al = rt_div(n, len_h + n);
    const float l_c = mom_lum(o.c.x, o.c.y, o.c.z);
    o.c = mk(hist.x + al * (o.c.x - hist.x), hist.y + al * (o.c.y - hist.y), hist.z + al * (o.c.z - hist.z));
    o.len = len_h + n;
    const float s2_h = rt_div(ss, sw);
    const float dof_h = fminf(rt_div(sd, sw), len_h);
    const float dl = l_c - mom_lum(hist.x, hist.y, hist.z);
    const float between = rt_div(len_h * n, len_h + n) * (dl * dl);
    o.dof = (dof_h + dof_c) + 1.0f;
    o.s2 = rt_div((dof_h * s2_h + dof_c * o.s2) + between, o.dof);
    return o;
}

// tv_run_pixel on a non-uniform frame: the pixel's own counts
RT_HD void tv_run_pixel_cnt(const rt_tv_cnt_args& V, int x, int y) {
    const rt_tp_uniform& T = V.t;
    const long p = (long)y * T.width + x;
    const float4 a = T.ga[p], b = T.gb[p];
    const TvOut o = tv_pixel_cnt(V, x, y, p, a, b);
    T.p_col[p] = make_float4(o.c.x, o.c.y, o.c.z, o.len);
    V.p_mom[p] = make_float2(o.s2, o.dof);
    T.p_ga[p] = a;
    T.p_gb[p] = b;
    if (T.rgba) T.rgba[p] = tone_map(o.c.x, o.c.y, o.c.z, 1u);
}

// The variance of the mean luminance that a pixel's pending state stands for:
// 0 where nothing is known (dof 0)
RT_HD float tv_var_of_mean(float2 m, float len) { return m.y > 0.0f ? rt_div(m.x, len) : 0.0f; }

// Input stage of pixel (x, y) of the levels behind the pass: {out.xyz, v0}
RT_HD float4 tv_input(const rt_tv_input& A, int x, int y) {
    const rt_at_frame& F = A.f;
    const long p = (long)y * F.width + x;
    const float4 c = A.col[p];
    const float2 m = tv_load2(A.mom + p);
    if (m.y >= A.dof_min) return make_float4(c.x, c.y, c.z, rt_div(m.x, c.w));
    return make_float4(c.x, c.y, c.z, dv_spatial(F, x, y, [&](long q) {
                           const float4 cq = A.col[q];
                           return mk(cq.x, cq.y, cq.z);
                       }));
}

}  // namespace
