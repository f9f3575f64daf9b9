// rt_temporal.h — temporal reprojection of the accumulated radiance across a
// camera move (the temporal stage of SVGF, Schied et al. 2017, without its
// variance estimate), shared by the HIP kernel (rt_temporal.hip, device pass)
// and the CPU backend (rt_cpu.cpp, host pass).  Like rt_denoise.h every
// function is written once and every float operation is one rounding in a fixed
// order (both passes built with -ffp-contract=off), so the two backends agree
// bit for bit.
//
// Pixel p = (x, y) of the current view, n frames accumulated, inv = 1 / n:
//   c_new = inv * frameSum(p);  out = c_new, len_out = n  (the no-history result)
//   unless: a history exists, p is a hit (prim >= 0), c_new is finite:
//   w = P_p - o';  v = R'^T w  (v.x = (rot'[0] w.x + rot'[3] w.y) + rot'[6] w.z,
//       columns 1, 2 for v.y, v.z);   require v.z * screen_z' > 0;
//   k = screen_z' / v.z;  fx = v.x k + (float)(W / 2);  fy = v.y k + (float)(H / 2)
//       (the inverse of primary_dir);  require fx, fy finite, -1 <= fx < W,
//       -1 <= fy < H;   x0 = floor(fx), ax = fx - x0; y0, ay likewise;
//   taps q = (x0 + i, y0 + j), j = 0, 1 (outer), i = 0, 1 (inner),
//       b = (i ? ax : 1 - ax) * (j ? ay : 1 - ay); a tap counts when q is in the
//       image, b > 0, prim_q == prim_p, dot(n_p, n_q) >= normal_cos_min,
//       |dot(n_p, P_q - P_p)| <= plane_tol * depth_p, the history colour at q
//       is finite and len_q > 0:   sw += b;  sc += b h_q;  sl += b len_q;
//   with sw > 0:  hist = sc / sw;  len_h = fminf(sl / sw, max_history);
//       a = n / (len_h + n);  out = hist + a (c_new - hist);  len_out = len_h + n.
// Stored: pending colour {out, len_out}, a copy of the two guide words, and
// (optionally) tone_map(out, 1).
//
// Non-uniform state (T.cnt non-null, cnt[p] = {n_p, J_p}; rt_render_adaptive):
// n and inv above are the pixel's own, n = (float)n_p, inv = rt_div(1, n), so
// c_new is the pixel's mean (rt_atrous.h), len_out = n_p without usable history
// and a = n_p / (len_h + n_p), len_out = len_h + n_p with one.  A history the
// pass leaves then carries per-pixel lengths; nothing else changes.
#pragma once
#include "rt_atrous.h"

namespace {

struct TpOut {
    f3 c;
    float len;
};

// The reprojected colour of pixel p = y * width + x whose guide words are a, b
// and which holds n frames (inv = 1 / n)
RT_HD TpOut tp_pixel(const rt_tp_uniform& T, int x, int y, long p, float4 a, float4 b, float n, float inv) {
    TpOut o;
    o.c = at_c0(T.accum, (long)T.width * T.height, inv, p);
    o.len = n;
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
    float sw = 0.0f, sl = 0.0f;
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
        }
    }
    if (!(sw > 0.0f)) return o;
    const f3 hist = mk(rt_div(sc.x, sw), rt_div(sc.y, sw), rt_div(sc.z, sw));
    const float len_h = fminf(rt_div(sl, sw), T.max_history);
    const float al = rt_div(n, len_h + n);
    o.c = mk(hist.x + al * (o.c.x - hist.x), hist.y + al * (o.c.y - hist.y), hist.z + al * (o.c.z - hist.z));
    o.len = len_h + n;
    return o;
}

// One pixel of the pass: reproject, then store the pending history of the
// current view (colour + length, the guide copy) and the RGBA
RT_HD void tp_run_pixel(const rt_tp_uniform& T, int x, int y, float n, float inv) {
    const long p = (long)y * T.width + x;
    const float4 a = T.ga[p], b = T.gb[p];
    const TpOut o = tp_pixel(T, x, y, p, a, b, n, inv);
    T.p_col[p] = make_float4(o.c.x, o.c.y, o.c.z, o.len);
    T.p_ga[p] = a;
    T.p_gb[p] = b;
    if (T.rgba) T.rgba[p] = tone_map(o.c.x, o.c.y, o.c.z, 1u);
}
RT_HD void tp_run_pixel(const rt_tp_uniform& T, int x, int y) { tp_run_pixel(T, x, y, T.n, T.inv); }
// the same in the non-uniform state: the pixel's own count
RT_HD void tp_run_pixel_cnt(const rt_tp_args& T, int x, int y) {
    const float nf = (float)T.cnt[(long)y * T.width + x].x;
    tp_run_pixel(T, x, y, nf, rt_div(1.0f, nf));
}

}  // namespace
