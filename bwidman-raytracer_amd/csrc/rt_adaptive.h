// rt_adaptive.h — variance-driven adaptive sampling: the selection criterion,
// the moment update of a listed pixel and the resolve pass, shared by the HIP
// unit (rt_adaptive.hip) and the CPU backend (rt_cpu.cpp).  Every float
// operation is one rounding in the order written (both built with
// -ffp-contract=off), so GPU and CPU contexts select the same pixels and keep
// the same moments bit for bit.
//
// A context in the non-uniform state holds {n_p, J_p} per pixel: the frames
// accumulated and the moment batches tracked for that pixel.  Per pixel q
//   v_q = M2_q * rt_div(1, (float)(J_q - 1) * (float)n_q)
// estimates the variance of the pixel's mean luminance (rt_moments.h).  The
// window of p is every q with |dx|, |dy| <= radius inside the image whose v_q
// and M_q are finite; row sums first, in increasing x, then the column sum of
// the row sums in increasing y; the tap count c is an integer.  With
// sv = sum v, sm = sum M, cf = (float)c:
//   b     = tolerance * (sm + cf * lum_floor)
//   hot_p = c > 0 && (sv * cf) > (b * b)
// i.e. the root of the window-mean variance of the mean exceeds `tolerance`
// times the window-mean luminance (plus the floor), without a division.
//   selected_p = (max_frames == 0 || n_p + k <= max_frames) && (n_p < min_frames || hot_p)
//
// A selected pixel then renders k more frames (rt_kernel_list.h); its moments
// take the step of rt_moments.h with the pixel's own weight
//   kw_p = rt_div(kf, (float)(n_p + k)),
// then J_p += 1, n_p += k, prev_p = frameSum_p.
//
// Selection from the reprojected variance (rt_render_adaptive_reprojected,
// DESIGN.md section 22).  The context's pending temporal set of the current view
// (rt_temporal_var; rt_temporal_var.h) gives per pixel q col_q = {out.rgb, len},
// mom_q = {s2, dof} and, from its guide copy, prim_q:
//   v_q = rt_div(s2_q, len_q)        m_q = mom_lum(col_q.rgb)
//   tap q counts (sv += v_q, sm += m_q, c++) iff dof_q > 0 and v_q, m_q finite
//   hot_p: the expression above over the window, unchanged (row sums in increasing
//          x, column sums in increasing y)
//   fresh_p = prim_p >= 0 && !(dof_p >= min_dof)
//   selected_p = (max_frames == 0 || n_p + k <= max_frames) &&
//                (n_p < min_frames || hot_p || fresh_p)
// fresh: a hit pixel about which the history says nothing (dof 0 or NaN), or too
// little, is rendered: disocclusions and the first view.  Miss pixels are not
// forced (the reprojection skips them); a silhouette's noise reaches them
// through the window.  The planes are only read.
//
// Counts.  A non-uniform state that rt_render_adaptive started has J_p >= 2;
// rt_render_adaptive_reprojected may start from one batch, and the pixels it does
// not select then keep J_p = 1 (n_p >= 1).  For them ad_var's divisor is 0: v_q
// is M2_q * inf, not finite (NaN for the M2_q = 0 a single batch leaves), and
// ad_row_sums skips the tap like any other non-finite one.
#pragma once
#include "rt_moments.h"

namespace {

RT_HD bool ad_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }  // false for NaN and +-inf

// the variance of pixel q's mean luminance (also rt_get_variance's in the non-uniform state)
RT_HD float ad_var(float M2, unsigned n, unsigned J) { return M2 * rt_div(1.0f, (float)(J - 1u) * (float)n); }

// row sums of the window of pixel (x, y), taps in increasing x
RT_HD void ad_row_sums(const rt_ad_args& A, int x, int y, long p) {
    float sv = 0.0f, sm = 0.0f;
    int c = 0;
    const int x0 = x - A.radius < 0 ? 0 : x - A.radius;
    const int x1 = x + A.radius >= A.width ? A.width - 1 : x + A.radius;
    for (int qx = x0; qx <= x1; qx++) {
        const long q = (long)y * A.width + qx;
        const float2 m = A.mom_in[q];
        const uint2 cn = A.cnt[q];
        const float v = ad_var(m.y, cn.x, cn.y);
        if (!ad_finite(v) || !ad_finite(m.x)) continue;
        sv = sv + v;
        sm = sm + m.x;
        c++;
    }
    A.rowv[p] = sv;
    A.rowm[p] = sm;
    A.rowc[p] = c;
}

// the column sum of the row sums in increasing y, the test and the selection of pixel (x, y)
RT_HD bool ad_selected(const rt_ad_args& A, int x, int y, long p) {
    const unsigned n = A.cnt[p].x;
    if (A.max_frames != 0u && (unsigned long long)n + (unsigned)A.k > A.max_frames) return false;
    if (n < A.min_frames) return true;
    float sv = 0.0f, sm = 0.0f;
    int c = 0;
    const int y0 = y - A.radius < 0 ? 0 : y - A.radius;
    const int y1 = y + A.radius >= A.height ? A.height - 1 : y + A.radius;
    for (int qy = y0; qy <= y1; qy++) {
        const long q = (long)qy * A.width + x;
        sv = sv + A.rowv[q];
        sm = sm + A.rowm[q];
        c += A.rowc[q];
    }
    const float cf = (float)c;
    const float b = A.tolerance * (sm + cf * A.lum_floor);
    return c > 0 && (sv * cf) > (b * b);
}

// ad_row_sums over the pending planes: per tap 16 bytes of {out.rgb, len} and 8
// of {s2, dof}
RT_HD void ad_row_sums_reproj(const rt_ad_reproj_args& R, int x, int y, long p) {
    const rt_ad_args& A = R.A;
    float sv = 0.0f, sm = 0.0f;
    int c = 0;
    const int x0 = x - A.radius < 0 ? 0 : x - A.radius;
    const int x1 = x + A.radius >= A.width ? A.width - 1 : x + A.radius;
    for (int qx = x0; qx <= x1; qx++) {
        const long q = (long)y * A.width + qx;
        const float4 col = R.p_col[q];
        const float2 m = R.p_mom[q];
        const float v = rt_div(m.x, col.w);
        const float l = mom_lum(col.x, col.y, col.z);
        if (!(m.y > 0.0f) || !ad_finite(v) || !ad_finite(l)) continue;
        sv = sv + v;
        sm = sm + l;
        c++;
    }
    A.rowv[p] = sv;
    A.rowm[p] = sm;
    A.rowc[p] = c;
}

// ad_selected with the `fresh` term: the pixel's dof and its primitive id, 4
// bytes each, more (of {s2, dof} only dof is used and the load narrows to it)
RT_HD bool ad_selected_reproj(const rt_ad_reproj_args& R, int x, int y, long p) {
    const rt_ad_args& A = R.A;
    const unsigned n = A.cnt[p].x;
    if (A.max_frames != 0u && (unsigned long long)n + (unsigned)A.k > A.max_frames) return false;
    const int prim = rt_f2i(reinterpret_cast<const float*>(R.p_ga + p)[3]);
    const float dof = R.p_mom[p].y;
    if (prim >= 0 && !(dof >= R.min_dof)) return true;
    return ad_selected(A, x, y, p);
}

// ad_selected for pixel x of shard row j (p = j * width + x in the shard; image
// row y = row_offset + j * shards): the same clauses in the same order, n_p from
// the shard's own counts, the column taps in increasing image y from the ranks'
// gathered row sums (rt_layout.h, rt_ad_shard_args) — the same float additions,
// so the shards select, interleaved, what one full-frame context selects.  The
// block and the row inside it advance per tap without a division: one division
// per pixel, wave-uniform on the device (the kernel hands in a uniform j).
RT_HD bool ad_selected_shard(const rt_ad_shard_args& S, int x, int j, long p) {
    const rt_ad_args& A = S.A;
    const unsigned n = A.cnt[p].x;
    if (A.max_frames != 0u && (unsigned long long)n + (unsigned)A.k > A.max_frames) return false;
    if (n < A.min_frames) return true;
    float sv = 0.0f, sm = 0.0f;
    int c = 0;
    const int y = S.row_offset + j * S.shards;
    const int y0 = y - A.radius < 0 ? 0 : y - A.radius;
    const int y1 = y + A.radius >= S.image_height ? S.image_height - 1 : y + A.radius;
    const long plane = (long)S.rows_per_shard * A.width;
    const int* taps = reinterpret_cast<const int*>(S.gathered);  // plane 2 holds integers
    int qj = y0 / S.shards;       // the tap row's row inside its block
    int r = y0 - qj * S.shards;   // and its block
    for (int qy = y0; qy <= y1; qy++) {
        const long q = ((long)r * 3 * S.rows_per_shard + qj) * A.width + x;
        sv = sv + S.gathered[q];
        sm = sm + S.gathered[q + plane];
        c += taps[q + 2 * plane];
        if (++r == S.shards) {
            r = 0;
            qj++;
        }
    }
    const float cf = (float)c;
    const float b = A.tolerance * (sm + cf * A.lum_floor);
    return c > 0 && (sv * cf) > (b * b);
}

// the moment step of listed pixel p behind its k new frames (rt_moments.h's
// with the pixel's own weight), and its counts
RT_HD void ad_update(const rt_ad_args& A, long p) {
    const uint2 cn = A.cnt[p];
    const float ax = A.accum[p], ay = A.accum[A.npix + p], az = A.accum[2 * A.npix + p];
    const float px = A.prev[p], py = A.prev[A.npix + p], pz = A.prev[2 * A.npix + p];
    const float2 m = A.mom[p];
    const float kw = rt_div(A.kf, (float)(cn.x + (unsigned)A.k));
    const float L = mom_lum(ax - px, ay - py, az - pz);
    const float l = L * A.invk;
    const float dl = l - m.x;
    const float M1 = m.x + dl * kw;
    const float M2n = m.y + (A.kf * dl) * (l - M1);
    A.prev[p] = ax;
    A.prev[A.npix + p] = ay;
    A.prev[2 * A.npix + p] = az;
    A.mom[p] = make_float2(M1, M2n);
    A.cnt[p] = make_uint2(cn.x + (unsigned)A.k, cn.y + 1u);
}

// the image of pixel p: complete whatever earlier renders wrote
RT_HD void ad_resolve(const rt_ad_args& A, long p) {
    const unsigned n = A.cnt[p].x;
    const float ax = A.accum[p], ay = A.accum[A.npix + p], az = A.accum[2 * A.npix + p];
    if (A.rgba) A.rgba[p] = tone_map(ax, ay, az, n);
    if (A.color) {
        const float inv = rt_div(1.0f, (float)n);
        A.color[3 * p + 0] = inv * ax;
        A.color[3 * p + 1] = inv * ay;
        A.color[3 * p + 2] = inv * az;
    }
}

}  // namespace
