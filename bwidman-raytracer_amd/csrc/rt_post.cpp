// rt_post.cpp — what the C ABI (include/rt_abi.h) offers after a render:
// first-hit feature buffers, the a-trous denoiser and temporal reprojection.
//
// None of them reads or writes the RNG state or the frame counter or writes
// frameSum; all always run the exact arithmetic (rt_set_precision selects
// render kernels only).  Compiled with -ffp-contract=off (fill_view's camera
// prelude, the sigma terms).
#include <cmath>

#include "rt_context.h"

namespace {

// Host copies of a result: the tone-mapped image in dn_rgba, the .xyz of
// `color` and the .w of `length` (each only with its destination; one buffer
// in both roles is fetched once).  Synchronises the context's stream.
int read_back(rt_context* c, size_t npix, uint8_t* rgba_out, const Buf* color, float* color_out, const Buf* length,
              float* length_out) {
    if (!color_out) color = nullptr;
    if (!length_out) length = nullptr;
    const float4* pc = color ? color->as<float4>() : nullptr;
    const float4* pl = length ? length->as<float4>() : nullptr;
    std::vector<float4> col, len;  // staging of a GPU context's buffers
    if (c->cpu) {
        if (rgba_out) std::memcpy(rgba_out, c->dn_rgba.p, npix * 4);
    } else {
        const Buf* first = color ? color : length;
        try {
            if (first) col.resize(npix);
            if (length && length != first) len.resize(npix);
        } catch (...) {
            (void)hipStreamSynchronize(c->stream);
            return fail(c, RT_ERR_OUT_OF_MEMORY, "host colour for %zu pixels", npix);
        }
        if (rgba_out) HIP_TRY(c, hipMemcpyAsync(rgba_out, c->dn_rgba.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
        if (first)
            HIP_TRY(c, hipMemcpyAsync(col.data(), first->p, npix * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        if (!len.empty())
            HIP_TRY(c, hipMemcpyAsync(len.data(), length->p, npix * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        pc = col.data();
        pl = len.empty() ? col.data() : len.data();
    }
    if (color_out) xyz_of(pc, npix, color_out);
    if (length_out) w_of(pl, npix, length_out);
    return RT_OK;
}

// The guides of the context's current full frame, recomputed when stale (on
// stream s for a GPU context: part of the denoise call that needs them)
int ensure_guides(rt_context* c, hipStream_t s) {
    if (c->guides_valid) return RT_OK;
    rt_kparams K;
    fill_view(c, c->width, c->height, 0, 1, c->height, K);
    const size_t npix = (size_t)c->height * c->width;
    for (Buf* b : {&c->guide_a, &c->guide_b})
        if (const int rc = ensure_buf(c, *b, npix * sizeof(float4), "host guides for %zu pixels", npix)) return rc;
    float4 *ga = c->guide_a.as<float4>(), *gb = c->guide_b.as<float4>();
    if (c->cpu)
        rt_cpu_aov(K, c->threads, ga, gb, nullptr);
    else
        HIP_TRY(c, K.bvh_nodes ? rt_launch_aov_bvh(K, ga, gb, nullptr, s) : rt_launch_aov(K, ga, gb, nullptr, s));
    c->guides_valid = true;
    return RT_OK;
}

// A scene, an accumulated frame and a full-frame pixel state: what the
// denoiser and the temporal reprojection (`who`) need besides their parameters
int full_frame_check(rt_context* c, const char* who) {
    if (!c->has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    if (c->frame < 2u || !c->accum.p)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "no frame accumulated yet (render first)");
    if (c->row_offset != 0 || c->row_stride > 1)
        return fail(c, RT_ERR_UNSUPPORTED,
                    "the context holds a row shard (offset %d, stride %d): %s needs a full frame", c->row_offset,
                    c->row_stride, who);
    return RT_OK;
}

// The conditions of a denoise call (and of the filter part of a temporal one)
static int denoise_check(rt_context* c, const rt_denoise_params* dp) {
    if (!c || !dp) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (dp->iterations < 0 || dp->iterations > RT_DENOISE_MAX_ITERATIONS)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "iterations %d outside 0..%d", dp->iterations,
                    RT_DENOISE_MAX_ITERATIONS);
    if (!(dp->sigma_color > 0.0f) || !(dp->sigma_normal > 0.0f) || !(dp->sigma_plane > 0.0f))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "sigmas must be > 0 (colour %g, normal %g, plane %g)",
                    (double)dp->sigma_color, (double)dp->sigma_normal, (double)dp->sigma_plane);
    return full_frame_check(c, "the denoiser");
}

// Every level of one denoise call; the final colour ends in dn_col[*final_buf]
// and, tone-mapped, in rgba (device pointer on a GPU context; may be null).
// src0 non-null (rt_temporal; iterations >= 1): level 0 filters that colour
// buffer instead of inv * frameSum.
int denoise_levels(rt_context* c, const rt_denoise_params* dp, hipStream_t s, unsigned* rgba, int* final_buf,
                   const float4* src0 = nullptr) {
    const HostFpEnv fp;
    int rc = denoise_check(c, dp);
    if (rc) return rc;
    const size_t npix = (size_t)c->height * c->width;
    if (!c->cpu) HIP_TRY(c, hipSetDevice(c->device));
    for (Buf& b : c->dn_col)
        if ((rc = ensure_buf(c, b, npix * sizeof(float4), "host colour buffers for %zu pixels", npix))) return rc;
    // after the render that made the frame, a previous denoise (shared colour
    // buffers and guides) and a reprojection pass (it reads the guides; its
    // filter writes the colour buffers), whatever streams they ran on
    if ((rc = order_after_all(c, s))) return rc;
    rc = ensure_guides(c, s);
    if (rc) return rc;
    rt_dn_level L;
    std::memset(&L, 0, sizeof L);
    L.width = c->width;
    L.height = c->height;
    L.inv = 1.0f / (float)(c->frame - 1u);
    L.in = 1.0f / (dp->sigma_normal * dp->sigma_normal);
    L.ip = 1.0f / (dp->sigma_plane * dp->sigma_plane);
    L.accum = c->accum.as<float>();
    L.ga = c->guide_a.as<float4>();
    L.gb = c->guide_b.as<float4>();
    float4* col[2] = {c->dn_col[0].as<float4>(), c->dn_col[1].as<float4>()};
    HIP_TRY(c, c->denoise.begin(s, true));
    const int levels = dp->iterations;
    for (int i = 0; i < (levels > 0 ? levels : 1); i++) {
        L.step = levels > 0 ? 1 << i : 0;  // step 0: the conversion pass of iterations == 0
        const float sc = dp->sigma_color * std::ldexp(1.0f, -i);
        L.ic = 1.0f / (sc * sc);
        L.first = i == 0 && !src0;
        L.last = i >= levels - 1;
        L.src = i > 0 ? col[(i - 1) & 1] : src0;
        L.dst = col[i & 1];
        L.rgba = L.last ? rgba : nullptr;
        if (c->cpu) {
            rt_cpu_denoise_level(L, c->threads);
        } else {
            // BWRT_DENOISE_KERNEL forces a variant; the policy is the per-level
            // winner of tools/time_denoise.py at 1920x1080 (profiles/denoise/,
            // DESIGN.md section 9): the LDS-tiled kernel up to step 16 (0.084-0.139
            // against 0.17-0.19 ms), the direct one at step 32 (0.24 against 0.31
            // ms: the tile's 108 KiB leave one workgroup per CU)
            const bool tiled = c->dn_kernel >= 0 ? c->dn_kernel == 1 : L.step <= 16;
            HIP_TRY(c, rt_launch_denoise_level(L, tiled, s));
        }
    }
    *final_buf = levels > 0 ? (levels - 1) & 1 : 0;
    HIP_TRY(c, c->denoise.end(s));
    return RT_OK;
}

// The variance-guided filter (rt_denoise_var.h) of one call on stream s: the
// input stage, then per level a sigma pass and the level.  The final {colour,
// variance} ends in dn_col[*final_buf] and, tone-mapped, in rgba (device
// pointer on a GPU context; may be null).
int denoise_var_passes(rt_context* c, const rt_denoise_var_params* dp, hipStream_t s, unsigned* rgba,
                       int* final_buf) {
    const HostFpEnv fp;
    if (!c || !dp) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (dp->iterations < 0 || dp->iterations > RT_DENOISE_MAX_ITERATIONS)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "iterations %d outside 0..%d", dp->iterations,
                    RT_DENOISE_MAX_ITERATIONS);
    if (!(dp->sigma_lum > 0.0f) || !(dp->sigma_normal > 0.0f) || !(dp->sigma_plane > 0.0f))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "sigmas must be > 0 (luminance %g, normal %g, plane %g)",
                    (double)dp->sigma_lum, (double)dp->sigma_normal, (double)dp->sigma_plane);
    if (dp->min_batches < 2) return fail(c, RT_ERR_INVALID_ARGUMENT, "min_batches %d < 2", dp->min_batches);
    int rc = full_frame_check(c, "the denoiser");
    if (rc) return rc;
    const size_t npix = (size_t)c->height * c->width;
    if (!c->cpu) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, c->denoise_var.create(true));  // on first use
    }
    for (Buf& b : c->dn_col)
        if ((rc = ensure_buf(c, b, npix * sizeof(float4), "host colour buffers for %zu pixels", npix))) return rc;
    if ((rc = ensure_buf(c, c->dn_rs, npix * sizeof(float), "host sigma plane for %zu pixels", npix))) return rc;
    // after the render that made the frame (and its moment update), and after
    // every pass that shares the guides and the colour buffers
    if ((rc = order_after_all(c, s))) return rc;
    rc = ensure_guides(c, s);
    if (rc) return rc;
    rt_dv_args A;
    std::memset(&A, 0, sizeof A);
    A.width = c->width;
    A.height = c->height;
    const float n = (float)(c->frame - 1u);
    A.inv = 1.0f / n;
    A.in = 1.0f / (dp->sigma_normal * dp->sigma_normal);
    A.ip = 1.0f / (dp->sigma_plane * dp->sigma_plane);
    A.sigma_lum = dp->sigma_lum;
    // the tracked variance of this very frame, else the spatial estimate
    A.tracked = c->mom_live && c->mom_next == c->frame && c->mom_batches >= (unsigned)dp->min_batches;
    if (A.tracked) {
        A.rd = 1.0f / ((float)(c->mom_batches - 1u) * n);
        A.mom = c->mom_m.as<float2>();
    }
    A.accum = c->accum.as<float>();
    A.ga = c->guide_a.as<float4>();
    A.gb = c->guide_b.as<float4>();
    A.rs = c->dn_rs.as<float>();
    float4* col[2] = {c->dn_col[0].as<float4>(), c->dn_col[1].as<float4>()};
    auto pass = [&](int stage) -> int {
        if (c->cpu) {
            rt_cpu_denoise_var(A, stage, c->threads);
            return RT_OK;
        }
        // BWRT_DENOISE_KERNEL forces a variant; the policy is the per-level
        // winner of tools/time_denoise_var.py at 1920x1080 (profiles/denoise_var/,
        // DESIGN.md section 11; sigma pass included): the LDS-tiled kernel up to
        // step 16 (0.120-0.171 against 0.195-0.206 ms), the direct one at step 32
        // (0.236 against 0.346 ms)
        const bool tiled = c->dn_kernel >= 0 ? c->dn_kernel == 1 : A.step <= 16;
        HIP_TRY(c, rt_launch_denoise_var(A, stage, tiled, s));
        return RT_OK;
    };
    HIP_TRY(c, c->denoise_var.begin(s, true));
    const int levels = dp->iterations;
    A.dst = col[0];
    A.last = levels == 0;
    A.rgba = A.last ? rgba : nullptr;
    if ((rc = pass(0))) return rc;
    for (int i = 0; i < levels; i++) {
        A.step = 1 << i;
        A.src = col[i & 1];
        A.dst = col[(i + 1) & 1];
        A.last = i == levels - 1;
        A.rgba = A.last ? rgba : nullptr;
        if ((rc = pass(1)) || (rc = pass(2))) return rc;
    }
    *final_buf = levels & 1;
    HIP_TRY(c, c->denoise_var.end(s));
    return RT_OK;
}

static int temporal_check(rt_context* c, const rt_temporal_params* tp, const rt_denoise_params* dn) {
    if (!c || !tp) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!(tp->max_history > 0.0f) || !(tp->plane_tol > 0.0f) ||
        !(tp->normal_cos_min >= -1.0f && tp->normal_cos_min <= 1.0f))
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "max_history and plane_tol must be > 0, normal_cos_min in -1..1 (%g, %g, %g)",
                    (double)tp->max_history, (double)tp->plane_tol, (double)tp->normal_cos_min);
    if (dn) {
        const int rc = denoise_check(c, dn);
        if (rc) return rc;
    }
    return full_frame_check(c, "reprojection");
}

// One temporal call on stream s: promote, reproject, store the pending result
// of the current view in tp[*set]; with a filter (dn, iterations >= 1) its
// levels follow and *filtered_buf is the dn_col buffer of the final colour
// (else -1: the final colour is the pending one).  rgba: device pointer on a
// GPU context; may be null.
int temporal_pass(rt_context* c, const rt_temporal_params* tp, const rt_denoise_params* dn, hipStream_t s,
                  unsigned* rgba, int* set, int* filtered_buf) {
    const HostFpEnv fp;
    int rc = temporal_check(c, tp, dn);
    if (rc) return rc;
    const bool filter = dn && dn->iterations > 0;
    const size_t npix = (size_t)c->height * c->width;
    if (c->tp_w != c->width || c->tp_h != c->height) {  // (rt_init_rand dropped them already)
        c->tp_has_hist = c->tp_has_pending = false;
        c->tp_w = c->width;
        c->tp_h = c->height;
    }
    if (!c->cpu) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, c->temporal.create(true));  // on first use
    }
    for (rt_context::TpSet& t : c->tp)
        for (Buf* b : {&t.col, &t.ga, &t.gb})
            if ((rc = ensure_buf(c, *b, npix * sizeof(float4), "host history buffers for %zu pixels", npix))) return rc;
    // after the render that made the frame, a previous denoise (the guides;
    // its levels may still read a pending colour) and a previous temporal
    // call (it reads the set this one writes), whatever streams they ran on
    if ((rc = order_after_all(c, s))) return rc;
    rc = ensure_guides(c, s);
    if (rc) return rc;
    // the first call of a later view: the pending result becomes the history.
    // The swap is of host-side roles only; the stream waits above order this
    // call's kernel after every earlier reader of the set it now writes.
    if (c->tp_has_pending && c->tp_pending_view != c->view) {
        c->tp_hist ^= 1;
        c->tp_has_hist = true;
        c->tp_has_pending = false;
    }
    const rt_context::TpSet& H = c->tp[c->tp_hist];
    rt_context::TpSet& P = c->tp[c->tp_hist ^ 1];
    rt_kparams K;
    fill_view(c, c->width, c->height, 0, 1, c->height, K);
    rt_tp_args T;
    std::memset(&T, 0, sizeof T);
    T.width = c->width;
    T.height = c->height;
    T.has_history = c->tp_has_hist ? 1 : 0;
    T.n = (float)(c->frame - 1u);
    T.inv = 1.0f / (float)(c->frame - 1u);
    T.max_history = tp->max_history;
    T.normal_cos_min = tp->normal_cos_min;
    T.plane_tol = tp->plane_tol;
    std::memcpy(T.h_cam, H.cam_pos, sizeof T.h_cam);
    std::memcpy(T.h_rot, H.rot, sizeof T.h_rot);
    T.h_screen_z = H.screen_z;
    T.accum = c->accum.as<float>();
    T.ga = c->guide_a.as<float4>();
    T.gb = c->guide_b.as<float4>();
    T.h_col = H.col.as<float4>();
    T.h_ga = H.ga.as<float4>();
    T.h_gb = H.gb.as<float4>();
    T.p_col = P.col.as<float4>();
    T.p_ga = P.ga.as<float4>();
    T.p_gb = P.gb.as<float4>();
    T.rgba = filter ? nullptr : rgba;  // the filter's last level writes it otherwise
    HIP_TRY(c, c->temporal.begin(s, true));
    if (c->cpu)
        rt_cpu_temporal(T, c->threads);
    else
        HIP_TRY(c, rt_launch_temporal(T, s));
    HIP_TRY(c, c->temporal.end(s));
    std::memcpy(P.cam_pos, K.cam_pos, sizeof P.cam_pos);
    std::memcpy(P.rot, K.rot, sizeof P.rot);
    P.screen_z = K.screen_z;
    c->tp_has_pending = true;
    c->tp_pending_view = c->view;
    *set = c->tp_hist ^ 1;
    *filtered_buf = -1;
    if (filter) {
        int fb = 0;
        rc = denoise_levels(c, dn, s, rgba, &fb, T.p_col);
        if (rc) return rc;
        *filtered_buf = fb;
    }
    return RT_OK;
}

// dn_rgba for a call that wants the tone-mapped image on the host
int ensure_rgba(rt_context* c, uint8_t* rgba_out, size_t npix) {
    if (!rgba_out) return RT_OK;
    if (!c->cpu) HIP_TRY(c, hipSetDevice(c->device));
    return ensure_buf(c, c->dn_rgba, npix * 4, "host RGBA for %zu pixels", npix);
}

}  // namespace

extern "C" {

int rt_render_aov(rt_context* c, const rt_render_params* p, float* albedo, float* normal, float* depth,
                  int32_t* prim) {
    const HostFpEnv fp;
    if (!c || !p) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!c->has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    const int stride = p->row_stride == 0 ? 1 : p->row_stride;
    if (const int rc = shard_check(c, p->width, p->height, p->row_offset, stride)) return rc;
    const int rows = shard_rows(p->height, p->row_offset, stride);
    const size_t npix = (size_t)rows * p->width;
    rt_kparams K;
    fill_view(c, p->width, p->height, p->row_offset, stride, rows, K);
    std::vector<float4> a, b, al;
    try {
        a.resize(npix);
        b.resize(npix);
        if (albedo) al.resize(npix);
    } catch (...) {
        return fail(c, RT_ERR_OUT_OF_MEMORY, "host buffers for %zu pixels", npix);
    }
    if (c->cpu) {
        rt_cpu_aov(K, c->threads, a.data(), b.data(), albedo ? al.data() : nullptr);
    } else {
        HIP_TRY(c, hipSetDevice(c->device));
        int rc = ensure_buf(c, c->aov_a, npix * sizeof(float4));
        if (!rc) rc = ensure_buf(c, c->aov_b, npix * sizeof(float4));
        if (!rc && albedo) rc = ensure_buf(c, c->aov_alb, npix * sizeof(float4));
        if (rc) return rc;
        float4 *da = c->aov_a.as<float4>(), *db = c->aov_b.as<float4>(), *dal = albedo ? c->aov_alb.as<float4>() : nullptr;
        HIP_TRY(c, K.bvh_nodes ? rt_launch_aov_bvh(K, da, db, dal, c->stream) : rt_launch_aov(K, da, db, dal, c->stream));
        HIP_TRY(c, hipMemcpyAsync(a.data(), da, npix * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(b.data(), db, npix * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        if (albedo)
            HIP_TRY(c, hipMemcpyAsync(al.data(), dal, npix * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (albedo) xyz_of(al.data(), npix, albedo);
    if (normal) xyz_of(a.data(), npix, normal);
    if (depth) w_of(b.data(), npix, depth);
    if (prim) w_of(a.data(), npix, prim);
    return RT_OK;
}

rt_denoise_params rt_denoise_params_default(void) {
    rt_denoise_params d;
    d.iterations = 5;
    // tools/denoise_sigma_sweep.py (DESIGN.md "Denoiser")
    d.sigma_color = 16.0f;
    d.sigma_normal = 0.5f;
    d.sigma_plane = 0.1f;
    return d;
}

int rt_denoise(rt_context* c, const rt_denoise_params* dp, uint8_t* rgba_out, float* color_out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const size_t npix = (size_t)c->height * c->width;
    int fb = 0;
    int rc = ensure_rgba(c, rgba_out, npix);
    if (!rc) rc = denoise_levels(c, dp, c->stream, rgba_out ? c->dn_rgba.as<unsigned>() : nullptr, &fb);
    if (rc) return rc;
    return read_back(c, npix, rgba_out, &c->dn_col[fb], color_out, nullptr, nullptr);
}

int rt_denoise_device(rt_context* c, const rt_denoise_params* dp, void* rgba_device, void* stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (c->cpu) return fail(c, RT_ERR_UNSUPPORTED, "rt_denoise_device: CPU context");
    if (rgba_device && ((uintptr_t)rgba_device & 3u))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "rgba_device not 4-byte aligned");
    int fb = 0;
    return denoise_levels(c, dp, stream ? (hipStream_t)stream : c->stream, (unsigned*)rgba_device, &fb);
}

float rt_last_denoise_ms(rt_context* c) { return c ? c->denoise.elapsed_ms() : -1.0f; }

// ---- variance-guided filter ------------------------------------------------------
// (csrc/rt_denoise_var.h has the arithmetic)

rt_denoise_var_params rt_denoise_var_params_default(void) {
    rt_denoise_var_params d;
    d.iterations = 5;
    // tools/denoise_var_sweep.py: on 8-frame estimates
    // the grid prefers a far wider luminance term than SVGF's 4
    d.sigma_lum = 32.0f;
    d.sigma_normal = 0.5f;
    d.sigma_plane = 0.1f;
    d.min_batches = 4;
    return d;
}

int rt_denoise_var(rt_context* c, const rt_denoise_var_params* dp, uint8_t* rgba_out, float* color_out,
                   float* var_out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const size_t npix = (size_t)c->height * c->width;
    int fb = 0;
    int rc = ensure_rgba(c, rgba_out, npix);
    if (!rc) rc = denoise_var_passes(c, dp, c->stream, rgba_out ? c->dn_rgba.as<unsigned>() : nullptr, &fb);
    if (rc) return rc;
    return read_back(c, npix, rgba_out, &c->dn_col[fb], color_out, &c->dn_col[fb], var_out);
}

int rt_denoise_var_device(rt_context* c, const rt_denoise_var_params* dp, void* rgba_device, void* stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (c->cpu) return fail(c, RT_ERR_UNSUPPORTED, "rt_denoise_var_device: CPU context");
    if (rgba_device && ((uintptr_t)rgba_device & 3u))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "rgba_device not 4-byte aligned");
    int fb = 0;
    return denoise_var_passes(c, dp, stream ? (hipStream_t)stream : c->stream, (unsigned*)rgba_device, &fb);
}

float rt_last_denoise_var_ms(rt_context* c) { return c ? c->denoise_var.elapsed_ms() : -1.0f; }

// ---- temporal reprojection ----------------------------------------------------
// (csrc/rt_temporal.h has the arithmetic)

rt_temporal_params rt_temporal_params_default(void) {
    rt_temporal_params t;
    // tools/temporal_sweep.py
    t.max_history = 32.0f;
    t.normal_cos_min = 0.9f;
    t.plane_tol = 0.02f;
    return t;
}

int rt_temporal(rt_context* c, const rt_temporal_params* tp, const rt_denoise_params* dn, uint8_t* rgba_out,
                float* color_out, float* length_out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const size_t npix = (size_t)c->height * c->width;
    int set = 0, fb = -1;
    int rc = ensure_rgba(c, rgba_out, npix);
    if (!rc) rc = temporal_pass(c, tp, dn, c->stream, rgba_out ? c->dn_rgba.as<unsigned>() : nullptr, &set, &fb);
    if (rc) return rc;
    const Buf& pending = c->tp[set].col;  // {colour, history length}
    return read_back(c, npix, rgba_out, fb >= 0 ? &c->dn_col[fb] : &pending, color_out, &pending, length_out);
}

int rt_temporal_device(rt_context* c, const rt_temporal_params* tp, const rt_denoise_params* dn, void* rgba_device,
                       void* stream) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (c->cpu) return fail(c, RT_ERR_UNSUPPORTED, "rt_temporal_device: CPU context");
    if (rgba_device && ((uintptr_t)rgba_device & 3u))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "rgba_device not 4-byte aligned");
    int set = 0, fb = -1;
    return temporal_pass(c, tp, dn, stream ? (hipStream_t)stream : c->stream, (unsigned*)rgba_device, &set, &fb);
}

int rt_temporal_reset(rt_context* c) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    // roles only: work still queued on the buffers is ordered by the next call's stream waits
    c->tp_has_hist = c->tp_has_pending = false;
    return RT_OK;
}

float rt_last_temporal_ms(rt_context* c) { return c ? c->temporal.elapsed_ms() : -1.0f; }

// ---- luminance moment tracking ------------------------------------------------
// (csrc/rt_moments.h has the update, rt_render.cpp runs
// it behind every render call)

int rt_set_moments(rt_context* c, int enable) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const bool on = enable != 0;
    // off ends the tracking; on starts not live (a render of frame 1 makes it
    // live), also in mid-accumulation.  The buffers stay for the next use.
    if (on != c->mom_on) c->mom_drop();
    c->mom_on = on;
    return RT_OK;
}

int rt_get_moments(const rt_context* c) { return c && c->mom_on ? 1 : 0; }

int rt_moments_batches(const rt_context* c) { return c && c->mom_live ? (int)c->mom_batches : 0; }

int rt_get_variance(rt_context* c, float* var_out, float* lum_out) {
    const HostFpEnv fp;
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (!c->mom_live || c->mom_batches < 2u)
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "no variance yet: moment tracking %s, %u batches (needs rt_set_moments and two render calls "
                    "of one accumulation)",
                    c->mom_live ? "live" : "not live", c->mom_live ? c->mom_batches : 0u);
    const size_t npix = (size_t)c->rows * c->width;
    const float2* m = c->mom_m.as<float2>();
    std::vector<float2> host;
    if (!c->cpu) {
        HIP_TRY(c, hipSetDevice(c->device));
        try {
            host.resize(npix);
        } catch (...) {
            return fail(c, RT_ERR_OUT_OF_MEMORY, "host moments for %zu pixels", npix);
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        const int rc = quiesce(c);  // the last render (and its update pass), on whatever stream it ran
        if (rc) return rc;
        HIP_TRY(c, hipMemcpy(host.data(), m, npix * sizeof(float2), hipMemcpyDeviceToHost));
        m = host.data();
    }
    // 1 / ((J - 1) n), n = the frames accumulated
    const float rd = 1.0f / ((float)(c->mom_batches - 1u) * (float)(c->mom_next - 1u));
    for (size_t i = 0; i < npix; i++) {
        if (var_out) var_out[i] = m[i].y * rd;
        if (lum_out) lum_out[i] = m[i].x;
    }
    return RT_OK;
}

}  // extern "C"
