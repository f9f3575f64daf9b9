// rt_post.cpp — what the C ABI (include/rt_abi.h) offers after a render:
// first-hit feature buffers, the a-trous denoisers and temporal reprojection
// (with and without the luminance moments).
//
// None of them reads or writes the RNG state or the frame counter or writes
// frameSum; all always run the exact arithmetic (rt_set_precision selects
// render kernels only).  Compiled with -ffp-contract=off (fill_view's camera
// prelude, the sigma terms).
#include <cmath>
#include <initializer_list>

#include "rt_adaptive.h"
#include "rt_group.h"
#include "rt_temporal_var.h"

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
// stream s for a GPU context: part of the denoise call that needs them).  Always
// of the full width x height view, whatever rows the context's own state holds.
int ensure_guides(rt_context* c, hipStream_t s) {
    if (c->vs.guides_valid()) return RT_OK;
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
    c->vs.guides_computed();
    return RT_OK;
}

// Which frame a full-frame pass reads.  A context whose
// pixel state is the full frame reads its own accumulation and never consults
// an assembled frame: a stale snapshot cannot replace newer data.  A context
// that holds a row shard reads its assembled frame (rt_assemble) while that is
// current: its planes, its n and, with moments, theirs and J.  A COUNTED
// assembled frame (rt_assemble_adaptive, section 19) also has every pixel's
// {n_p, J_p} (frame_counts): the passes take those, as on a context in the
// non-uniform state, and n and J here are only the uniform base.
struct FrameSrc {
    const float* sum;    // frameSum, 3 planes of width * height
    const float2* mom;   // {M, M2} per pixel (read only when `tracked`)
    unsigned frames;     // n
    unsigned batches;    // J
    bool tracked;        // mom describes this very frame
};
bool reads_assembled(const rt_context* c) { return c->holds_shard() && c->assembled_current(); }
FrameSrc frame_src(const rt_context* c) {
    if (reads_assembled(c)) {
        const rt_view_state::Assembled& a = c->vs.assembled();  // (batches is 0 without moments)
        const bool mom = c->assembled_shape().moments;
        return {c->as.sum.as<float>(), mom ? c->as.mom.as<float2>() : nullptr, a.frames, a.batches, mom};
    }
    return {c->accum.as<float>(), c->mom_m.as<float2>(), c->st.frames(), c->st.batches(), c->st.current()};
}

// A scene, an accumulated frame and a full-frame pixel state (or a current
// assembled frame on a shard context): what the denoiser and the temporal
// reprojection (`who`) need besides their parameters
int full_frame_check(rt_context* c, const char* who) {
    if (!c->has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    if (reads_assembled(c)) {
        // a snapshot with its own n >= 1, whatever state the shard's own accumulation is in; one with
        // counts is a non-uniform frame, which the passes take only behind the same switch
        if (c->assembled_shape().counted && !c->st.filters())
            return fail(c, RT_ERR_UNSUPPORTED,
                        "the assembled frame is non-uniform (rt_assemble_adaptive): %s takes one frame count for all "
                        "pixels (rt_set_adaptive_filters)", who);
        return RT_OK;
    }
    const char* shard = "the context holds a row shard (offset %d, stride %d): %s needs a full frame%s";
    // (a stale assembled frame is reported whatever the shard's own frame counter says)
    if (c->holds_shard() && c->vs.assembled().made)
        return fail(c, RT_ERR_UNSUPPORTED, shard, c->row_offset, c->row_stride, who,
                    " (its assembled frame is stale: the view or the frame shape changed since rt_assemble)");
    if (c->st.frame() < 2u || !c->accum.p)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "no frame accumulated yet (render first)");
    if (c->holds_shard()) return fail(c, RT_ERR_UNSUPPORTED, shard, c->row_offset, c->row_stride, who, "");
    if (c->st.filters_refuse())
        return fail(c, RT_ERR_UNSUPPORTED,
                    "the accumulation is non-uniform (rt_render_adaptive): %s takes one frame count for all pixels", who);
    return RT_OK;
}

// The counts {n_p, J_p} of the context's own pixel state while that is
// non-uniform; null = uniform.  The adaptive call that wrote them ran inside the
// render pass, so prepare_frame's order_after_all has ordered the stream behind
// its update and resolve passes, whatever stream it ran on.
const uint2* own_counts(const rt_context* c) { return c->st.nonuniform() ? c->ad_cnt.as<uint2>() : nullptr; }

// The counts a full-frame pass takes beside frame_src's planes (then every
// pixel's colour is rt_div(1, n_p) * frameSum_p, rt_atrous.h); null = uniform.
// An assembled frame brings its own or has none: the shard's counts describe
// other pixels.
const uint2* frame_counts(const rt_context* c) {
    if (reads_assembled(c)) return c->assembled_shape().counted ? c->as.cnt.as<uint2>() : nullptr;
    return own_counts(c);
}

// iterations and sigmas of a filter (`term`: what its first sigma weighs)
int filter_check(rt_context* c, int iterations, const char* term, float s0, float sn, float sp) {
    if (iterations < 0 || iterations > RT_DENOISE_MAX_ITERATIONS)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "iterations %d outside 0..%d", iterations, RT_DENOISE_MAX_ITERATIONS);
    if (!(s0 > 0.0f) || !(sn > 0.0f) || !(sp > 0.0f))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "sigmas must be > 0 (%s %g, normal %g, plane %g)", term, (double)s0,
                    (double)sn, (double)sp);
    return RT_OK;
}

// The conditions of a denoise call (and of the filter part of a temporal one)
int denoise_check(rt_context* c, const rt_denoise_params* dp) {
    if (!c || !dp) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    const int rc = filter_check(c, dp->iterations, "colour", dp->sigma_color, dp->sigma_normal, dp->sigma_plane);
    return rc ? rc : full_frame_check(c, "the denoiser");
}

// A buffer of a full-frame pass: `elem` bytes per pixel, and the message of a
// CPU context that cannot allocate it
struct Need {
    Buf* buf;
    size_t elem;
    const char* host_oom;
};

// Everything a full-frame pass (`who`) on stream s does before its first
// kernel: the frame check, the device, the pass's events (on first use), its
// buffers, then stream s ordered after the render that made the frame (and its
// moment update) and after every earlier pass (they share the guides, the
// colour buffers and the history sets, whatever streams they ran on), and the
// guides.
int prepare_frame(rt_context* c, const char* who, Pass& pass, hipStream_t s, std::initializer_list<Need> bufs) {
    int rc = full_frame_check(c, who);
    if (rc) return rc;
    const size_t npix = (size_t)c->height * c->width;
    if (!c->cpu) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, pass.create(true));
    }
    for (const Need& n : bufs)
        if ((rc = ensure_buf(c, *n.buf, npix * n.elem, n.host_oom, npix))) return rc;
    if ((rc = order_after_all(c, s))) return rc;
    return ensure_guides(c, s);
}

Need colour_buf(Buf& b) { return {&b, sizeof(float4), "host colour buffers for %zu pixels"}; }

// The fields of an a-trous frame that hold for every pass of one call
void fill_frame(const rt_context* c, float sigma_normal, float sigma_plane, rt_at_frame& F) {
    F.width = c->width;
    F.height = c->height;
    const FrameSrc src = frame_src(c);
    F.inv = 1.0f / (float)src.frames;
    F.in = 1.0f / (sigma_normal * sigma_normal);
    F.ip = 1.0f / (sigma_plane * sigma_plane);
    F.accum = src.sum;
    F.ga = c->guide_a.as<float4>();
    F.gb = c->guide_b.as<float4>();
}

// The variant of a filter level on a GPU context.  BWRT_DENOISE_KERNEL forces
// one; the policy is the per-level winner at 1920x1080, the same for both
// filters: the LDS-tiled kernel up to step 16, the direct one at step 32 (the
// tile's 108 KiB leave one workgroup per CU).
//   rt_denoise, tools/time_denoise.py (profiles/denoise/):
//     tiled 0.084-0.139 against 0.17-0.19 ms up to step 16, direct 0.24 against
//     0.31 ms at step 32
//   rt_denoise_var, tools/time_denoise_var.py (profiles/denoise_var/, DESIGN.md
//     section 11; sigma pass included): tiled 0.120-0.171 against 0.195-0.206
//     ms up to step 16, direct 0.236 against 0.346 ms at step 32
bool level_tiled(const rt_context* c, int step) { return c->dn_kernel >= 0 ? c->dn_kernel == 1 : step <= 16; }

// Where a pass left its result for read_back
struct Result {
    const Buf* color = nullptr;
    const Buf* length = nullptr;
    const Buf* moments = nullptr;  // rt_temporal_var: the pending {s2, dof}
    bool filtered = false;         // rt_temporal_var: color's .w is the levels' final variance
};

// Every level of one denoise call on stream s; the final colour ends in
// out.color and, tone-mapped, in rgba (device pointer on a GPU context; may be
// null).  src0 non-null (rt_temporal; iterations >= 1): level 0 filters that
// colour buffer instead of inv * frameSum.
int denoise_levels(rt_context* c, const rt_denoise_params* dp, hipStream_t s, unsigned* rgba, Result& out,
                   const float4* src0 = nullptr) {
    const HostFpEnv fp;
    int rc = denoise_check(c, dp);
    if (!rc) rc = prepare_frame(c, "the denoiser", c->denoise, s, {colour_buf(c->dn_col[0]), colour_buf(c->dn_col[1])});
    if (rc) return rc;
    rt_dn_level L;
    std::memset(&L, 0, sizeof L);
    fill_frame(c, dp->sigma_normal, dp->sigma_plane, L.f);
    L.cnt = frame_counts(c);  // (read where `first` is: level 0 and the conversion pass)
    float4* col[2] = {c->dn_col[0].as<float4>(), c->dn_col[1].as<float4>()};
    HIP_TRY(c, c->denoise.begin(s, true));
    const int levels = dp->iterations;
    for (int i = 0; i < (levels > 0 ? levels : 1); i++) {
        L.f.step = levels > 0 ? 1 << i : 0;  // step 0: the conversion pass of iterations == 0
        const float sc = dp->sigma_color * std::ldexp(1.0f, -i);
        L.ic = 1.0f / (sc * sc);
        L.first = i == 0 && !src0;
        L.f.last = i >= levels - 1;
        L.f.src = i > 0 ? col[(i - 1) & 1] : src0;
        L.f.dst = col[i & 1];
        L.f.rgba = L.f.last ? rgba : nullptr;
        if (c->cpu)
            rt_cpu_denoise_level(L, c->threads);
        else
            HIP_TRY(c, rt_launch_denoise_level(L, level_tiled(c, L.f.step), s));
    }
    out.color = &c->dn_col[levels > 0 ? (levels - 1) & 1 : 0];
    HIP_TRY(c, c->denoise.end(s));
    return RT_OK;
}

// The parameter rules of the variance-guided filter
int denoise_var_check(rt_context* c, const rt_denoise_var_params* dp) {
    const int rc = filter_check(c, dp->iterations, "luminance", dp->sigma_lum, dp->sigma_normal, dp->sigma_plane);
    if (rc) return rc;
    if (dp->min_batches < 2) return fail(c, RT_ERR_INVALID_ARGUMENT, "min_batches %d < 2", dp->min_batches);
    return RT_OK;
}

// The pending state of an rt_temporal_var call, for the levels that run behind it
struct TvPending {
    const float4* col;  // {out.rgb, len_out}
    const float2* mom;  // {s2_out, dof_out}
};

// The variance-guided filter (rt_denoise_var.h) of one call on stream s: the
// input stage, then per level a sigma pass and the level.  The final {colour,
// variance} ends in out.color = out.length and, tone-mapped, in rgba (device
// pointer on a GPU context; may be null).  tv non-null (rt_temporal_var on a
// uniform frame; iterations >= 1): the input stage is rt_temporal_var.h's over
// that pending state instead of frameSum and the tracked moments.
int denoise_var_passes(rt_context* c, const rt_denoise_var_params* dp, hipStream_t s, unsigned* rgba, Result& out,
                       const TvPending* tv = nullptr) {
    const HostFpEnv fp;
    if (!c || !dp) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    int rc = denoise_var_check(c, dp);
    if (rc) return rc;
    rc = prepare_frame(c, "the denoiser", c->denoise_var, s,
                       {colour_buf(c->dn_col[0]), colour_buf(c->dn_col[1]),
                        {&c->dn_rs, sizeof(float), "host sigma plane for %zu pixels"}});
    if (rc) return rc;
    rt_dv_args A;
    std::memset(&A, 0, sizeof A);
    fill_frame(c, dp->sigma_normal, dp->sigma_plane, A.f);
    A.sigma_lum = dp->sigma_lum;
    // the tracked variance of this very frame, else the spatial estimate
    const FrameSrc src = frame_src(c);
    A.tracked = src.tracked && src.batches >= (unsigned)dp->min_batches;
    if (A.tracked) {
        A.rd = 1.0f / ((float)(src.batches - 1u) * (float)src.frames);
        A.mom = src.mom;
    }
    // non-uniform: the frame and batch counts are the uniform base, but every
    // pixel's moments are current for its own n_p (the state lives only while
    // tracking does): the choice is per pixel, J_p >= min_batches.  The moments
    // are the frame's own; a counted assembled frame of 4 planes has none and
    // J_p = 0 everywhere, so every pixel takes the spatial estimate.
    if ((A.cnt = frame_counts(c))) {
        A.tracked = 0;
        A.min_batches = (unsigned)dp->min_batches;
        A.mom = src.mom;
    }
    A.rs = c->dn_rs.as<float>();
    float4* col[2] = {c->dn_col[0].as<float4>(), c->dn_col[1].as<float4>()};
    const int levels = dp->iterations;
    // stage 0 into col[0], then level i (sigma pass and level) from col[i & 1] into the other
    auto pass = [&](int stage, int i) -> int {
        A.f.last = i == levels - 1;
        A.f.rgba = A.f.last ? rgba : nullptr;
        if (c->cpu)
            rt_cpu_denoise_var(A, stage, c->threads);
        else
            HIP_TRY(c, rt_launch_denoise_var(A, stage, level_tiled(c, A.f.step), s));
        return RT_OK;
    };
    HIP_TRY(c, c->denoise_var.begin(s, true));
    A.f.dst = col[0];
    if (tv) {
        rt_tv_input I;
        std::memset(&I, 0, sizeof I);
        I.f = A.f;  // (last = 0: a level follows)
        I.dof_min = (float)dp->min_batches - 1.5f;
        I.col = tv->col;
        I.mom = tv->mom;
        if (c->cpu)
            rt_cpu_temporal_var_input(I, c->threads);
        else
            HIP_TRY(c, rt_launch_temporal_var_input(I, s));
    } else if ((rc = pass(0, -1))) {
        return rc;
    }
    for (int i = 0; i < levels; i++) {
        A.f.step = 1 << i;
        A.f.src = col[i & 1];
        A.f.dst = col[(i + 1) & 1];
        if ((rc = pass(1, i)) || (rc = pass(2, i))) return rc;
    }
    out.color = &c->dn_col[levels & 1];
    if (!tv) out.length = out.color;
    HIP_TRY(c, c->denoise_var.end(s));
    return RT_OK;
}

int temporal_check(rt_context* c, const rt_temporal_params* tp, const rt_denoise_params* dn) {
    if (!c || !tp) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!(tp->max_history > 0.0f) || !(tp->plane_tol > 0.0f) ||
        !(tp->normal_cos_min >= -1.0f && tp->normal_cos_min <= 1.0f))
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "max_history and plane_tol must be > 0, normal_cos_min in -1..1 (%g, %g, %g)",
                    (double)tp->max_history, (double)tp->plane_tol, (double)tp->normal_cos_min);
    return dn ? denoise_check(c, dn) : RT_OK;
}

// The history sets at the start of one rt_temporal or rt_temporal_var call (the
// two share them; rt_view.h has the rules).  Fills the pass T (zeroed by the
// caller; all but rgba) and the current view K; returns the set the call writes
// and, through `hist`, the history it reads.
rt_context::TpSet& temporal_sets(rt_context* c, const rt_temporal_params* tp, rt_tp_uniform& T, rt_kparams& K,
                                 const rt_context::TpSet** hist = nullptr) {
    c->vs.temporal_start(c->width, c->height);
    const rt_context::TpSet& H = c->tp[c->vs.history_set()];
    rt_context::TpSet& P = c->tp[c->vs.pending_set()];
    fill_view(c, c->width, c->height, 0, 1, c->height, K);
    T.width = c->width;
    T.height = c->height;
    T.has_history = c->vs.has_history() ? 1 : 0;
    const FrameSrc src = frame_src(c);
    T.n = (float)src.frames;
    T.inv = 1.0f / (float)src.frames;
    T.max_history = tp->max_history;
    T.normal_cos_min = tp->normal_cos_min;
    T.plane_tol = tp->plane_tol;
    std::memcpy(T.h_cam, H.cam_pos, sizeof T.h_cam);
    std::memcpy(T.h_rot, H.rot, sizeof T.h_rot);
    T.h_screen_z = H.screen_z;
    T.accum = src.sum;
    T.ga = c->guide_a.as<float4>();
    T.gb = c->guide_b.as<float4>();
    T.h_col = H.col.as<float4>();
    T.h_ga = H.ga.as<float4>();
    T.h_gb = H.gb.as<float4>();
    T.p_col = P.col.as<float4>();
    T.p_ga = P.ga.as<float4>();
    T.p_gb = P.gb.as<float4>();
    if (hist) *hist = &H;
    return P;
}

// The pending set P now holds the result of the current view K
void temporal_stored(rt_context* c, rt_context::TpSet& P, const rt_kparams& K, bool has_mom) {
    std::memcpy(P.cam_pos, K.cam_pos, sizeof P.cam_pos);
    std::memcpy(P.rot, K.rot, sizeof P.rot);
    P.screen_z = K.screen_z;
    c->vs.temporal_stored(has_mom);
}

// One temporal call on stream s: promote, reproject, store the pending result
// of the current view {colour, history length} in out.length; with a filter
// (dn, iterations >= 1) its levels follow and out.color is their final colour,
// else the pending one.  rgba: device pointer on a GPU context; may be null.
int temporal_pass(rt_context* c, const rt_temporal_params* tp, const rt_denoise_params* dn, hipStream_t s,
                  unsigned* rgba, Result& out) {
    const HostFpEnv fp;
    int rc = temporal_check(c, tp, dn);
    if (!rc) {
        auto hist = [](Buf& b) { return Need{&b, sizeof(float4), "host history buffers for %zu pixels"}; };
        rt_context::TpSet *t0 = &c->tp[0], *t1 = &c->tp[1];
        rc = prepare_frame(c, "reprojection", c->temporal, s,
                           {hist(t0->col), hist(t0->ga), hist(t0->gb), hist(t1->col), hist(t1->ga), hist(t1->gb)});
    }
    if (rc) return rc;
    const bool filter = dn && dn->iterations > 0;
    rt_tp_args T;
    std::memset(&T, 0, sizeof T);
    rt_kparams K;
    rt_context::TpSet& P = temporal_sets(c, tp, T, K);
    T.rgba = filter ? nullptr : rgba;  // the filter's last level writes it otherwise
    T.cnt = frame_counts(c);           // non-uniform: they replace n and inv
    HIP_TRY(c, c->temporal.begin(s, true));
    if (c->cpu)
        rt_cpu_temporal(T, c->threads);
    else
        HIP_TRY(c, rt_launch_temporal(T, s));
    HIP_TRY(c, c->temporal.end(s));
    temporal_stored(c, P, K, false);
    out.color = out.length = &P.col;
    return filter ? denoise_levels(c, dn, s, rgba, out, T.p_col) : RT_OK;
}

// One rt_temporal_var call on stream s (rt_temporal_var.h): rt_temporal's pass
// on the shared history sets with the {s2, dof} plane beside the colour, then,
// with a filter (dv, iterations >= 1), the variance-guided levels behind the
// call's own input stage.  out.length and out.moments are the pending planes,
// out.color the levels' final {colour, variance} or the pending colour.
// `counted` (rt_temporal_var_counted): a non-uniform frame is taken, behind
// rt_set_adaptive_filters (full_frame_check), with every pixel's own counts.
int temporal_var_pass(rt_context* c, const rt_temporal_params* tp, const rt_denoise_var_params* dv, hipStream_t s,
                      unsigned* rgba, Result& out, bool counted = false) {
    const HostFpEnv fp;
    int rc = temporal_check(c, tp, nullptr);
    if (!rc && dv) rc = denoise_var_check(c, dv);
    if (!rc) rc = full_frame_check(c, "moment reprojection");
    // (before anything is allocated or promoted: per-pixel counts in the merge are rt_temporal_var_counted's)
    if (!rc && !counted && frame_counts(c))
        return fail(c, RT_ERR_UNSUPPORTED,
                    "the frame is non-uniform (rt_render_adaptive, rt_assemble_adaptive): rt_temporal_var takes one "
                    "frame count for all pixels, with or without rt_set_adaptive_filters");
    if (!rc) {
        auto hist = [](Buf& b, size_t elem) { return Need{&b, elem, "host history buffers for %zu pixels"}; };
        rt_context::TpSet *t0 = &c->tp[0], *t1 = &c->tp[1];
        const size_t e = sizeof(float4);
        rc = prepare_frame(c, "moment reprojection", c->temporal_var, s,
                           {hist(t0->col, e), hist(t0->ga, e), hist(t0->gb, e), hist(t0->mom, sizeof(float2)),
                            hist(t1->col, e), hist(t1->ga, e), hist(t1->gb, e), hist(t1->mom, sizeof(float2))});
    }
    if (rc) return rc;
    const bool filter = dv && dv->iterations > 0;
    rt_tv_cnt_args V;
    std::memset(&V, 0, sizeof V);
    rt_kparams K;
    const rt_context::TpSet* H;
    rt_context::TpSet& P = temporal_sets(c, tp, V.t, K, &H);
    V.t.rgba = filter ? nullptr : rgba;  // the filter's last level writes it otherwise
    const FrameSrc src = frame_src(c);
    V.tracked = src.tracked && src.batches >= 2u;
    if (V.tracked) {
        V.dof_c = (float)(src.batches - 1u);
        V.mom = src.mom;
    }
    // non-uniform: whether the frame carries moments at all; J_p >= 2 is the pixel's question
    if ((V.cnt = frame_counts(c))) {
        V.tracked = src.tracked;
        V.dof_c = 0.0f;
        V.mom = src.tracked ? src.mom : nullptr;
    }
    V.h_mom = c->vs.history_has_moments() ? H->mom.as<float2>() : nullptr;
    V.p_mom = P.mom.as<float2>();
    HIP_TRY(c, c->temporal_var.begin(s, true));
    if (c->cpu)
        rt_cpu_temporal_var(V, c->threads);
    else
        HIP_TRY(c, rt_launch_temporal_var(V, s));
    HIP_TRY(c, c->temporal_var.end(s));
    temporal_stored(c, P, K, true);
    out.color = out.length = &P.col;
    out.moments = &P.mom;
    out.filtered = filter;
    if (!filter) return RT_OK;
    const TvPending pend{V.t.p_col, V.p_mom};
    return denoise_var_passes(c, dv, s, rgba, out, &pend);
}

// A host entry point: run(stream, rgba, out) is the pass, on the context's
// stream, with dn_rgba for its RGBA when the caller wants the image; then the
// host copies of what it left in `out`
template <class Run>
int host_call(rt_context* c, uint8_t* rgba_out, float* color_out, float* length_out, const Run& run,
              Result* kept = nullptr) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const size_t npix = (size_t)c->height * c->width;
    if (rgba_out) {
        if (!c->cpu) HIP_TRY(c, hipSetDevice(c->device));
        if (const int rc = ensure_buf(c, c->dn_rgba, npix * 4, "host RGBA for %zu pixels", npix)) return rc;
    }
    Result out;
    if (const int rc = run(c->stream, rgba_out ? c->dn_rgba.as<unsigned>() : nullptr, out)) return rc;
    if (kept) *kept = out;
    return read_back(c, npix, rgba_out, out.color, color_out, out.length, length_out);
}

// The host form of rt_temporal_var and rt_temporal_var_counted: the pass, the
// host copies, and moments_out
int temporal_var_host(rt_context* c, const rt_temporal_params* tp, const rt_denoise_var_params* dv, uint8_t* rgba_out,
                      float* color_out, float* length_out, float* moments_out, bool counted) {
    Result res;
    int rc = host_call(c, rgba_out, color_out, length_out, [&](hipStream_t s, unsigned* rgba, Result& out) {
        return temporal_var_pass(c, tp, dv, s, rgba, out, counted);
    }, &res);
    if (rc || !moments_out) return rc;
    // {variance of the mean, dof}: the pending planes, and behind a filter its final .w
    const HostFpEnv fp;
    const size_t npix = (size_t)c->height * c->width;
    const float2* mom = res.moments->as<float2>();
    const float4* len = res.length->as<float4>();
    const float4* var = res.filtered ? res.color->as<float4>() : nullptr;
    std::vector<float2> hm;
    std::vector<float4> hv;
    if (!c->cpu) {  // (read_back has synchronised the stream: the buffers are settled)
        if (!try_resize(hm, npix) || !try_resize(hv, npix))
            return fail(c, RT_ERR_OUT_OF_MEMORY, "host moments for %zu pixels", npix);
        HIP_TRY(c, hipMemcpyAsync(hm.data(), mom, npix * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(hv.data(), var ? var : len, npix * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        mom = hm.data();
        len = hv.data();
        if (var) var = hv.data();
    }
    for (size_t i = 0; i < npix; i++) {
        moments_out[2 * i] = var ? var[i].w : tv_var_of_mean(mom[i], len[i].w);
        moments_out[2 * i + 1] = mom[i].y;
    }
    return RT_OK;
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
    return host_call(c, rgba_out, color_out, nullptr, [&](hipStream_t s, unsigned* rgba, Result& out) {
        return denoise_levels(c, dp, s, rgba, out);
    });
}

int rt_denoise_device(rt_context* c, const rt_denoise_params* dp, void* rgba_device, void* stream) {
    hipStream_t s;
    Result out;
    const int rc = device_call(c, "rt_denoise_device", {{rgba_device, "rgba_device", false}}, stream, &s);
    return rc ? rc : denoise_levels(c, dp, s, (unsigned*)rgba_device, out);
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
    return host_call(c, rgba_out, color_out, var_out, [&](hipStream_t s, unsigned* rgba, Result& out) {
        return denoise_var_passes(c, dp, s, rgba, out);
    });
}

int rt_denoise_var_device(rt_context* c, const rt_denoise_var_params* dp, void* rgba_device, void* stream) {
    hipStream_t s;
    Result out;
    const int rc = device_call(c, "rt_denoise_var_device", {{rgba_device, "rgba_device", false}}, stream, &s);
    return rc ? rc : denoise_var_passes(c, dp, s, (unsigned*)rgba_device, out);
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
    return host_call(c, rgba_out, color_out, length_out, [&](hipStream_t s, unsigned* rgba, Result& out) {
        return temporal_pass(c, tp, dn, s, rgba, out);
    });
}

int rt_temporal_device(rt_context* c, const rt_temporal_params* tp, const rt_denoise_params* dn, void* rgba_device,
                       void* stream) {
    hipStream_t s;
    Result out;
    const int rc = device_call(c, "rt_temporal_device", {{rgba_device, "rgba_device", false}}, stream, &s);
    return rc ? rc : temporal_pass(c, tp, dn, s, (unsigned*)rgba_device, out);
}

int rt_temporal_reset(rt_context* c) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    // roles only: work still queued on the buffers is ordered by the next call's stream waits
    c->vs.drop_history();
    return RT_OK;
}

float rt_last_temporal_ms(rt_context* c) { return c ? c->temporal.elapsed_ms() : -1.0f; }

// ---- temporal reprojection of the luminance moments ----------------------------
// (csrc/rt_temporal_var.h has the arithmetic)

int rt_temporal_var(rt_context* c, const rt_temporal_params* tp, const rt_denoise_var_params* dv, uint8_t* rgba_out,
                    float* color_out, float* length_out, float* moments_out) {
    return temporal_var_host(c, tp, dv, rgba_out, color_out, length_out, moments_out, false);
}

int rt_temporal_var_device(rt_context* c, const rt_temporal_params* tp, const rt_denoise_var_params* dv,
                           void* rgba_device, void* stream) {
    hipStream_t s;
    Result out;
    const int rc = device_call(c, "rt_temporal_var_device", {{rgba_device, "rgba_device", false}}, stream, &s);
    return rc ? rc : temporal_var_pass(c, tp, dv, s, (unsigned*)rgba_device, out);
}

// The count-aware form: rt_temporal_var's signatures
int rt_temporal_var_counted(rt_context* c, const rt_temporal_params* tp, const rt_denoise_var_params* dv,
                            uint8_t* rgba_out, float* color_out, float* length_out, float* moments_out) {
    return temporal_var_host(c, tp, dv, rgba_out, color_out, length_out, moments_out, true);
}

int rt_temporal_var_counted_device(rt_context* c, const rt_temporal_params* tp, const rt_denoise_var_params* dv,
                                   void* rgba_device, void* stream) {
    hipStream_t s;
    Result out;
    const int rc = device_call(c, "rt_temporal_var_counted_device", {{rgba_device, "rgba_device", false}}, stream, &s);
    return rc ? rc : temporal_var_pass(c, tp, dv, s, (unsigned*)rgba_device, out, true);
}

float rt_last_temporal_var_ms(rt_context* c) { return c ? c->temporal_var.elapsed_ms() : -1.0f; }

// ---- luminance moment tracking ------------------------------------------------
// (csrc/rt_moments.h has the update, rt_render.cpp runs
// it behind every render call)

int rt_set_moments(rt_context* c, int enable) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    // off ends the tracking; on starts not live (a render of frame 1 makes it
    // live), also in mid-accumulation.  The buffers stay for the next use.
    c->st.set_tracking(enable != 0);
    return RT_OK;
}

int rt_get_moments(const rt_context* c) { return c && c->st.tracking() ? 1 : 0; }

int rt_moments_batches(const rt_context* c) { return c ? (int)c->st.batches() : 0; }

int rt_get_variance(rt_context* c, float* var_out, float* lum_out) {
    const HostFpEnv fp;
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const unsigned J = c->st.batches();
    // (a non-uniform state on a one-batch base, rt_render_adaptive_reprojected's, has pixels with
    // J_p = 2 and more: they report; a pixel still at J_p = 1 has no estimate and reports ad_var's
    // own value there, M2 * inf, which is not finite: NaN for the M2 = 0 of a single batch)
    if (J < 2u && !(J == 1u && c->st.nonuniform()))
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "no variance yet: moment tracking %s, %u batches (needs rt_set_moments and two render calls "
                    "of one accumulation)",
                    J ? "live" : "not live", J);
    const size_t npix = (size_t)c->rows * c->width;
    const float2* m = c->mom_m.as<float2>();
    const uint2* cn = own_counts(c);  // non-uniform: each pixel's own {n_p, J_p}
    std::vector<float2> host;
    std::vector<uint2> host_cn;
    if (!c->cpu) {
        if (!try_resize(host, npix) || (cn && !try_resize(host_cn, npix)))
            return fail(c, RT_ERR_OUT_OF_MEMORY, "host moments for %zu pixels", npix);
        // behind the last render (and its update pass), on whatever stream it ran
        const int rc = read_settled(c, {{host.data(), m, npix * sizeof(float2)},
                                        {cn ? host_cn.data() : nullptr, cn, npix * sizeof(uint2)}});
        if (rc) return rc;
        m = host.data();
        if (cn) cn = host_cn.data();
    }
    // M2 / ((J - 1) n): the selection's own expression, n the frames accumulated
    const uint2 uniform = make_uint2(c->st.tracked_frames(), J);
    for (size_t i = 0; i < npix; i++) {
        const uint2 nj = cn ? cn[i] : uniform;
        if (var_out) var_out[i] = ad_var(m[i].y, nj.x, nj.y);
        if (lum_out) lum_out[i] = m[i].x;
    }
    return RT_OK;
}

}  // extern "C"
