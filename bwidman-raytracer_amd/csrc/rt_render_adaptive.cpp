// rt_render_adaptive.cpp — variance-driven adaptive sampling at the C ABI
// (include/rt_abi.h): rt_render_adaptive*, rt_adaptive_last_stats,
// rt_get_counts.  csrc/rt_adaptive.h has the selection's arithmetic,
// rt_adaptive.hip and rt_kernel_list.h the kernels, rt_cpu.cpp their host twins.
//
// One call is, on one stream and inside one render pass (so every later call
// is ordered after all of it): [count fill, the first call of an accumulation]
// row sums, column sums + test + scan + scatter, the list render kernel, the
// moment update of the listed pixels, the resolve pass.  The list and its
// length never leave the device.
#include <cmath>

#include "rt_context.h"

namespace {

int params_check(rt_context* c, const rt_adaptive_params* p, int& max_bounces) {
    if (!c || !p) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!c->has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    if (p->samples < 1 || !(p->tolerance > 0.0f) || !(p->lum_floor >= 0.0f) || std::isinf(p->lum_floor) ||
        p->radius < 0 || p->radius > RT_ADAPTIVE_MAX_RADIUS)
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "bad adaptive params: samples %d (>= 1), tolerance %g (> 0), lum_floor %g (>= 0, finite), "
                    "radius %d (0..%d)",
                    p->samples, (double)p->tolerance, (double)p->lum_floor, p->radius, RT_ADAPTIVE_MAX_RADIUS);
    if (max_bounces < 0) max_bounces = c->max_bounces;
    if (max_bounces > RT_MAX_BOUNCES) return fail(c, RT_ERR_UNSUPPORTED, "max_bounces %d > %d", max_bounces, RT_MAX_BOUNCES);
    if (c->precision == RT_PRECISION_REFERENCE_FAST)
        return fail(c, RT_ERR_UNSUPPORTED,
                    "rt_render_adaptive: not in RT_PRECISION_REFERENCE_FAST (a list schedule would be a new "
                    "arithmetic form of that mode)");
    if (c->rng.p && (c->row_offset != 0 || c->row_stride > 1))
        return fail(c, RT_ERR_UNSUPPORTED,
                    "the context holds a row shard (offset %d, stride %d): the selection window needs a full frame",
                    c->row_offset, c->row_stride);
    const rt_accum_state& st = c->st;
    if (st.batches() < 2u || !c->rng.p)
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "rt_render_adaptive needs live moment tracking with at least 2 batches (rt_set_moments and two "
                    "render calls of one accumulation): tracking %s, %u batches",
                    st.batches() ? "live" : "not live", st.batches());
    if (!st.current())
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "rt_render_adaptive: the tracked moments continue at frame %u but the frame counter is %u (the "
                    "accumulation was restarted by a scene, camera or reset call): render first",
                    st.tracked_frames() + 1u, st.frame());
    if (st.adaptive_base() + (unsigned)p->samples > 0xffffffffull)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "frame count overflow");
    return RT_OK;
}

// The buffers of the non-uniform state and of a selection; the arguments of
// this call's passes.  `fresh`: the counts are to be filled first.
int setup(rt_context* c, const rt_adaptive_params* p, rt_ad_args& A, bool& fresh) {
    const size_t npix = (size_t)c->height * c->width;
    const int wpr = (c->width + 63) / 64;
    const size_t nwords = (size_t)wpr * c->height;
    const char* oom = "host adaptive state for %zu pixels";
    int rc = ensure_buf(c, c->ad_cnt, npix * sizeof(uint2), oom, npix);
    if (!rc) rc = ensure_buf(c, c->ad_rows, npix * 3 * sizeof(float), oom, npix);
    if (!rc) rc = ensure_buf(c, c->ad_mask, nwords * sizeof(unsigned long long), oom, npix);
    if (!rc) rc = ensure_buf(c, c->ad_pop, nwords * sizeof(unsigned), oom, npix);
    if (!rc) rc = ensure_buf(c, c->ad_list, npix * sizeof(int), oom, npix);
    if (!rc) rc = ensure_buf(c, c->ad_stat, 16, oom, npix);
    if (rc) return rc;
    fresh = !c->st.nonuniform();
    std::memset(&A, 0, sizeof A);
    A.width = c->width;
    A.height = c->height;
    A.npix = (long)npix;
    A.words_per_row = wpr;
    A.k = p->samples;
    A.radius = p->radius;
    A.tolerance = p->tolerance;
    A.lum_floor = p->lum_floor;
    A.min_frames = p->min_frames;
    A.max_frames = p->max_frames;
    A.kf = (float)p->samples;
    A.invk = 1.0f / A.kf;
    A.mom_in = c->mom_m.as<float2>();
    A.mom = c->mom_m.as<float2>();
    A.cnt = c->ad_cnt.as<uint2>();
    A.accum = c->accum.as<float>();
    A.prev = c->mom_prev.as<float>();
    A.rowv = c->ad_rows.as<float>();
    A.rowm = A.rowv + npix;
    A.rowc = reinterpret_cast<int*>(A.rowv + 2 * npix);
    A.mask = c->ad_mask.as<unsigned long long>();
    A.pop = c->ad_pop.as<unsigned>();
    A.list = c->ad_list.as<int>();
    A.total = c->ad_stat.as<unsigned long long>();
    A.list_n = reinterpret_cast<unsigned*>(A.total + 1);
    return RT_OK;
}

void kparams(rt_context* c, int samples, int max_bounces, rt_kparams& K) {
    fill_view(c, c->width, c->height, 0, 1, c->rows, K);
    K.samples = samples;
    K.max_bounces = max_bounces;
    K.first_frame = 2u;  // never 1: a listed pixel continues (its frame is n_p + 1, from the counts)
    K.rng = c->rng.as<unsigned>();
    K.accum = c->accum.as<float>();
    K.rgba = nullptr;  // the resolve pass writes the image
}

int cpu_adaptive(rt_context* c, const rt_adaptive_params* p, int max_bounces, float* color) {
    const HostFpEnv fp;
    rt_ad_args A;
    bool fresh = false;
    if (const int rc = setup(c, p, A, fresh)) return rc;
    A.rgba = c->rgba.as<unsigned>();
    A.color = color;
    if (fresh) {
        const uint2 v = make_uint2(c->st.tracked_frames(), c->st.batches());
        for (long i = 0; i < A.npix; i++) A.cnt[i] = v;
        *A.total = (unsigned long long)A.npix * v.x;
    }
    rt_kparams K;
    kparams(c, p->samples, max_bounces, K);
    using clock = std::chrono::steady_clock;
    auto ms = [](clock::time_point a, clock::time_point b) { return std::chrono::duration<float, std::milli>(b - a).count(); };
    (void)c->render.begin(nullptr, true);
    const auto t0 = clock::now();
    rt_cpu_adaptive_select(A, c->threads);
    const auto t1 = clock::now();
    rt_cpu_adaptive_render(K, A, c->threads);
    const auto t2 = clock::now();
    rt_cpu_adaptive_finish(A, c->threads);
    const auto t3 = clock::now();
    (void)c->render.end(nullptr);
    c->ad_cpu_ms[0] = ms(t0, t1);
    c->ad_cpu_ms[1] = ms(t1, t2);
    c->ad_cpu_ms[2] = ms(t2, t3);
    c->ad_cpu_selected = (long long)*A.list_n;
    c->ad_cpu_total = (long long)*A.total;
    c->st.adaptive_done(p->samples);
    return RT_OK;
}

// The GPU call on stream s; rgba / color: device pointers or null
int gpu_adaptive(rt_context* c, const rt_adaptive_params* p, int max_bounces, unsigned* rgba, float* color,
                 hipStream_t s) {
    const HostFpEnv fp;
    HIP_TRY(c, hipSetDevice(c->device));
    rt_ad_args A;
    bool fresh = false;
    if (const int rc = setup(c, p, A, fresh)) return rc;
    A.rgba = rgba;
    A.color = color;
    rt_kparams K;
    kparams(c, p->samples, max_bounces, K);
    const int which = c->ad_kernel;
    if (rt_render_list_queued(K, which) && (c->grec == 1 || (c->grec < 0 && rt_render_wants_global_records(K, c->num_cus)))) {
        if (const int rc = ensure_buf(c, c->rec, rt_render_rec_floats(K) * sizeof(float))) return rc;
        K.rec = c->rec.as<float>();
    }
    const bool timed = c->ktiming;
    if (timed)
        for (hipEvent_t& e : c->ad_ev)
            if (!e) HIP_TRY(c, hipEventCreate(&e));
    if (const int rc = order_after_all(c, s)) return rc;
    rt_launched_kernel[0] = 0;
    HIP_TRY(c, c->render.begin(s, c->ktiming));
    c->ad_timed = false;
    if (timed) HIP_TRY(c, hipEventRecord(c->ad_ev[0], s));
    hipError_t e = hipSuccess;
    if (fresh) e = rt_launch_adaptive_fill(A.cnt, A.total, A.npix, c->st.tracked_frames(), c->st.batches(), s);
    if (e == hipSuccess) e = rt_launch_adaptive(A, 0, s);
    if (e == hipSuccess) e = rt_launch_adaptive(A, 1, s);
    if (e == hipSuccess && timed) e = hipEventRecord(c->ad_ev[1], s);
    const rt_list_args L = {A.list, A.list_n, A.cnt};
    if (e == hipSuccess) e = rt_launch_render_list(K, L, c->num_cus, which, s);
    c->kernel_name = rt_launched_kernel;
    if (e == hipSuccess && timed) e = hipEventRecord(c->ad_ev[2], s);
    if (e == hipSuccess) e = rt_launch_adaptive(A, 2, s);
    if (e == hipSuccess) e = rt_launch_adaptive(A, 3, s);
    if (e == hipSuccess && timed) e = hipEventRecord(c->ad_ev[3], s);
    if (e != hipSuccess) {
        // what ran is unknown: the moments and counts no longer describe frameSum
        c->st.end_tracking();
        (void)c->render.end(s);
        return hip_fail(c, e, "rt_render_adaptive launch");
    }
    HIP_TRY(c, c->render.end(s));
    c->ad_timed = timed;
    c->st.adaptive_done(p->samples);
    return RT_OK;
}

int read_stats(rt_context* c, rt_adaptive_stats* st) {
    if (!c || !st) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!c->st.nonuniform()) return fail(c, RT_ERR_INVALID_ARGUMENT, "no adaptive call in this accumulation");
    if (c->cpu) {
        st->selected = c->ad_cpu_selected;
        st->frames_total = c->ad_cpu_total;
        st->select_ms = c->ad_cpu_ms[0];
        st->render_ms = c->ad_cpu_ms[1];
        st->resolve_ms = c->ad_cpu_ms[2];
        return RT_OK;
    }
    unsigned long long h[2] = {0, 0};
    if (const int rc = read_settled(c, {{h, c->ad_stat.p, sizeof h}})) return rc;
    st->frames_total = (long long)h[0];
    st->selected = (long long)(unsigned)h[1];
    st->select_ms = st->render_ms = st->resolve_ms = -1.0f;
    if (c->ad_timed && hipEventSynchronize(c->ad_ev[3]) == hipSuccess) {
        float* out[3] = {&st->select_ms, &st->render_ms, &st->resolve_ms};
        for (int i = 0; i < 3; i++)
            if (hipEventElapsedTime(out[i], c->ad_ev[i], c->ad_ev[i + 1]) != hipSuccess) *out[i] = -1.0f;
    }
    return RT_OK;
}

}  // namespace

extern "C" {

rt_adaptive_params rt_adaptive_params_default(void) {
    rt_adaptive_params d;
    // the values of the CPU emulation that motivated the feature (DESIGN.md
    // section 14): equal error with about 0.67 of the samples
    d.samples = 8;
    d.tolerance = 0.1f;
    d.lum_floor = 0.01f;
    d.radius = 2;
    d.min_frames = 0u;
    d.max_frames = 0u;
    return d;
}

int rt_render_adaptive(rt_context* c, const rt_adaptive_params* p, int max_bounces, uint8_t* rgba_out, float* color_out,
                       rt_adaptive_stats* stats_out) {
    if (const int rc = params_check(c, p, max_bounces)) return rc;
    const size_t npix = (size_t)c->height * c->width;
    if (c->cpu) {
        if (const int rc = cpu_adaptive(c, p, max_bounces, color_out)) return rc;
        if (rgba_out) std::memcpy(rgba_out, c->rgba.p, npix * 4);
        return stats_out ? read_stats(c, stats_out) : RT_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_buf(c, c->rgba, npix * 4);
    if (!rc && color_out) rc = ensure_buf(c, c->ad_color, npix * 3 * sizeof(float));
    if (rc) return rc;
    rc = gpu_adaptive(c, p, max_bounces, c->rgba.as<unsigned>(), color_out ? c->ad_color.as<float>() : nullptr, c->stream);
    if (rc) return rc;
    if (rgba_out) HIP_TRY(c, hipMemcpyAsync(rgba_out, c->rgba.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (color_out)
        HIP_TRY(c, hipMemcpyAsync(color_out, c->ad_color.p, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return stats_out ? read_stats(c, stats_out) : RT_OK;
}

int rt_render_adaptive_device(rt_context* c, const rt_adaptive_params* p, int max_bounces, void* rgba_device,
                              void* stream) {
    if (c && c->cpu) return fail(c, RT_ERR_UNSUPPORTED, "rt_render_adaptive_device: CPU context");
    if (const int rc = params_check(c, p, max_bounces)) return rc;
    if (rgba_device && ((uintptr_t)rgba_device & 3u))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "rgba_device not 4-byte aligned");
    return gpu_adaptive(c, p, max_bounces, (unsigned*)rgba_device, nullptr, stream ? (hipStream_t)stream : c->stream);
}

int rt_adaptive_last_stats(rt_context* c, rt_adaptive_stats* stats_out) { return read_stats(c, stats_out); }

int rt_get_counts(rt_context* c, uint32_t* frames_out, uint32_t* batches_out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (!c->rng.p) return fail(c, RT_ERR_INVALID_ARGUMENT, "no shard state (render or rt_init_rand first)");
    const size_t npix = (size_t)c->rows * c->width;
    if (!c->st.nonuniform()) {  // uniform: the context's counts
        const uint32_t n = c->st.frames(), J = c->st.batches();
        for (size_t i = 0; i < npix; i++) {
            if (frames_out) frames_out[i] = n;
            if (batches_out) batches_out[i] = J;
        }
        return RT_OK;
    }
    const uint2* cn = c->ad_cnt.as<uint2>();
    std::vector<uint2> host;
    if (!c->cpu) {
        if (!try_resize(host, npix)) return fail(c, RT_ERR_OUT_OF_MEMORY, "host counts for %zu pixels", npix);
        if (const int rc = read_settled(c, {{host.data(), cn, npix * sizeof(uint2)}})) return rc;
        cn = host.data();
    }
    for (size_t i = 0; i < npix; i++) {
        if (frames_out) frames_out[i] = cn[i].x;
        if (batches_out) batches_out[i] = cn[i].y;
    }
    return RT_OK;
}

}  // extern "C"
