// rt_render_adaptive.cpp — variance-driven adaptive sampling at the C ABI
// (include/rt_abi.h): rt_render_adaptive*, rt_adaptive_last_stats,
// rt_get_counts, and the two-phase form on row shards (rt_adaptive_export_rows*,
// rt_render_adaptive_shard*, rt_render_adaptive_multi).
// rt_render_adaptive_reprojected* is the same call with the selection made from
// the pending planes of rt_temporal_var (a moving camera: DESIGN.md section 22).
// csrc/rt_adaptive.h has the selection's arithmetic, rt_adaptive.hip and
// rt_kernel_list.h the kernels, rt_cpu.cpp their host twins.
//
// One call is, on one stream and inside one render pass (so every later call
// is ordered after all of it): [count fill, the first call of an accumulation]
// row sums, column sums + test + scan + scatter, the list render kernel, the
// moment update of the listed pixels, the resolve pass.  The list and its
// length never leave the device.
//
// On row shards the row sums are phase 1 (rt_adaptive_export_rows: the shard's
// own rows into its block, nothing of the accumulation's state changes) and the
// rest is phase 2 (rt_render_adaptive_shard), whose test reads the column taps
// from the ranks' gathered blocks; every pass behind the test is the full
// frame's over the shard's rows * width.
#include <cmath>

#include "rt_group.h"

namespace {

// min_batches: 2 for the selection from the tracked moments (its variance needs
// two), 1 for the selection from the pending planes
int params_check(rt_context* c, const rt_adaptive_params* p, int& max_bounces, bool shard_ok = false,
                 unsigned min_batches = 2u) {
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
    if (!shard_ok && c->rng.p && c->holds_shard())
        return fail(c, RT_ERR_UNSUPPORTED,
                    "the context holds a row shard (offset %d, stride %d): the selection window needs a full frame",
                    c->row_offset, c->row_stride);
    const rt_accum_state& st = c->st;
    if (st.batches() < min_batches || !c->rng.p)
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "rt_render_adaptive needs live moment tracking with at least %u batches (rt_set_moments and %s "
                    "of one accumulation): tracking %s, %u batches",
                    min_batches, min_batches >= 2u ? "two render calls" : "a render call",
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
    const size_t npix = (size_t)c->rows * c->width;  // the context's pixel state: the frame, or its row shard
    const int wpr = (c->width + 63) / 64;
    const size_t nwords = (size_t)wpr * c->rows;
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
    A.height = c->rows;
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
    fill_view(c, c->width, c->height, c->row_offset, c->row_stride > 1 ? c->row_stride : 1, c->rows, K);
    K.samples = samples;
    K.max_bounces = max_bounces;
    K.first_frame = 2u;  // never 1: a listed pixel continues (its frame is n_p + 1, from the counts)
    K.rng = c->rng.as<unsigned>();
    K.accum = c->accum.as<float>();
    K.rgba = nullptr;  // the resolve pass writes the image
}

// The ranks' gathered row-sum blocks of a phase 2 (p null: a full-frame call,
// which makes its own row sums), or (col non-null, a full-frame call) the
// pending planes that rt_render_adaptive_reprojected selects from
struct Gathered {
    const float* p = nullptr;
    int shards = 0, rows_per_shard = 0;
    const float4* col = nullptr;
    const float2* mom = nullptr;
    const float4* ga = nullptr;
    float min_dof = 0.0f;
};

rt_ad_reproj_args reproj_args(const rt_ad_args& A, const Gathered& g) {
    rt_ad_reproj_args R;
    R.A = A;
    R.p_col = g.col;
    R.p_mom = g.mom;
    R.p_ga = g.ga;
    R.min_dof = g.min_dof;
    return R;
}

rt_ad_shard_args shard_args(const rt_context* c, const rt_ad_args& A, const Gathered& g) {
    rt_ad_shard_args S;
    S.A = A;
    S.gathered = g.p;
    S.shards = g.shards;
    S.rows_per_shard = g.rows_per_shard;
    S.image_height = c->height;
    S.row_offset = c->row_offset;
    return S;
}

int cpu_adaptive(rt_context* c, const rt_adaptive_params* p, int max_bounces, float* color, const Gathered& g) {
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
    if (g.p)
        rt_cpu_adaptive_select_shard(shard_args(c, A, g), c->threads);
    else if (g.col)
        rt_cpu_adaptive_select_reproj(reproj_args(A, g), c->threads);
    else
        rt_cpu_adaptive_select(A, c->threads);
    const auto t1 = clock::now();
    rt_cpu_adaptive_render(K, c->nee_args(K.max_bounces), A, c->threads);
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
                 hipStream_t s, const Gathered& g) {
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
    const rt_nee_args N = c->nee_args(K.max_bounces);  // a table: the list render is the NEE kernel's
    if (!N.n_lights && rt_render_list_queued(K, which) && (c->grec == 1 || (c->grec < 0 && rt_render_wants_global_records(K, c->num_cus)))) {
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
    if (e == hipSuccess && g.col) {
        e = rt_launch_adaptive_reproj(reproj_args(A, g), s);
    } else {
        if (e == hipSuccess && !g.p) e = rt_launch_adaptive(A, 0, s);
        if (e == hipSuccess) e = g.p ? rt_launch_adaptive_shard(shard_args(c, A, g), s) : rt_launch_adaptive(A, 1, s);
    }
    if (e == hipSuccess && timed) e = hipEventRecord(c->ad_ev[1], s);
    const rt_list_args L = {A.list, A.list_n, A.cnt};
    if (e == hipSuccess)
        e = N.n_lights ? rt_launch_render_nee(K, N, &L, c->num_cus, 0, s) : rt_launch_render_list(K, L, c->num_cus, which, s);
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

// What rt_render_adaptive_reprojected needs: rt_render_adaptive's conditions
// with one tracked batch, min_dof, and a pending temporal set of the current
// view that carries moments; g then names its planes.  A refusal touches nothing.
int reprojected_check(rt_context* c, const rt_adaptive_reprojected_params* p, int& max_bounces, Gathered& g,
                      rt_adaptive_params& base) {
    if (!c || !p) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    base = {p->samples, p->tolerance, p->lum_floor, p->radius, p->min_frames, p->max_frames};
    if (const int rc = params_check(c, &base, max_bounces, false, 1u)) return rc;
    if (!(p->min_dof >= 0.0f))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "bad adaptive params: min_dof %g (>= 0)", (double)p->min_dof);
    if (!c->vs.pending_current(c->width, c->height))
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "rt_render_adaptive_reprojected: no pending temporal set of the current view (call "
                    "rt_temporal_var after the render of this view)");
    if (!c->vs.pending_has_moments())
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "rt_render_adaptive_reprojected: the pending temporal set was written by rt_temporal and has no "
                    "moments (call rt_temporal_var)");
    const rt_context::TpSet& P = c->tp[c->vs.pending_set()];
    g = Gathered{};
    g.col = P.col.as<float4>();
    g.mom = P.mom.as<float2>();
    g.ga = P.ga.as<float4>();
    g.min_dof = p->min_dof;
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

// ---- on row shards --------------------------------------------------------------
size_t block_words(const rt_context* c, int rows_per_shard) { return (size_t)3 * (size_t)rows_per_shard * (size_t)c->width; }

// What phase 1 needs besides its destination: rt_render_adaptive's checks minus the shard refusal
int export_rows_check(rt_context* c, const rt_adaptive_params* p, int rows_per_shard) {
    int mb = -1;
    if (const int rc = params_check(c, p, mb, true)) return rc;
    if (const int rc = block_rows_check(c, rows_per_shard)) return rc;
    return block_plane_check(c, rows_per_shard);
}

// Phase 1 of a checked call: the row sums of the context's own rows into
// `block` (device memory on a GPU context, on stream s: after the last render
// and its moment update, and the next render after it, as an rt_export_shard;
// host memory on a CPU context).  In the uniform state the counts the row sums
// read are the context's, written to the scratch the first adaptive call fills
// anyway: nothing a uniform render, rt_export_shard or rt_get_counts reads.
int export_rows_pass(rt_context* c, const rt_adaptive_params* p, int rows_per_shard, float* block, hipStream_t s) {
    const HostFpEnv fp;
    if (!c->cpu) HIP_TRY(c, hipSetDevice(c->device));
    rt_ad_args A;
    bool fresh = false;
    if (const int rc = setup(c, p, A, fresh)) return rc;
    const long plane = (long)rows_per_shard * c->width;
    A.rowv = block;
    A.rowm = block + plane;
    A.rowc = reinterpret_cast<int*>(block + 2 * plane);
    if (c->cpu) {
        if (fresh) {
            const uint2 v = make_uint2(c->st.tracked_frames(), c->st.batches());
            for (long i = 0; i < A.npix; i++) A.cnt[i] = v;
        }
        (void)c->xport.begin(nullptr, false);
        rt_cpu_adaptive_rows_block(A, plane, c->threads);
        (void)c->xport.end(nullptr);
    } else {
        HIP_TRY(c, c->xport.create(false));
        if (const int rc = order_after_all(c, s)) return rc;
        if (fresh)
            HIP_TRY(c, rt_launch_adaptive_fill(A.cnt, A.total, A.npix, c->st.tracked_frames(), c->st.batches(), s));
        HIP_TRY(c, rt_launch_adaptive_rows_block(A, plane, s));
        HIP_TRY(c, c->xport.end(s));
    }
    c->st.export_done(p->radius);
    return RT_OK;
}

// What phase 2 needs besides its source and destinations
int shard_call_check(rt_context* c, const rt_adaptive_params* p, int& max_bounces, const void* gathered, int shards,
                     int rows_per_shard) {
    if (!c || !p || !gathered) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (const int rc = params_check(c, p, max_bounces, true)) return rc;
    if (!c->st.export_current(p->radius))
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "rt_render_adaptive_shard: no current rt_adaptive_export_rows of this context with radius %d (none "
                    "was made, or a render, reset, scene or camera call came since)",
                    p->radius);
    if (shards != (c->row_stride > 1 ? c->row_stride : 1))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "shards %d is not the context's row stride %d", shards,
                    c->row_stride > 1 ? c->row_stride : 1);
    if (const int rc = block_cover_check(c, "gather", shards, rows_per_shard)) return rc;
    return block_plane_check(c, rows_per_shard);
}

// Phase 2 of a checked call on the host forms' path: `gathered` is host memory
// (staged to the device on a GPU context), the outputs are the shard's rows in
// shard order; synchronous
int shard_call_host(rt_context* c, const rt_adaptive_params* p, int max_bounces, const float* gathered, int shards,
                    int rows_per_shard, uint8_t* rgba_out, float* color_out, bool sync) {
    const size_t npix = (size_t)c->rows * c->width;
    if (c->cpu) {
        if (const int rc = cpu_adaptive(c, p, max_bounces, color_out, {gathered, shards, rows_per_shard})) return rc;
        if (rgba_out) std::memcpy(rgba_out, c->rgba.p, npix * 4);
        return RT_OK;
    }
    const size_t gbytes = (size_t)shards * block_words(c, rows_per_shard) * sizeof(float);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_buf(c, c->rgba, npix * 4);
    if (!rc && color_out) rc = ensure_buf(c, c->ad_color, npix * 3 * sizeof(float));
    if (!rc && gathered != c->ad_gather.p) rc = ensure_buf(c, c->ad_gather, gbytes);
    if (rc) return rc;
    if (gathered != c->ad_gather.p)
        HIP_TRY(c, hipMemcpyAsync(c->ad_gather.p, gathered, gbytes, hipMemcpyHostToDevice, c->stream));
    rc = gpu_adaptive(c, p, max_bounces, c->rgba.as<unsigned>(), color_out ? c->ad_color.as<float>() : nullptr, c->stream,
                      {c->ad_gather.as<float>(), shards, rows_per_shard});
    if (rc) return rc;
    if (rgba_out) HIP_TRY(c, hipMemcpyAsync(rgba_out, c->rgba.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (color_out)
        HIP_TRY(c, hipMemcpyAsync(color_out, c->ad_color.p, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (sync) HIP_TRY(c, hipStreamSynchronize(c->stream));
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
        if (const int rc = cpu_adaptive(c, p, max_bounces, color_out, {})) return rc;
        if (rgba_out) std::memcpy(rgba_out, c->rgba.p, npix * 4);
        return stats_out ? read_stats(c, stats_out) : RT_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_buf(c, c->rgba, npix * 4);
    if (!rc && color_out) rc = ensure_buf(c, c->ad_color, npix * 3 * sizeof(float));
    if (rc) return rc;
    rc = gpu_adaptive(c, p, max_bounces, c->rgba.as<unsigned>(), color_out ? c->ad_color.as<float>() : nullptr, c->stream, {});
    if (rc) return rc;
    if (rgba_out) HIP_TRY(c, hipMemcpyAsync(rgba_out, c->rgba.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (color_out)
        HIP_TRY(c, hipMemcpyAsync(color_out, c->ad_color.p, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return stats_out ? read_stats(c, stats_out) : RT_OK;
}

int rt_render_adaptive_device(rt_context* c, const rt_adaptive_params* p, int max_bounces, void* rgba_device,
                              void* stream) {
    if (const int rc = device_ctx(c, "rt_render_adaptive_device")) return rc;
    if (const int rc = params_check(c, p, max_bounces)) return rc;
    if (const int rc = device_aligned(c, {{rgba_device, "rgba_device", false}})) return rc;
    return gpu_adaptive(c, p, max_bounces, (unsigned*)rgba_device, nullptr, device_stream(c, stream), {});
}

// ---- selection from the reprojected variance -----------------------------------
// (csrc/rt_adaptive.h has the selection)

rt_adaptive_reprojected_params rt_adaptive_reprojected_params_default(void) {
    rt_adaptive_reprojected_params d;
    const rt_adaptive_params a = rt_adaptive_params_default();
    d.samples = a.samples;
    d.tolerance = a.tolerance;
    d.lum_floor = a.lum_floor;
    d.radius = a.radius;
    d.min_frames = a.min_frames;
    d.max_frames = a.max_frames;
    // tools/adaptive_temporal_sweep.py (profiles/adaptive_temporal/sweep.txt): the row
    // with the smallest mean ratio to uniform renders at equal frames.  rt_temporal_var's estimate is
    // biased high under motion, so the tolerance is far above rt_adaptive_params_default()'s, and the
    // window adds nothing there: the term that decides is `fresh`, below four degrees of freedom
    d.tolerance = 0.4f;
    d.radius = 0;
    d.min_dof = 4.0f;
    return d;
}

int rt_render_adaptive_reprojected(rt_context* c, const rt_adaptive_reprojected_params* p, int max_bounces,
                                   uint8_t* rgba_out, float* color_out, rt_adaptive_stats* stats_out) {
    Gathered g{};
    rt_adaptive_params base;
    if (const int rc = reprojected_check(c, p, max_bounces, g, base)) return rc;
    const size_t npix = (size_t)c->height * c->width;
    if (c->cpu) {
        if (const int rc = cpu_adaptive(c, &base, max_bounces, color_out, g)) return rc;
        if (rgba_out) std::memcpy(rgba_out, c->rgba.p, npix * 4);
        return stats_out ? read_stats(c, stats_out) : RT_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_buf(c, c->rgba, npix * 4);
    if (!rc && color_out) rc = ensure_buf(c, c->ad_color, npix * 3 * sizeof(float));
    if (rc) return rc;
    rc = gpu_adaptive(c, &base, max_bounces, c->rgba.as<unsigned>(), color_out ? c->ad_color.as<float>() : nullptr,
                      c->stream, g);
    if (rc) return rc;
    if (rgba_out) HIP_TRY(c, hipMemcpyAsync(rgba_out, c->rgba.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (color_out)
        HIP_TRY(c, hipMemcpyAsync(color_out, c->ad_color.p, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return stats_out ? read_stats(c, stats_out) : RT_OK;
}

int rt_render_adaptive_reprojected_device(rt_context* c, const rt_adaptive_reprojected_params* p, int max_bounces,
                                          void* rgba_device, void* stream) {
    if (const int rc = device_ctx(c, "rt_render_adaptive_reprojected_device")) return rc;
    Gathered g{};
    rt_adaptive_params base;
    if (const int rc = reprojected_check(c, p, max_bounces, g, base)) return rc;
    if (const int rc = device_aligned(c, {{rgba_device, "rgba_device", false}})) return rc;
    return gpu_adaptive(c, &base, max_bounces, (unsigned*)rgba_device, nullptr, device_stream(c, stream), g);
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

int rt_adaptive_export_rows(rt_context* c, const rt_adaptive_params* p, int rows_per_shard, float* block_host) {
    if (!c || !p || !block_host) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    int rc = export_rows_check(c, p, rows_per_shard);
    if (rc) return rc;
    if (c->cpu) return export_rows_pass(c, p, rows_per_shard, block_host, nullptr);
    const size_t bytes = block_words(c, rows_per_shard) * sizeof(float);
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_buf(c, c->ad_block, bytes))) return rc;
    if ((rc = export_rows_pass(c, p, rows_per_shard, c->ad_block.as<float>(), c->stream))) return rc;
    HIP_TRY(c, hipMemcpyAsync(block_host, c->ad_block.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

int rt_adaptive_export_rows_device(rt_context* c, const rt_adaptive_params* p, int rows_per_shard, void* block_device,
                                   void* stream) {
    if (!p) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    hipStream_t s;
    if (const int rc = device_call(c, "rt_adaptive_export_rows_device", {{block_device, "block_device", true}}, stream, &s))
        return rc;
    if (const int rc = export_rows_check(c, p, rows_per_shard)) return rc;
    return export_rows_pass(c, p, rows_per_shard, (float*)block_device, s);
}

int rt_render_adaptive_shard(rt_context* c, const rt_adaptive_params* p, int max_bounces, const float* gathered_host,
                             int shards, int rows_per_shard, uint8_t* rgba_out, float* color_out,
                             rt_adaptive_stats* stats_out) {
    if (const int rc = shard_call_check(c, p, max_bounces, gathered_host, shards, rows_per_shard)) return rc;
    if (const int rc = shard_call_host(c, p, max_bounces, gathered_host, shards, rows_per_shard, rgba_out, color_out, true))
        return rc;
    return stats_out ? read_stats(c, stats_out) : RT_OK;
}

int rt_render_adaptive_shard_device(rt_context* c, const rt_adaptive_params* p, int max_bounces,
                                    const void* gathered_device, int shards, int rows_per_shard, void* rgba_device,
                                    void* stream) {
    if (const int rc = device_ctx(c, "rt_render_adaptive_shard_device")) return rc;
    if (const int rc = shard_call_check(c, p, max_bounces, gathered_device, shards, rows_per_shard)) return rc;
    const int rc = device_aligned(c, {{gathered_device, "gathered_device", true}, {rgba_device, "rgba_device", false}});
    if (rc) return rc;
    return gpu_adaptive(c, p, max_bounces, (unsigned*)rgba_device, nullptr, device_stream(c, stream),
                        {(const float*)gathered_device, shards, rows_per_shard});
}

int rt_render_adaptive_multi(rt_context* const* ctxs, int n, const rt_adaptive_params* p, int max_bounces,
                             uint8_t* rgba_out, rt_adaptive_stats* stats_out) {
    if (!ctxs || n <= 0 || !ctxs[0]) return RT_ERR_INVALID_ARGUMENT;
    rt_context* d = ctxs[0];
    if (!p) return fail(d, RT_ERR_INVALID_ARGUMENT, "null argument");
    // every condition first: a refusal touches nothing
    if (const int rc = group_scan(ctxs, n, d, "rt_render_adaptive_multi")) return rc;
    const int width = d->width, height = d->height;
    if (width <= 0 || height <= 0)
        return fail(d, RT_ERR_INVALID_ARGUMENT, "no frame shape yet (render or rt_init_rand first)");
    const int active = group_active(n, height), rps = group_rows_per_shard(n, height);
    std::vector<int> bounces;
    if (!try_resize(bounces, (size_t)active)) return fail(d, RT_ERR_OUT_OF_MEMORY, "host state for %d contexts", n);
    for (int i = 0; i < active; i++) {
        rt_context* c = ctxs[i];
        // (a full-frame context's row stride may read 0 or 1)
        if (const int rc = group_shard_check(d, c, i, n, c->row_stride > 1 ? c->row_stride : 1, width, height)) return rc;
        if (const int rc = group_counters_check(d, c, i, d, true)) return rc;
        bounces[(size_t)i] = max_bounces;
        if (const int rc = params_check(c, p, bounces[(size_t)i], true)) {
            if (c != d) (void)fail(d, rc, "context %d: %s", i, c->err.c_str());
            return rc;
        }
        if (const int rc = block_plane_check(d, rps)) return rc;
    }
    const size_t blk = block_words(d, rps);
    const size_t gbytes = (size_t)n * blk * sizeof(float);
    // (from here on a failure at context i leaves work of the contexts before it in flight: group_drain)
    // the gathered blocks: on every GPU context's device; CPU contexts share context 0's
    for (int i = 0; i < (d->cpu ? 1 : active); i++) {
        rt_context* c = ctxs[i];
        if (!c->cpu && hipSetDevice(c->device) != hipSuccess) return fail(c, RT_ERR_HIP, "hipSetDevice");
        if (const int rc = ensure_buf(c, c->ad_gather, gbytes, "host gathered row sums (%zu words)", (size_t)n * blk))
            return rc;
    }
    // phase 1 into the context's own slot, then that block to every other context
    for (int i = 0; i < active; i++) {
        rt_context* c = ctxs[i];
        float* own = (c->cpu ? d : c)->ad_gather.as<float>() + (size_t)i * blk;
        if (const int rc = export_rows_pass(c, p, rps, own, c->stream)) return group_drain(ctxs, i + 1, rc);
        for (int j = 0; j < active && !c->cpu; j++) {
            if (j == i) continue;
            rt_context* o = ctxs[j];
            float* dst = o->ad_gather.as<float>() + (size_t)i * blk;
            const hipError_t e = group_copy(dst, o, own, c, blk * sizeof(float));
            if (e != hipSuccess) return group_drain(ctxs, i + 1, hip_fail(c, e, "block copy"));
        }
    }
    // every block is in place before a phase 2 is queued (the call synchronises anyway)
    if (const int rc = group_sync(ctxs, active)) return rc;
    for (int i = 0; i < active; i++) {
        rt_context* c = ctxs[i];
        const float* g = (c->cpu ? d : c)->ad_gather.as<float>();
        if (const int rc = shard_call_host(c, p, bounces[(size_t)i], g, n, rps, nullptr, nullptr, false))
            return group_drain(ctxs, i + 1, rc);
        if (!rgba_out) continue;
        // the shard's rows to their image rows: row j of context i is row i + j * n
        uint8_t* dst = rgba_out + (size_t)i * width * 4;
        if (c->cpu) {
            for (int j = 0; j < c->rows; j++)
                std::memcpy(dst + (size_t)j * n * width * 4, c->rgba.as<uint8_t>() + (size_t)j * width * 4, (size_t)width * 4);
        } else {
            const hipError_t e = hipMemcpy2DAsync(dst, (size_t)n * width * 4, c->rgba.p, (size_t)width * 4, (size_t)width * 4,
                                                  (size_t)c->rows, hipMemcpyDeviceToHost, c->stream);
            if (e != hipSuccess) return group_drain(ctxs, i + 1, hip_fail(c, e, "hipMemcpy2DAsync"));
        }
    }
    rt_adaptive_stats sum = {0, 0, -1.0f, -1.0f, -1.0f};
    if (const int rc = group_sync(ctxs, active)) return rc;
    for (int i = 0; i < active && stats_out; i++) {
        rt_context* c = ctxs[i];
        rt_adaptive_stats st;
        if (const int rc = read_stats(c, &st)) return group_drain(ctxs, active, rc);
        sum.selected += st.selected;
        sum.frames_total += st.frames_total;
        sum.select_ms = st.select_ms > sum.select_ms ? st.select_ms : sum.select_ms;
        sum.render_ms = st.render_ms > sum.render_ms ? st.render_ms : sum.render_ms;
        sum.resolve_ms = st.resolve_ms > sum.resolve_ms ? st.resolve_ms : sum.resolve_ms;
    }
    if (stats_out) *stats_out = sum;
    return RT_OK;
}

}  // extern "C"
