// rt_render.cpp — the render calls of the C ABI (include/rt_abi.h): kernel
// parameters of a view, the launch policy, rt_render*, single-process
// multi-GPU rendering and the row de-interleave.
//
// Compiled with -ffp-contract=off: the camera prelude (Main.cu:336-338) uses
// the reference's float operations in the reference's order.
#include <cmath>

#include "rt_group.h"

static int prepare(rt_context* c, const rt_render_params* p, rt_kparams& K, unsigned& first) {
    const HostFpEnv fp;
    if (!c || !p) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!c->has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    const int stride = p->row_stride == 0 ? 1 : p->row_stride;
    if (p->width <= 0 || p->height <= 0 || p->samples <= 0 || p->row_offset < 0 || stride < 0 ||
        p->row_offset >= p->height)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "bad render params %dx%d samples %d shard %d/%d", p->width,
                    p->height, p->samples, p->row_offset, stride);
    if (p->max_bounces < 0) return fail(c, RT_ERR_INVALID_ARGUMENT, "max_bounces < 0");
    if (p->max_bounces > RT_MAX_BOUNCES)
        return fail(c, RT_ERR_UNSUPPORTED, "max_bounces %d > %d", p->max_bounces, RT_MAX_BOUNCES);
    if (c->light_sampling && c->precision == RT_PRECISION_REFERENCE_FAST)
        return fail(c, RT_ERR_UNSUPPORTED,
                    "light sampling (rt_set_light_sampling) is not available in RT_PRECISION_REFERENCE_FAST (its "
                    "estimator is specified in exact arithmetic only)");
    if (c->width != p->width || c->height != p->height || c->row_offset != p->row_offset ||
        c->row_stride != stride || !c->rng.p) {
        int rc = rt_init_rand(c, p->width, p->height, p->row_offset, stride);
        if (rc) return rc;
    }
    // a non-uniform accumulation (rt_render_adaptive) ends at a render of
    // frame 1; no uniform render can continue it
    switch (c->st.uniform_start(p->first_frame, p->samples, first)) {
        case rt_accum_state::Start::nonuniform:
            return fail(c, RT_ERR_UNSUPPORTED,
                        "the accumulation is non-uniform (rt_render_adaptive): a uniform render cannot continue it "
                        "(first_frame %u; 1 restarts)", first);
        case rt_accum_state::Start::overflow: return fail(c, RT_ERR_INVALID_ARGUMENT, "frame counter overflow");
        case rt_accum_state::Start::ok: break;
    }
    if (!c->cpu) HIP_TRY(c, hipSetDevice(c->device));

    fill_view(c, p->width, p->height, p->row_offset, stride, c->rows, K);
    K.samples = p->samples;
    K.max_bounces = p->max_bounces;
    K.first_frame = first;
    K.rng = c->rng.as<unsigned>();
    K.accum = c->accum.as<float>();
    return RT_OK;
}

void fill_view(rt_context* c, int width, int height, int row_offset, int stride, int rows, rt_kparams& K) {
    std::memset(&K, 0, sizeof K);
    K.width = width;
    K.height = height;
    K.row_offset = row_offset;
    K.row_stride = stride;
    K.rows = rows;
    // host prelude, Main.cu:336-338
    const rt_camera& cam = c->camera;
    K.cam_pos[0] = cam.position.x;
    K.cam_pos[1] = cam.position.y;
    K.cam_pos[2] = cam.position.z;
    K.screen_z = -(float)(width / 2) / tanf(cam.fov / 2.0f);
    {
        const float cy = cosf(cam.angle[0]), sy = sinf(cam.angle[0]);  // rotationMatrix3DY
        const float cx = cosf(cam.angle[1]), sx = sinf(cam.angle[1]);  // rotationMatrix3DX
        const float L[3][3] = {{cy, 0, sy}, {0, 1, 0}, {-sy, 0, cy}};
        const float U[3][3] = {{1, 0, 0}, {0, cx, -sx}, {0, sx, cx}};
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)  // dot(a.row(i), b.col(j)), Math.cuh:191-199
                K.rot[3 * i + j] = L[i][0] * U[0][j] + L[i][1] * U[1][j] + L[i][2] * U[2][j];
    }
    K.jitter = (float)(0.001 * (width / 1000));  // Main.cu:291
    K.bg[0] = c->background[0];
    K.bg[1] = c->background[1];
    K.bg[2] = c->background[2];
    const rt_compiled_scene& sc = c->scene;
    K.n_sph = sc.n_sph;
    K.n_pln = sc.n_pln;
    K.n_tri = sc.n_tri;
    K.n_quad = sc.n_quad;
    K.cull_omax = sc.cull_omax;
    K.bvh_order_stride = sc.bvh_nodes_per_order * 8;
    K.bvh_order_mask = sc.bvh_order_mask;
    int nmax = sc.n_sph;  // Main.cu:217
    if (sc.n_pln > nmax) nmax = sc.n_pln;
    if (sc.n_tri > nmax) nmax = sc.n_tri;
    if (sc.n_quad > nmax) nmax = sc.n_quad;
    K.n_max = nmax;
    const float* base = c->scene_buf.as<const float>();
    K.sph = base;
    K.pln = base + sc.off_pln;
    K.tri = base + sc.off_tri;
    K.quad = base + sc.off_quad;
    K.hit = base + sc.off_hit;
    K.bvh_nodes = sc.off_bvh ? base + sc.off_bvh : nullptr;
    K.bvh_leafrec = sc.off_bvh ? base + sc.off_bvh_prims : nullptr;
    K.bvh_leafvtx = sc.off_bvh ? base + sc.off_bvh_vtx : nullptr;
    K.bvh_nodes16 = sc.off_bvh && sc.off_bvh16 ? reinterpret_cast<const unsigned*>(base + sc.off_bvh16) : nullptr;
    K.bvh_n_nodes = sc.bvh_nodes_per_order;
    K.ovf_sc = sc.ovf_sc;
    K.ovf_nm = sc.ovf_nm;
    K.ovf_im = sc.ovf_im;
    K.cull_dmax = sc.cull_dmax;
    K.spp_inner = c->spp_inner;
}

// Luminance moment tracking (rt_set_moments, rt_moments.h) of the call that
// renders frames first .. first + samples - 1: whether it is tracked (`run`;
// rt_accum.h steps 4 and 5), its buffers and the arguments of its update pass.
static int moments_prepare(rt_context* c, unsigned first, int samples, rt_mom_args& A, bool& run) {
    run = c->st.uniform_track(first);
    if (!run) return RT_OK;
    const size_t npix = (size_t)c->rows * c->width;
    const char* oom = "host moments for %zu pixels";
    int rc = ensure_buf(c, c->mom_prev, npix * 3 * sizeof(float), oom, npix);
    if (!rc) rc = ensure_buf(c, c->mom_m, npix * sizeof(float2), oom, npix);
    if (rc) {
        c->st.end_tracking();
        return rc;
    }
    const HostFpEnv fp;
    A.npix = (long)npix;
    A.first = first == 1u;
    A.kf = (float)samples;
    A.invk = 1.0f / A.kf;
    A.kw = A.kf / (float)(first - 1u + (unsigned)samples);
    A.accum = c->accum.as<float>();
    A.prev = c->mom_prev.as<float>();
    A.mom = c->mom_m.as<float2>();
    return RT_OK;
}

// The CPU backend's render: rt_cpu.cpp over the host state, synchronous
static int cpu_render(rt_context* c, const rt_render_params* p, int threads, uint8_t* rgba_out, float* accum_out) {
    rt_kparams K;
    unsigned first = 0;
    int rc = prepare(c, p, K, first);
    if (rc) return rc;
    const size_t npix = (size_t)c->rows * c->width;
    K.rgba = c->rgba.as<unsigned>();
    rt_mom_args MA;
    bool track = false;
    if ((rc = moments_prepare(c, first, p->samples, MA, track))) return rc;
    (void)c->render.begin(nullptr, true);
    rt_cpu_render(K, c->nee_args(K.max_bounces), threads > 0 ? threads : c->threads);
    if (track) rt_cpu_moments(MA, threads > 0 ? threads : c->threads);
    (void)c->render.end(nullptr);
    c->st.uniform_done(first, p->samples, track);
    if (rgba_out) std::memcpy(rgba_out, c->rgba.p, npix * 4);
    if (accum_out) planes_to_rgb(c->accum.as<float>(), npix, accum_out);
    return RT_OK;
}

static rt_context::SkyKey sky_key_of(const rt_context* c, const rt_kparams& K) {
    rt_context::SkyKey k;
    k.gen = c->sky_gen;
    k.width = K.width;
    k.height = K.height;
    k.rows = K.rows;
    k.row_offset = K.row_offset;
    k.row_stride = K.row_stride;
    k.tile_w = K.tile_w;
    k.tile_sq = K.tile_sq;
    k.spp_inner = K.spp_inner;
    k.jitter = K.jitter;
    return k;
}

void sky_table(rt_context* c, const rt_kparams& K) {
    const rt_context::SkyKey k = sky_key_of(c, K);
    if (k == c->sky_key) return;
    // the last upload read sky_bits (it precedes that launch's kernel on its stream)
    if (c->sky_uploaded && c->sky_ev) (void)hipEventSynchronize(c->sky_ev);
    rt_sky_build(K, c->sky_prims, c->sky_bits);
    c->sky_key = k;
    c->sky_builds++;
    c->sky_uploaded = false;
    c->sky_any = false;
    for (const uint32_t w : c->sky_bits) c->sky_any = c->sky_any || w != 0u;
}

void policy_tiles(const rt_context* c, rt_kparams& K) {
    // wave tiles: 8 x 8 pixels; on small shards (one rank of a multi-GPU
    // frame, below 1024 pixels per CU) 32 x 2 (config 3 at 1/8: 0.249 ->
    // 0.244 ms); BVH scenes 4 x 16 on small shards: squarer tiles keep a
    // wave's rays closer together (config 5: 170.4 -> 167.7 ms; at 1/8 38.5 ->
    // 35.2).  Full brute-force frames took 16 x 4 until late in round 3; with
    // the kernel of then, 8 x 8 is ahead (bench kernel average, config 3,
    // three alternating runs: 0.7495 / 0.7535 / 0.7497 vs 0.7579 / 0.7616 /
    // 0.7559 ms; c2 -3 %, c4 5.51 vs 5.53 ms; 1/2 shard -2 %, 1/4 flat;
    // profiles/r03e/c3_knobs.txt, profiles/r03e/tiles/)
    const bool small = (long)K.rows * K.width <= (long)c->num_cus * 1024;
    K.tile_w = c->tile_w >= 0 ? c->tile_w : K.bvh_nodes ? (small ? 4 : 8) : (small ? 32 : 8);
    K.tile_sq = c->tile_sq;
}

static int launch(rt_context* c, rt_kparams& K, hipStream_t s, unsigned first, int samples) {
    policy_tiles(c, K);
    const bool small = (long)K.rows * K.width <= (long)c->num_cus * 1024;
    // BVH refill kernel: test the parked leaves once this many of a wave's 64
    // lanes are ready; small shards (every wave resident at once, the frame
    // ends with the slowest waves) batch later
    K.leaf_batch = c->leaf_batch > 0 ? c->leaf_batch : small ? RT_LEAF_BATCH_SMALL : RT_LEAF_BATCH;
    K.refill = c->refill > 0 ? c->refill : small ? RT_REFILL_SMALL : RT_REFILL;
    // next-event estimation: its own kernel (rt_kernel_nee.h), which takes no
    // global records, no launch-order feedback and no sky table
    const rt_nee_args N = c->nee_args(K.max_bounces);
    const bool nee = N.n_lights > 0;
    // deep paths: the sorted kernel's record stack in global memory (launch policy)
    K.rec = nullptr;
    // the render units of the precision mode
    const bool fast = c->precision == RT_PRECISION_REFERENCE_FAST;
    const auto wants_global_records = fast ? rt_fast::rt_render_wants_global_records : rt_render_wants_global_records;
    const auto launch_render = fast ? rt_fast::rt_launch_render : rt_launch_render;
    if (!c->simple && !nee && (c->grec == 1 || (c->grec < 0 && wants_global_records(K, c->num_cus)))) {
        const int rc = ensure_buf(c, c->rec, rt_render_rec_floats(K) * sizeof(float));
        if (rc) return rc;
        K.rec = c->rec.as<float>();
    }
    unsigned long long* stamps = nullptr;
    const int NST = 40;  // 8 per-phase wave-cycle sums + utilisation / branch counters
    if (tuning_env("BWRT_STAMPS")) {  // diagnostic builds (-DRT_STAMPS)
        if (hipMalloc(&stamps, NST * sizeof(unsigned long long)) == hipSuccess)
            (void)hipMemsetAsync(stamps, 0, NST * sizeof(unsigned long long), s);
        K.stamps = stamps;
    }
    const char* gtimes = tuning_env("BWRT_GTIMES");  // diagnostic builds (-DRT_GTIMES): group times file
    const size_t NGT = (size_t)RT_GTIMES_WORDS;
    if (gtimes && !stamps) {
        if (hipMalloc(&stamps, NGT * sizeof(unsigned long long)) == hipSuccess)
            (void)hipMemsetAsync(stamps, 0, NGT * sizeof(unsigned long long), s);
        K.stamps = stamps;
    }
    // launch-order feedback: room for a grid of 64-lane groups over the
    // padded wave tiles (any block size needs fewer groups)
    if (c->order_feedback && !c->simple && !nee) {
        const size_t cap = ((size_t)K.width + 128) * ((size_t)K.rows + 128) / 64 + 1;  // tiles padded to 2 x 2
        const void* before = c->gorder.p;
        int rc = ensure_buf(c, c->gcost, cap * sizeof(unsigned));
        if (!rc) rc = ensure_buf(c, c->gorder, cap * sizeof(int));
        if (rc) return rc;
        if (c->gorder.p != before) c->order_n = 0;  // fresh buffer: no order yet
        K.group_cost = c->gcost.as<unsigned>();
        K.group_order = c->gorder.as<int>();
        K.order_n = c->order_n;
        K.order_cap = (long)(c->gorder.bytes / sizeof(int));
        // BVH scenes re-sort every launch: their order keeps improving when
        // sorted from costs measured under the previous order (config 5: 85.8
        // / 86.3 / 86.1 ms every launch vs 86.7 / 87.0 / 87.0 every 16th), and
        // the sort is 6.5 us of an 86 ms frame (profiles/r03g/order_period_configs_ab.txt)
        K.order_sort = K.bvh_nodes || c->order_stale || c->launches % (unsigned long long)c->order_period == 0;
        c->order_stale = false;
    }
    // moment tracking: its buffers before anything is queued
    rt_mom_args MA;
    bool track = false;
    if (const int rc = moments_prepare(c, first, samples, MA, track)) return rc;
    // after the last render, denoise and reprojection pass on another stream
    int orc = order_after_all(c, s);
    if (orc) return orc;
    // sky table (rt_sky.h), for launches of the sorted brute-force kernel: an
    // unchanged view costs the key compare; a view's first launch goes without
    // a table (rt_context.h sky_eager), its second builds and uploads one
    // ahead of the kernel on its stream
    bool sky = !nee && c->sky_on && rt_render_takes_sorted(K, c->num_cus, c->simple, c->block, c->spread);
    if (sky && !c->sky_eager) {
        const rt_context::SkyKey k = sky_key_of(c, K);
        if (!(k == c->sky_key) && !(k == c->sky_seen)) {
            c->sky_seen = k;
            sky = false;
        }
    }
    if (sky) {
        sky_table(c, K);
        if (c->sky_any && !c->sky_uploaded) {
            const size_t bytes = c->sky_bits.size() * sizeof(uint32_t);
            if (const int rc = ensure_buf(c, c->sky_buf, bytes)) return rc;
            if (!c->sky_ev) HIP_TRY(c, hipEventCreateWithFlags(&c->sky_ev, hipEventDisableTiming));
            HIP_TRY(c, hipMemcpyAsync(c->sky_buf.p, c->sky_bits.data(), bytes, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipEventRecord(c->sky_ev, s));
            c->sky_uploaded = true;
        }
        if (c->sky_any) K.sky = c->sky_buf.as<unsigned>();
    }
    rt_order_groups_last = 0;
    rt_launched_kernel[0] = 0;
    // the start marker only with kernel timing on; the one end event serves
    // both the ordering of later calls and the timing (Pass::end)
    HIP_TRY(c, c->render.begin(s, c->ktiming));
    hipError_t e = nee ? rt_launch_render_nee(K, N, nullptr, c->num_cus, c->grid_mult, s)
                       : launch_render(K, c->num_cus, c->grid_mult, c->simple, c->block, s, c->spread);
    if (e == hipSuccess && rt_order_groups_last > 0) c->order_n = rt_order_groups_last;
    c->kernel_name = rt_launched_kernel;
    c->launches++;
    if (gtimes && stamps) {
        std::vector<unsigned long long> h(NGT);
        (void)hipMemcpyAsync(h.data(), stamps, NGT * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        if (FILE* f = std::fopen(gtimes, "wb")) {
            std::fwrite(h.data(), sizeof(unsigned long long), NGT, f);
            std::fclose(f);
        }
        (void)hipFree(stamps);
        stamps = nullptr;
    }
    if (stamps) {
        unsigned long long h[NST] = {0};
        (void)hipMemcpyAsync(h, stamps, sizeof h, hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        std::fprintf(stderr, "stamps");
        for (int k = 0; k < NST; k++) std::fprintf(stderr, " %llu", h[k]);
        std::fprintf(stderr, "\n");
        (void)hipFree(stamps);
    }
    if (e != hipSuccess) {
        c->st.end_tracking();
        return hip_fail(c, e, "rt_render_kernel launch");
    }
    // the moment update of this call's batch: behind the render kernel on the
    // same stream and inside the render pass, so the pass's one end event (or
    // none, between back-to-back renders on the context's stream) orders every
    // later call after it and no packet of its own goes on the stream
    if (track) {
        e = rt_launch_moments(MA, s);
        if (e != hipSuccess) {
            c->st.end_tracking();
            return hip_fail(c, e, "rt_moments_kernel launch");
        }
    }
    if ((e = c->render.end(s)) != hipSuccess) {  // both kernels are queued: frameSum moved on
        c->st.end_tracking();
        return hip_fail(c, e, "c->render.end(s)");
    }
    c->st.uniform_done(first, samples, track);
    return RT_OK;
}

// The context's next `samples` frames of a shard, at its own bounce limit
static rt_render_params next_frames(const rt_context* c, int width, int height, int samples, int row_offset,
                                    int row_stride) {
    rt_render_params p;
    p.width = width;
    p.height = height;
    p.samples = samples;
    p.max_bounces = c->max_bounces;
    p.first_frame = 0;
    p.row_offset = row_offset;
    p.row_stride = row_stride;
    return p;
}

extern "C" {

int rt_render_ex(rt_context* c, const rt_render_params* p, uint8_t* rgba_out, float* accum_out) {
    if (c && c->cpu) return cpu_render(c, p, 0, rgba_out, accum_out);
    rt_kparams K;
    unsigned first = 0;
    int rc = prepare(c, p, K, first);
    if (rc) return rc;
    const size_t npix = (size_t)c->rows * c->width;
    rc = ensure_buf(c, c->rgba, npix * 4);
    if (rc) return rc;
    K.rgba = c->rgba.as<unsigned>();
    rc = launch(c, K, c->stream, first, p->samples);
    if (rc) return rc;
    if (rgba_out) HIP_TRY(c, hipMemcpyAsync(rgba_out, c->rgba.p, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (accum_out) {
        std::vector<float> planes(npix * 3);
        HIP_TRY(c, hipMemcpyAsync(planes.data(), c->accum.p, npix * 3 * sizeof(float), hipMemcpyDeviceToHost,
                                  c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        planes_to_rgb(planes.data(), npix, accum_out);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

int rt_render(rt_context* c, int width, int height, int samples, uint8_t* rgba_out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const rt_render_params p = next_frames(c, width, height, samples, 0, 1);
    return rt_render_ex(c, &p, rgba_out, nullptr);
}

// Single-process multi-GPU (the C++ host's counterpart of bench.py's one
// process per GPU): context i renders rows y = i (mod n) on its own stream,
// all launches in flight at once; the shards come back through pinned host
// buffers and are interleaved on the host.
int rt_render_multi(rt_context* const* ctxs, int n, int width, int height, int samples, uint8_t* rgba_out) {
    if (!ctxs || n <= 0 || width <= 0 || height <= 0 || samples <= 0) return RT_ERR_INVALID_ARGUMENT;
    // (every entry reports on itself, a null one with the bare code)
    if (const int rc = group_scan(ctxs, n, nullptr, "rt_render_multi", true)) return rc;
    const int active = group_active(n, height);
    // a failure at context i leaves contexts 0..i-1 with renders and copies
    // into their pinned buffers in flight: drain them before returning, so a
    // later call cannot reuse host_rgba under a running copy
    for (int i = 0; i < active; i++) {
        rt_context* c = ctxs[i];
        const rt_render_params p = next_frames(c, width, height, samples, i, n);
        rt_kparams K;
        unsigned first = 0;
        int rc = prepare(c, &p, K, first);
        if (rc) return group_drain(ctxs, i, rc);
        const size_t bytes = (size_t)c->rows * width * 4;
        rc = ensure_buf(c, c->rgba, bytes);
        if (rc) return group_drain(ctxs, i, rc);
        if (c->host_rgba_bytes < bytes) {
            rc = quiesce(c);
            if (rc) return group_drain(ctxs, i, rc);
            if (hipStreamSynchronize(c->stream) != hipSuccess) return group_drain(ctxs, i, fail(c, RT_ERR_HIP, "stream sync"));
            if (c->host_rgba) (void)hipHostFree(c->host_rgba);
            c->host_rgba = nullptr;
            c->host_rgba_bytes = 0;
            const hipError_t e = hipHostMalloc(&c->host_rgba, bytes, hipHostMallocDefault);
            if (e != hipSuccess) return group_drain(ctxs, i, hip_fail(c, e, "hipHostMalloc"));
            c->host_rgba_bytes = bytes;
        }
        K.rgba = c->rgba.as<unsigned>();
        rc = launch(c, K, c->stream, first, samples);
        if (rc) return group_drain(ctxs, i + 1, rc);
        const hipError_t e = hipMemcpyAsync(c->host_rgba, c->rgba.p, bytes, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) return group_drain(ctxs, i + 1, hip_fail(c, e, "hipMemcpyAsync"));
    }
    if (const int rc = group_sync(ctxs, active)) return rc;
    for (int i = 0; i < active && rgba_out; i++) {
        const rt_context* c = ctxs[i];
        const uint8_t* src = (const uint8_t*)c->host_rgba;
        for (int j = 0; j < c->rows; j++)
            std::memcpy(rgba_out + ((size_t)(i + j * n) * width) * 4, src + (size_t)j * width * 4, (size_t)width * 4);
    }
    return RT_OK;
}

int rt_render_device(rt_context* c, const rt_render_params* p, void* rgba_device, void* stream) {
    int rc = device_ctx(c, "rt_render_device");
    if (rc) return rc;
    rt_kparams K;
    unsigned first = 0;
    if ((rc = prepare(c, p, K, first))) return rc;
    if ((rc = device_aligned(c, {{rgba_device, "rgba_device", false}}))) return rc;
    K.rgba = (unsigned*)rgba_device;
    return launch(c, K, device_stream(c, stream), first, p->samples);
}

int rt_deinterleave_rows_device(rt_context* c, const void* gathered, void* image, int width, int height,
                                int shards, int rows_per_shard, void* stream) {
    if (!c || !gathered || !image) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (width <= 0 || height <= 0 || shards <= 0 || rows_per_shard * shards < height)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "bad deinterleave geometry");
    if (c->cpu) return fail(c, RT_ERR_UNSUPPORTED, "rt_deinterleave_rows_device: CPU context");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    HIP_TRY(c, rt_launch_deinterleave((const unsigned*)gathered, (unsigned*)image, width, height, shards,
                                      rows_per_shard, c->deint_blocks, s));
    HIP_TRY(c, c->aux.end(s));
    return RT_OK;
}

int rt_sky_table(rt_context* c, const rt_render_params* p, int tile_w, int tile_sq, uint32_t* bits, size_t words,
                 long long* tiles_out, unsigned long long* builds_out) {
    const HostFpEnv fp;
    if (!c || !p) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!c->has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    const int stride = p->row_stride == 0 ? 1 : p->row_stride;
    if (const int rc = shard_check(c, p->width, p->height, p->row_offset, stride)) return rc;
    if (tile_w > 64 || (tile_w > 0 && (tile_w & (tile_w - 1))))
        return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_sky_table: tile_w %d is not a power of two up to 64", tile_w);
    if (words && !bits) return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_sky_table: null bits");
    rt_kparams K;
    fill_view(c, p->width, p->height, p->row_offset, stride, shard_rows(p->height, p->row_offset, stride), K);
    if (tile_w < 0) {
        policy_tiles(c, K);
    } else {
        K.tile_w = tile_w;
        K.tile_sq = tile_sq != 0;
    }
    sky_table(c, K);
    for (size_t i = 0; i < words; i++) bits[i] = i < c->sky_bits.size() ? c->sky_bits[i] : 0u;
    if (tiles_out) *tiles_out = rt_sky_tiles(K);
    if (builds_out) *builds_out = c->sky_builds;
    return RT_OK;
}

int rt_render_cpu(rt_context* c, const rt_render_params* p, int threads, uint8_t* rgba_out, float* accum_out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (!c->cpu) return fail(c, RT_ERR_INVALID_ARGUMENT, "rt_render_cpu: not a CPU context (rt_create_cpu)");
    if (threads < 0) return fail(c, RT_ERR_INVALID_ARGUMENT, "threads < 0");
    return cpu_render(c, p, threads, rgba_out, accum_out);
}

}  // extern "C"
