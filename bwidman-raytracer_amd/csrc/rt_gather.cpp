// rt_gather.cpp — row shards into one frame (include/rt_abi.h, DESIGN.md
// sections 17 and 19): rt_export_shard writes a context's block, rt_assemble
// de-interleaves the ranks' gathered blocks into the context's assembled frame,
// rt_assemble_multi does both for the contexts of one process.  The _adaptive
// forms do the same with COUNTED blocks, which carry every pixel's {n_p, J_p},
// so that a frame sampled adaptively on row shards reaches the count-aware
// passes.  rt_layout.h (rt_asm_args) has the one block layout of the four plane
// counts, rt_assemble.h the indexing; the full-frame passes pick the assembled
// frame up in rt_post.cpp (frame_src, frame_counts).  Both forms run the same
// passes: `counted` decides only which plane counts an entry point accepts and
// whether it takes a non-uniform accumulation.
//
// No call reads or writes the RNG state or the frame counter or writes
// frameSum, the moments or the counts; all are copies, so there is no
// arithmetic to keep exact.
#include "rt_group.h"

namespace {

// The plain and the full plane count of the uncounted (3, 5) and of the counted
// (4, 7) entry points
int plain_planes(bool counted) { return counted ? 4 : 3; }
int full_planes(bool counted) { return counted ? 7 : 5; }
int planes_check(rt_context* c, int planes, bool counted) {
    if (planes == plain_planes(counted) || planes == full_planes(counted)) return RT_OK;
    return fail(c, RT_ERR_INVALID_ARGUMENT, "planes %d is neither %d nor %d", planes, plain_planes(counted),
                full_planes(counted));
}

size_t block_floats(const rt_context* c, int rows_per_shard, int planes) {
    return (size_t)planes * (size_t)rows_per_shard * (size_t)c->width;
}

// What an export needs besides its destination.  Only a counted block can
// stand for a non-uniform accumulation.
int export_check(rt_context* c, int rows_per_shard, int planes, bool counted) {
    if (const int rc = planes_check(c, planes, counted)) return rc;
    if (!counted && c->st.nonuniform())
        return fail(c, RT_ERR_UNSUPPORTED,
                    "the accumulation is non-uniform (rt_render_adaptive): a block carries one frame count");
    if (c->st.frame() < 2u || !c->accum.p || c->rows <= 0)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "no frame accumulated yet (render first)");
    if (const int rc = block_rows_check(c, rows_per_shard)) return rc;
    if (const int rc = block_plane_check(c, rows_per_shard)) return rc;
    if (rt_block_shape_of(planes).moments && !c->st.current())
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "%d planes need current moments (rt_set_moments before the accumulation's first render)", planes);
    return RT_OK;
}

// The export pass of a checked call into `block` (device memory on a GPU
// context, on stream s: after the last render or adaptive call and its update
// and resolve, and the next render after it; host memory on a CPU context).  A
// counted block of a uniform accumulation gets the context's {n, J} for every
// pixel: nothing of the context is written.
int export_pass(rt_context* c, int rows_per_shard, int planes, float* block, hipStream_t s) {
    const rt_block_shape B = rt_block_shape_of(planes);
    rt_asm_args A;
    std::memset(&A, 0, sizeof A);
    A.width = c->width;
    A.rows = c->rows;
    A.shards = 1;
    A.rows_per_shard = rows_per_shard;
    A.planes = planes;
    A.sum = c->accum.as<float>();
    A.mom = B.moments ? c->mom_m.as<float2>() : nullptr;
    A.block = block;
    if (B.counted) {
        A.cnt = c->st.nonuniform() ? c->ad_cnt.as<uint2>() : nullptr;
        A.n = c->st.frames();
        A.j = c->st.batches();
    }
    if (c->cpu) {
        (void)c->xport.begin(nullptr, false);
        rt_cpu_export_shard(A, c->threads);
        (void)c->xport.end(nullptr);
        return RT_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->xport.create(false));
    if (const int rc = order_after_all(c, s)) return rc;
    HIP_TRY(c, rt_launch_export_shard(A, c->deint_blocks, s));
    HIP_TRY(c, c->xport.end(s));
    return RT_OK;
}

void report(const rt_context* c, unsigned* frames_out, unsigned* batches_out) {
    if (frames_out) *frames_out = c->st.frames();
    if (batches_out) *batches_out = c->st.batches();
}

// The host form of an export (`counted`: rt_export_shard_adaptive)
int export_host(rt_context* c, int rows_per_shard, int planes, float* block, unsigned* frames_out,
                unsigned* batches_out, bool counted) {
    if (!c || !block) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    int rc = export_check(c, rows_per_shard, planes, counted);
    if (rc) return rc;
    if (c->cpu) {
        if ((rc = export_pass(c, rows_per_shard, planes, block, nullptr))) return rc;
    } else {
        const size_t bytes = block_floats(c, rows_per_shard, planes) * sizeof(float);
        HIP_TRY(c, hipSetDevice(c->device));
        if ((rc = ensure_buf(c, c->as_block, bytes))) return rc;
        if ((rc = export_pass(c, rows_per_shard, planes, c->as_block.as<float>(), c->stream))) return rc;
        HIP_TRY(c, hipMemcpyAsync(block, c->as_block.p, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    report(c, frames_out, batches_out);
    return RT_OK;
}

// The device form (`name`: the entry point)
int export_device(rt_context* c, const char* name, int rows_per_shard, int planes, void* block_device, void* stream,
                  unsigned* frames_out, unsigned* batches_out, bool counted) {
    hipStream_t s;
    int rc = device_call(c, name, {{block_device, "block_device", true}}, stream, &s);
    if (rc) return rc;
    if ((rc = export_check(c, rows_per_shard, planes, counted))) return rc;
    if ((rc = export_pass(c, rows_per_shard, planes, (float*)block_device, s))) return rc;
    report(c, frames_out, batches_out);
    return RT_OK;
}

// What an assembly needs besides its source
int assemble_check(rt_context* c, int shards, int rows_per_shard, int planes, unsigned frames, bool counted) {
    if (!c->has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    if (c->width <= 0 || c->height <= 0)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "no frame shape yet (render or rt_init_rand first)");
    if (const int rc = planes_check(c, planes, counted)) return rc;
    if (const int rc = block_cover_check(c, "assembly", shards, rows_per_shard)) return rc;
    if (frames < 1u) return fail(c, RT_ERR_INVALID_ARGUMENT, "frames must be >= 1");
    return block_plane_check(c, rows_per_shard);
}

// The assembly pass of a checked call from `gathered` (device memory on a GPU
// context, on stream s: after every earlier pass that reads the assembled
// frame, and they after it), then the snapshot's record.  The context has one
// assembled frame: a counted and an uncounted assembly replace each other's.
int assemble_pass(rt_context* c, const float* gathered, int shards, int rows_per_shard, int planes, unsigned frames,
                  unsigned batches, hipStream_t s) {
    const size_t npix = (size_t)c->height * c->width;
    const char* oom = "host assembled frame for %zu pixels";
    const bool counted = rt_block_shape_of(planes).counted, moments = rt_block_shape_of(planes).moments;
    if (!c->cpu) HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_buf(c, c->as.sum, npix * 3 * sizeof(float), oom, npix);
    if (!rc && moments) rc = ensure_buf(c, c->as.mom, npix * sizeof(float2), oom, npix);
    if (!rc && counted) rc = ensure_buf(c, c->as.cnt, npix * sizeof(uint2), oom, npix);
    if (rc) {
        // a buffer of the earlier frame went in the attempt to grow
        const rt_block_shape B = c->assembled_shape();
        if (!c->as.sum.p || (B.moments && !c->as.mom.p) || (B.counted && !c->as.cnt.p)) c->vs.assembled_drop();
        return rc;
    }
    rt_asm_args A;
    std::memset(&A, 0, sizeof A);
    A.width = c->width;
    A.rows = c->height;
    A.shards = shards;
    A.rows_per_shard = rows_per_shard;
    A.planes = planes;
    A.sum = c->as.sum.as<float>();
    A.mom = moments ? c->as.mom.as<float2>() : nullptr;
    A.block = const_cast<float*>(gathered);
    A.cnt = counted ? c->as.cnt.as<uint2>() : nullptr;
    c->vs.assembled_drop();  // until the pass is queued: a failure leaves no half-written snapshot behind
    if (c->cpu) {
        (void)c->assemble.begin(nullptr, true);
        rt_cpu_assemble(A, c->threads);
        (void)c->assemble.end(nullptr);
    } else {
        HIP_TRY(c, c->assemble.create(true));
        if ((rc = order_after_all(c, s))) return rc;
        HIP_TRY(c, c->assemble.begin(s, true));
        HIP_TRY(c, rt_launch_assemble(A, c->deint_blocks, s));
        HIP_TRY(c, c->assemble.end(s));
    }
    c->vs.assembled_done(c->width, c->height, planes, frames, moments ? batches : 0u);
    return RT_OK;
}

int assemble_host(rt_context* c, const float* gathered, int shards, int rows_per_shard, int planes, unsigned frames,
                  unsigned batches, bool counted) {
    if (!c || !gathered) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    int rc = assemble_check(c, shards, rows_per_shard, planes, frames, counted);
    if (rc) return rc;
    if (c->cpu) return assemble_pass(c, gathered, shards, rows_per_shard, planes, frames, batches, nullptr);
    const size_t bytes = (size_t)shards * block_floats(c, rows_per_shard, planes) * sizeof(float);
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_buf(c, c->as_gather, bytes))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->as_gather.p, gathered, bytes, hipMemcpyHostToDevice, c->stream));
    rc = assemble_pass(c, c->as_gather.as<float>(), shards, rows_per_shard, planes, frames, batches, c->stream);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return rc;
}

int assemble_device(rt_context* c, const char* name, const void* gathered_device, int shards, int rows_per_shard,
                    int planes, unsigned frames, unsigned batches, void* stream, bool counted) {
    hipStream_t s;
    int rc = device_call(c, name, {{gathered_device, "gathered_device", true}}, stream, &s);
    if (rc) return rc;
    if ((rc = assemble_check(c, shards, rows_per_shard, planes, frames, counted))) return rc;
    return assemble_pass(c, (const float*)gathered_device, shards, rows_per_shard, planes, frames, batches, s);
}

// rt_assemble_multi and, `counted`, rt_assemble_adaptive_multi (`name`): 3 and
// 5 planes against 4 and 7, and only the counted form takes contexts in the
// non-uniform state
int assemble_multi(rt_context* const* ctxs, int n, int planes, int dst, bool counted, const char* name) {
    if (!ctxs || n <= 0 || dst < 0 || dst >= n || !ctxs[dst]) return RT_ERR_INVALID_ARGUMENT;
    rt_context* d = ctxs[dst];
    const int plain = plain_planes(counted), full = full_planes(counted);
    if (planes != 0 && planes != plain && planes != full)
        return fail(d, RT_ERR_INVALID_ARGUMENT, "planes %d is neither 0, %d nor %d", planes, plain, full);
    // every condition first: a refusal touches nothing
    if (const int rc = group_scan(ctxs, n, d, name)) return rc;
    const int width = d->width, height = d->height;
    if (!d->has_scene) return fail(d, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    if (width <= 0 || height <= 0)
        return fail(d, RT_ERR_INVALID_ARGUMENT, "no frame shape yet (render or rt_init_rand first)");
    const int active = group_active(n, height);
    bool current = true;
    for (int i = 0; i < active; i++) {
        const rt_context* c = ctxs[i];
        if (const int rc = group_shard_check(d, c, i, n, c->row_stride, width, height)) return rc;
        if (!counted && c->st.nonuniform())
            return fail(d, RT_ERR_UNSUPPORTED,
                        "the accumulation is non-uniform (rt_render_adaptive): a block carries one frame count");
        if (c->st.frame() < 2u) return fail(d, RT_ERR_INVALID_ARGUMENT, "no frame accumulated yet (render first)");
        if (const int rc = group_counters_check(d, c, i, ctxs[0], false)) return rc;
        current = current && c->st.current() && c->st.batches() == ctxs[0]->st.batches();
    }
    if (planes == 0) planes = current ? full : plain;
    if (planes == full && !current)
        return fail(d, RT_ERR_INVALID_ARGUMENT,
                    "%d planes need current moments of equal batches on every context (rt_set_moments)", full);
    const int rps = group_rows_per_shard(n, height);
    const unsigned frames = ctxs[0]->st.frames(), batches = ctxs[0]->st.batches();
    const size_t blk = block_floats(d, rps, planes);
    if (!d->cpu) HIP_TRY(d, hipSetDevice(d->device));
    int rc = ensure_buf(d, d->as_gather, (size_t)n * blk * sizeof(float), "host gathered blocks (%zu floats)",
                        (size_t)n * blk);
    if (rc) return rc;
    float* gathered = d->as_gather.as<float>();
    // (as_gather is read only by assemblies of host forms, which synchronise before they return)
    // a failure at context i leaves exports and copies of contexts 0..i-1 in flight: drain them
    for (int i = 0; i < active; i++) {
        rt_context* c = ctxs[i];
        if (c->cpu) {
            if ((rc = export_pass(c, rps, planes, gathered + (size_t)i * blk, nullptr))) return rc;
            continue;
        }
        if (hipSetDevice(c->device) != hipSuccess) return group_drain(ctxs, i, fail(c, RT_ERR_HIP, "hipSetDevice"));
        if ((rc = ensure_buf(c, c->as_block, blk * sizeof(float)))) return group_drain(ctxs, i, rc);
        if ((rc = export_pass(c, rps, planes, c->as_block.as<float>(), c->stream))) return group_drain(ctxs, i + 1, rc);
        const hipError_t e = group_copy(gathered + (size_t)i * blk, d, c->as_block.p, c, blk * sizeof(float));
        if (e != hipSuccess) return group_drain(ctxs, i + 1, hip_fail(c, e, "block copy"));
    }
    // the blocks are in place before the assembly is queued (the call synchronises anyway)
    if ((rc = group_sync(ctxs, active))) return rc;
    rc = assemble_pass(d, gathered, n, rps, planes, frames, batches, d->stream);
    if (!d->cpu) HIP_TRY(d, hipStreamSynchronize(d->stream));
    return rc;
}

}  // namespace

extern "C" {

int rt_export_shard(rt_context* c, int rows_per_shard, int planes, float* block, unsigned* frames_out,
                    unsigned* batches_out) {
    return export_host(c, rows_per_shard, planes, block, frames_out, batches_out, false);
}

int rt_export_shard_device(rt_context* c, int rows_per_shard, int planes, void* block_device, void* stream,
                           unsigned* frames_out, unsigned* batches_out) {
    return export_device(c, "rt_export_shard_device", rows_per_shard, planes, block_device, stream, frames_out,
                         batches_out, false);
}

int rt_export_shard_adaptive(rt_context* c, int rows_per_shard, int planes, float* block, unsigned* frames_out,
                             unsigned* batches_out) {
    return export_host(c, rows_per_shard, planes, block, frames_out, batches_out, true);
}

int rt_export_shard_adaptive_device(rt_context* c, int rows_per_shard, int planes, void* block_device, void* stream,
                                    unsigned* frames_out, unsigned* batches_out) {
    return export_device(c, "rt_export_shard_adaptive_device", rows_per_shard, planes, block_device, stream,
                         frames_out, batches_out, true);
}

int rt_assemble(rt_context* c, const float* gathered, int shards, int rows_per_shard, int planes, unsigned frames,
                unsigned batches) {
    return assemble_host(c, gathered, shards, rows_per_shard, planes, frames, batches, false);
}

int rt_assemble_device(rt_context* c, const void* gathered_device, int shards, int rows_per_shard, int planes,
                       unsigned frames, unsigned batches, void* stream) {
    return assemble_device(c, "rt_assemble_device", gathered_device, shards, rows_per_shard, planes, frames, batches,
                           stream, false);
}

int rt_assemble_adaptive(rt_context* c, const float* gathered, int shards, int rows_per_shard, int planes,
                         unsigned frames, unsigned batches) {
    return assemble_host(c, gathered, shards, rows_per_shard, planes, frames, batches, true);
}

int rt_assemble_adaptive_device(rt_context* c, const void* gathered_device, int shards, int rows_per_shard, int planes,
                                unsigned frames, unsigned batches, void* stream) {
    return assemble_device(c, "rt_assemble_adaptive_device", gathered_device, shards, rows_per_shard, planes, frames,
                           batches, stream, true);
}

int rt_assemble_multi(rt_context* const* ctxs, int n, int planes, int dst) {
    return assemble_multi(ctxs, n, planes, dst, false, "rt_assemble_multi");
}

int rt_assemble_adaptive_multi(rt_context* const* ctxs, int n, int planes, int dst) {
    return assemble_multi(ctxs, n, planes, dst, true, "rt_assemble_adaptive_multi");
}

int rt_assembled(const rt_context* c, unsigned* frames_out, unsigned* batches_out) {
    if (!c || !c->assembled_current()) return 0;
    if (frames_out) *frames_out = c->vs.assembled().frames;
    if (batches_out) *batches_out = c->vs.assembled().batches;
    return 1;
}

int rt_get_assembled(rt_context* c, float* accum_rgb, float* moments) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const rt_view_state::Assembled& a = c->vs.assembled();
    if (!a.made) return fail(c, RT_ERR_INVALID_ARGUMENT, "no assembled frame (rt_assemble first)");
    if (moments && !c->assembled_shape().moments)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "the assembled frame has %d planes: no moments", a.planes);
    const size_t npix = (size_t)a.height * a.width;
    if (c->cpu) {
        if (accum_rgb) planes_to_rgb(c->as.sum.as<float>(), npix, accum_rgb);
        if (moments) std::memcpy(moments, c->as.mom.p, npix * sizeof(float2));
        return RT_OK;
    }
    std::vector<float> planes;
    if (accum_rgb && !try_resize(planes, npix * 3))
        return fail(c, RT_ERR_OUT_OF_MEMORY, "host assembled frame for %zu pixels", npix);
    const int rc = read_settled(c, {{accum_rgb ? planes.data() : nullptr, c->as.sum.p, npix * 3 * sizeof(float)},
                                    {moments, c->as.mom.p, npix * sizeof(float2)}});
    if (rc) return rc;
    if (accum_rgb) planes_to_rgb(planes.data(), npix, accum_rgb);
    return RT_OK;
}

int rt_get_assembled_counts(rt_context* c, uint32_t* frames_out, uint32_t* batches_out) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    const rt_view_state::Assembled& a = c->vs.assembled();
    if (!a.made) return fail(c, RT_ERR_INVALID_ARGUMENT, "no assembled frame (rt_assemble_adaptive first)");
    if (!c->assembled_shape().counted)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "the assembled frame has %d planes: no counts", a.planes);
    const size_t npix = (size_t)a.height * a.width;
    const uint2* cn = c->as.cnt.as<uint2>();
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

int rt_assemble_drop(rt_context* c) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    // the record only: passes still queued on the buffers are ordered by the next assembly's stream waits
    c->vs.assembled_drop();
    return RT_OK;
}

float rt_last_assemble_ms(rt_context* c) { return c ? c->assemble.elapsed_ms() : -1.0f; }

}  // extern "C"
