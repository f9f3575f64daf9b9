// rt_gather.cpp — row shards into one frame (include/rt_abi.h, DESIGN.md
// section 17): rt_export_shard writes a context's block, rt_assemble
// de-interleaves the ranks' gathered blocks into the context's assembled frame,
// rt_assemble_multi does both for the contexts of one process.  rt_layout.h
// (rt_asm_args) has the block layout, rt_assemble.h the indexing; the full-frame
// passes pick the assembled frame up in rt_post.cpp (frame_src).
//
// Neither call reads or writes the RNG state or the frame counter or writes
// frameSum or the moments; both are copies, so there is no arithmetic to keep
// exact.
#include "rt_context.h"

namespace {

size_t block_floats(const rt_context* c, int rows_per_shard, int planes) {
    return (size_t)planes * (size_t)rows_per_shard * (size_t)c->width;
}

// What an export needs besides its destination
int export_check(rt_context* c, int rows_per_shard, int planes) {
    if (planes != 3 && planes != 5) return fail(c, RT_ERR_INVALID_ARGUMENT, "planes %d is neither 3 nor 5", planes);
    if (c->st.nonuniform())
        return fail(c, RT_ERR_UNSUPPORTED,
                    "the accumulation is non-uniform (rt_render_adaptive): a block carries one frame count");
    if (c->st.frame() < 2u || !c->accum.p || c->rows <= 0)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "no frame accumulated yet (render first)");
    if (rows_per_shard < c->rows)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "rows_per_shard %d below the shard's %d rows", rows_per_shard, c->rows);
    if ((long long)rows_per_shard * c->width > (1ll << 31))
        return fail(c, RT_ERR_UNSUPPORTED, "block plane larger than 2^31 floats");
    if (planes == 5 && !c->st.current())
        return fail(c, RT_ERR_INVALID_ARGUMENT,
                    "5 planes need current moments (rt_set_moments before the accumulation's first render)");
    return RT_OK;
}

// The export pass of a checked call into `block` (device memory on a GPU
// context, on stream s: after the last render and its moment update, and the
// next render after it; host memory on a CPU context)
int export_pass(rt_context* c, int rows_per_shard, int planes, float* block, hipStream_t s) {
    rt_asm_args A;
    std::memset(&A, 0, sizeof A);
    A.width = c->width;
    A.rows = c->rows;
    A.shards = 1;
    A.rows_per_shard = rows_per_shard;
    A.planes = planes;
    A.sum = c->accum.as<float>();
    A.mom = planes == 5 ? c->mom_m.as<float2>() : nullptr;
    A.block = block;
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

// What an assembly needs besides its source
int assemble_check(rt_context* c, int shards, int rows_per_shard, int planes, unsigned frames) {
    if (!c->has_scene) return fail(c, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    if (c->width <= 0 || c->height <= 0)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "no frame shape yet (render or rt_init_rand first)");
    if (planes != 3 && planes != 5) return fail(c, RT_ERR_INVALID_ARGUMENT, "planes %d is neither 3 nor 5", planes);
    if (shards < 1 || rows_per_shard < 1 || (long long)rows_per_shard * shards < c->height)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "bad assembly geometry: %d shards of %d rows for height %d", shards,
                    rows_per_shard, c->height);
    if (frames < 1u) return fail(c, RT_ERR_INVALID_ARGUMENT, "frames must be >= 1");
    if ((long long)rows_per_shard * c->width > (1ll << 31))
        return fail(c, RT_ERR_UNSUPPORTED, "block plane larger than 2^31 floats");
    return RT_OK;
}

// The assembly pass of a checked call from `gathered` (device memory on a GPU
// context, on stream s: after every earlier pass that reads the assembled
// frame, and they after it), then the snapshot's record
int assemble_pass(rt_context* c, const float* gathered, int shards, int rows_per_shard, int planes, unsigned frames,
                  unsigned batches, hipStream_t s) {
    const size_t npix = (size_t)c->height * c->width;
    const char* oom = "host assembled frame for %zu pixels";
    if (!c->cpu) HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_buf(c, c->as.sum, npix * 3 * sizeof(float), oom, npix);
    if (!rc && planes == 5) rc = ensure_buf(c, c->as.mom, npix * sizeof(float2), oom, npix);
    if (rc) {
        if (!c->as.sum.p || (c->as.planes == 5 && !c->as.mom.p)) c->as.made = false;  // it went in the attempt to grow
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
    A.mom = planes == 5 ? c->as.mom.as<float2>() : nullptr;
    A.block = const_cast<float*>(gathered);
    c->as.made = false;  // until the pass is queued: a failure leaves no half-written snapshot behind
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
    c->as.made = true;
    c->as.planes = planes;
    c->as.width = c->width;
    c->as.height = c->height;
    c->as.frames = frames;
    c->as.batches = planes == 5 ? batches : 0u;
    c->as.view = c->view;
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_export_shard(rt_context* c, int rows_per_shard, int planes, float* block, unsigned* frames_out,
                    unsigned* batches_out) {
    if (!c || !block) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    int rc = export_check(c, rows_per_shard, planes);
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

int rt_export_shard_device(rt_context* c, int rows_per_shard, int planes, void* block_device, void* stream,
                           unsigned* frames_out, unsigned* batches_out) {
    if (!c || !block_device) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (c->cpu) return fail(c, RT_ERR_UNSUPPORTED, "rt_export_shard_device: CPU context");
    if ((uintptr_t)block_device & 3u) return fail(c, RT_ERR_INVALID_ARGUMENT, "block_device not 4-byte aligned");
    int rc = export_check(c, rows_per_shard, planes);
    if (rc) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = export_pass(c, rows_per_shard, planes, (float*)block_device, s))) return rc;
    report(c, frames_out, batches_out);
    return RT_OK;
}

int rt_assemble(rt_context* c, const float* gathered, int shards, int rows_per_shard, int planes, unsigned frames,
                unsigned batches) {
    if (!c || !gathered) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    int rc = assemble_check(c, shards, rows_per_shard, planes, frames);
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

int rt_assemble_device(rt_context* c, const void* gathered_device, int shards, int rows_per_shard, int planes,
                       unsigned frames, unsigned batches, void* stream) {
    if (!c || !gathered_device) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (c->cpu) return fail(c, RT_ERR_UNSUPPORTED, "rt_assemble_device: CPU context");
    if ((uintptr_t)gathered_device & 3u) return fail(c, RT_ERR_INVALID_ARGUMENT, "gathered_device not 4-byte aligned");
    const int rc = assemble_check(c, shards, rows_per_shard, planes, frames);
    if (rc) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return assemble_pass(c, (const float*)gathered_device, shards, rows_per_shard, planes, frames, batches, s);
}

int rt_assemble_multi(rt_context* const* ctxs, int n, int planes, int dst) {
    if (!ctxs || n <= 0 || dst < 0 || dst >= n || !ctxs[dst]) return RT_ERR_INVALID_ARGUMENT;
    rt_context* d = ctxs[dst];
    if (planes != 0 && planes != 3 && planes != 5)
        return fail(d, RT_ERR_INVALID_ARGUMENT, "planes %d is neither 0, 3 nor 5", planes);
    // every condition first: a refusal touches nothing
    for (int i = 0; i < n; i++) {
        if (!ctxs[i]) return fail(d, RT_ERR_INVALID_ARGUMENT, "null context %d", i);
        if (ctxs[i]->cpu != d->cpu)
            return fail(d, RT_ERR_INVALID_ARGUMENT, "rt_assemble_multi: GPU and CPU contexts mixed");
        for (int j = 0; j < i; j++)
            if (ctxs[j] == ctxs[i]) return fail(d, RT_ERR_INVALID_ARGUMENT, "context listed twice");
    }
    const int width = d->width, height = d->height;
    if (!d->has_scene) return fail(d, RT_ERR_NO_SCENE, "rt_set_scene() not called");
    if (width <= 0 || height <= 0)
        return fail(d, RT_ERR_INVALID_ARGUMENT, "no frame shape yet (render or rt_init_rand first)");
    const int active = n < height ? n : height;  // contexts beyond the image height hold no rows
    bool current = true;
    for (int i = 0; i < active; i++) {
        const rt_context* c = ctxs[i];
        if (c->width != width || c->height != height || c->row_offset != i || c->row_stride != n || !c->accum.p)
            return fail(d, RT_ERR_INVALID_ARGUMENT,
                        "context %d holds %dx%d offset %d stride %d, not shard %d of %d of %dx%d", i, c->width,
                        c->height, c->row_offset, c->row_stride, i, n, width, height);
        if (c->st.nonuniform())
            return fail(d, RT_ERR_UNSUPPORTED,
                        "the accumulation is non-uniform (rt_render_adaptive): a block carries one frame count");
        if (c->st.frame() < 2u) return fail(d, RT_ERR_INVALID_ARGUMENT, "no frame accumulated yet (render first)");
        if (c->st.frame() != ctxs[0]->st.frame())
            return fail(d, RT_ERR_INVALID_ARGUMENT, "frame counters differ (context %d: %u, context 0: %u)", i,
                        c->st.frame(), ctxs[0]->st.frame());
        current = current && c->st.current() && c->st.batches() == ctxs[0]->st.batches();
    }
    if (planes == 0) planes = current ? 5 : 3;
    if (planes == 5 && !current)
        return fail(d, RT_ERR_INVALID_ARGUMENT,
                    "5 planes need current moments of equal batches on every context (rt_set_moments)");
    const int rps = (height + n - 1) / n;
    const unsigned frames = ctxs[0]->st.frames(), batches = ctxs[0]->st.batches();
    const size_t blk = block_floats(d, rps, planes);
    if (!d->cpu) HIP_TRY(d, hipSetDevice(d->device));
    int rc = ensure_buf(d, d->as_gather, (size_t)n * blk * sizeof(float), "host gathered blocks (%zu floats)",
                        (size_t)n * blk);
    if (rc) return rc;
    float* gathered = d->as_gather.as<float>();
    // (as_gather is read only by assemblies of host forms, which synchronise before they return)
    // a failure at context i leaves exports and copies of contexts 0..i-1 in flight: drain them
    auto drain = [&](int launched, int code) {
        for (int j = 0; j < launched && !d->cpu; j++) {
            (void)hipSetDevice(ctxs[j]->device);
            (void)hipStreamSynchronize(ctxs[j]->stream);
        }
        return code;
    };
    for (int i = 0; i < active; i++) {
        rt_context* c = ctxs[i];
        if (c->cpu) {
            if ((rc = export_pass(c, rps, planes, gathered + (size_t)i * blk, nullptr))) return drain(i, rc);
            continue;
        }
        if (hipSetDevice(c->device) != hipSuccess) return drain(i, fail(c, RT_ERR_HIP, "hipSetDevice"));
        if ((rc = ensure_buf(c, c->as_block, blk * sizeof(float)))) return drain(i, rc);
        if ((rc = export_pass(c, rps, planes, c->as_block.as<float>(), c->stream))) return drain(i + 1, rc);
        const hipError_t e =
            c->device == d->device
                ? hipMemcpyAsync(gathered + (size_t)i * blk, c->as_block.p, blk * sizeof(float), hipMemcpyDeviceToDevice,
                                 c->stream)
                : hipMemcpyPeerAsync(gathered + (size_t)i * blk, d->device, c->as_block.p, c->device,
                                     blk * sizeof(float), c->stream);
        if (e != hipSuccess) return drain(i + 1, hip_fail(c, e, "block copy"));
    }
    // the blocks are in place before the assembly is queued (the call synchronises anyway)
    for (int i = 0; i < active && !d->cpu; i++) {
        rt_context* c = ctxs[i];
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    rc = assemble_pass(d, gathered, n, rps, planes, frames, batches, d->stream);
    if (!d->cpu) HIP_TRY(d, hipStreamSynchronize(d->stream));
    return rc;
}

int rt_assembled(const rt_context* c, unsigned* frames_out, unsigned* batches_out) {
    if (!c || !c->assembled_current()) return 0;
    if (frames_out) *frames_out = c->as.frames;
    if (batches_out) *batches_out = c->as.batches;
    return 1;
}

int rt_get_assembled(rt_context* c, float* accum_rgb, float* moments) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    if (!c->as.made) return fail(c, RT_ERR_INVALID_ARGUMENT, "no assembled frame (rt_assemble first)");
    if (moments && c->as.planes != 5)
        return fail(c, RT_ERR_INVALID_ARGUMENT, "the assembled frame has 3 planes: no moments");
    const size_t npix = (size_t)c->as.height * c->as.width;
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

int rt_assemble_drop(rt_context* c) {
    if (!c) return RT_ERR_INVALID_ARGUMENT;
    // the record only: passes still queued on the buffers are ordered by the next assembly's stream waits
    c->as.made = false;
    return RT_OK;
}

float rt_last_assemble_ms(rt_context* c) { return c ? c->assemble.elapsed_ms() : -1.0f; }

}  // extern "C"
