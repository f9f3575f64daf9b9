// rt_group.h — what the entry points over several contexts and over shard
// blocks share (rt_render_multi, rt_assemble*_multi, rt_render_adaptive_multi;
// rt_export_shard*, rt_assemble*, rt_adaptive_export_rows*,
// rt_render_adaptive_shard*), and the preamble of the _device entry points.
// Plain functions; every refusal is the failure on the context named `on`.
// Private to csrc/.
#pragma once
#include "rt_context.h"

// ---- a list of contexts -----------------------------------------------------------
// The list scan: a null entry, a context of the other kind, a repeated one.
// `on`: the context that reports; null: the entry itself, and a null entry is
// the bare code (rt_render_multi, which takes GPU contexts only: gpu_only).
// Else the kinds must not be mixed: every entry as `on`.
inline int group_scan(rt_context* const* ctxs, int n, rt_context* on, const char* name, bool gpu_only = false) {
    for (int i = 0; i < n; i++) {
        if (!ctxs[i]) return on ? fail(on, RT_ERR_INVALID_ARGUMENT, "null context %d", i) : RT_ERR_INVALID_ARGUMENT;
        rt_context* d = on ? on : ctxs[i];
        if (gpu_only && ctxs[i]->cpu) return fail(d, RT_ERR_UNSUPPORTED, "%s: CPU context", name);
        if (!gpu_only && ctxs[i]->cpu != d->cpu)
            return fail(d, RT_ERR_INVALID_ARGUMENT, "%s: GPU and CPU contexts mixed", name);
        for (int j = 0; j < i; j++)
            if (ctxs[j] == ctxs[i]) return fail(d, RT_ERR_INVALID_ARGUMENT, "context listed twice");
    }
    return RT_OK;
}

// n contexts over `height` rows, context i rows i, i + n, ...: the contexts
// that hold rows (those beyond the image height hold none) and the rows of one
// block plane
inline int group_active(int n, int height) { return n < height ? n : height; }
inline int group_rows_per_shard(int n, int height) { return (height + n - 1) / n; }

// Context i holds shard i of n of width x height and has state (`stride`: its
// row stride as the caller reads it)
inline int group_shard_check(rt_context* on, const rt_context* c, int i, int n, int stride, int width, int height) {
    if (c->width == width && c->height == height && c->row_offset == i && stride == n && c->accum.p) return RT_OK;
    return fail(on, RT_ERR_INVALID_ARGUMENT, "context %d holds %dx%d offset %d stride %d, not shard %d of %d of %dx%d", i,
                c->width, c->height, c->row_offset, c->row_stride, i, n, width, height);
}

// Context i is as far as context 0 (`first`): the frame counters, and with
// `batches` the tracked batches, are equal
inline int group_counters_check(rt_context* on, const rt_context* c, int i, const rt_context* first, bool batches) {
    if (!batches) {
        if (c->st.frame() == first->st.frame()) return RT_OK;
        return fail(on, RT_ERR_INVALID_ARGUMENT, "frame counters differ (context %d: %u, context 0: %u)", i, c->st.frame(),
                    first->st.frame());
    }
    if (c->st.frame() == first->st.frame() && c->st.batches() == first->st.batches()) return RT_OK;
    return fail(on, RT_ERR_INVALID_ARGUMENT, "frame counters or batches differ (context %d: %u, %u; context 0: %u, %u)", i,
                c->st.frame(), c->st.batches(), first->st.frame(), first->st.batches());
}

// A failure at context i leaves work of the contexts before it in flight:
// wait for the first `launched` contexts' streams, whatever that returns
inline int group_drain(rt_context* const* ctxs, int launched, int code) {
    for (int j = 0; j < launched; j++) {
        if (ctxs[j]->cpu) continue;
        (void)hipSetDevice(ctxs[j]->device);
        (void)hipStreamSynchronize(ctxs[j]->stream);
    }
    return code;
}

// Wait for the streams of the first `active` contexts
inline int group_sync(rt_context* const* ctxs, int active) {
    for (int i = 0; i < active; i++) {
        rt_context* c = ctxs[i];
        if (c->cpu) continue;
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return RT_OK;
}

// `bytes` of device memory from context `from` to context `to`, on from's
// stream: on one device, or between peers
inline hipError_t group_copy(void* dst, const rt_context* to, const void* src, const rt_context* from, size_t bytes) {
    return to->device == from->device ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, from->stream)
                                      : hipMemcpyPeerAsync(dst, to->device, src, from->device, bytes, from->stream);
}

// ---- the geometry of a block (rt_layout.h rt_asm_args) ----------------------------
// a block plane has room for the context's rows
inline int block_rows_check(rt_context* c, int rows_per_shard) {
    if (rows_per_shard >= c->rows) return RT_OK;
    return fail(c, RT_ERR_INVALID_ARGUMENT, "rows_per_shard %d below the shard's %d rows", rows_per_shard, c->rows);
}
// a block plane's words are indexed in 32 bits
inline int block_plane_check(rt_context* c, int rows_per_shard) {
    if ((long long)rows_per_shard * c->width <= (1ll << 31)) return RT_OK;
    return fail(c, RT_ERR_UNSUPPORTED, "block plane larger than 2^31 words");
}
// `shards` blocks cover the frame's rows (`what`: "assembly", "gather")
inline int block_cover_check(rt_context* c, const char* what, int shards, int rows_per_shard) {
    if (shards >= 1 && rows_per_shard >= 1 && (long long)rows_per_shard * shards >= c->height) return RT_OK;
    return fail(c, RT_ERR_INVALID_ARGUMENT, "bad %s geometry: %d shards of %d rows for height %d", what, shards,
                rows_per_shard, c->height);
}

// ---- the _device entry points -----------------------------------------------------
// A device pointer of the call with its name; `required`: null is refused
struct DevPtr {
    const void* p;
    const char* name;
    bool required;
};
// Entry point `name` takes a GPU context and its required pointers: the null
// refusal, then the CPU context's
inline int device_ctx(rt_context* c, const char* name, std::initializer_list<DevPtr> ptrs = {}) {
    bool missing = !c;
    for (const DevPtr& d : ptrs) missing = missing || (d.required && !d.p);
    if (missing) return fail(c, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (c->cpu) return fail(c, RT_ERR_UNSUPPORTED, "%s: CPU context", name);
    return RT_OK;
}
// Kernels move 4-byte words through every pointer of the call
inline int device_aligned(rt_context* c, std::initializer_list<DevPtr> ptrs) {
    for (const DevPtr& d : ptrs)
        if ((uintptr_t)d.p & 3u) return fail(c, RT_ERR_INVALID_ARGUMENT, "%s not 4-byte aligned", d.name);
    return RT_OK;
}
// the caller's stream, or the context's
inline hipStream_t device_stream(const rt_context* c, void* stream) { return stream ? (hipStream_t)stream : c->stream; }
// The three in this order (entry points that check their parameters before the
// alignment call them one by one): RT_OK and the stream of the call, or the failure
inline int device_call(rt_context* c, const char* name, std::initializer_list<DevPtr> ptrs, void* stream, hipStream_t* s) {
    if (const int rc = device_ctx(c, name, ptrs)) return rc;
    if (const int rc = device_aligned(c, ptrs)) return rc;
    *s = device_stream(c, stream);
    return RT_OK;
}
