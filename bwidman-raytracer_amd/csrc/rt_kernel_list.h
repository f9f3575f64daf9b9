// rt_kernel_list.h — the render kernels of an adaptive call (rt_adaptive.h):
// work item i is pixel list[i] of the selected pixels' list, whose length stays
// on the device.  A listed pixel continues its own accumulation: the lane loads
// its RNG state and frameSum (always: n_p >= 2), starts at frame n_p + 1 and
// renders K.samples frames; it stores RNG state and frameSum (the RGBA of the
// whole frame is the resolve pass's).  Per-pixel arithmetic is rt_path.h's, so
// a listed pixel ends with the bits a uniform render stopped at its frame count
// would give it.
//
//   rt_render_list_kernel          the sorted kernel's round machinery (task
//                                  queue, three barriers, record stack) over list
//                                  items instead of tile items; brute-force scenes
//   rt_render_list_simple_kernel   one path per lane, persistent lanes taking
//                                  items g, g + T, ...: BVH scenes and
//                                  samplesPerPixel > 1 (as the launch policy sends
//                                  those to the simple kernel), and the A/B
//                                  reference of the queued one
//
// The one-path-per-lane kernel is rt_kernel_lane.h's lane_loop with LIST, the
// text the NEE kernel takes too; load_list_item and store_list_pixel live there
// and serve the queued kernel as well.  The queued kernel keeps its own copy of
// rt_kernel_sorted.h's round loop: shared fragments would change that product
// kernel's instruction stream (as the pair kernel's would,
// profiles/kernel_split/dropped.txt).
// Exact units only: the reference-fast mode has no adaptive render.
#pragma once
#include <cstdio>

#include "rt_kernel_lane.h"
#include "rt_kernel_sorted.h"  // RT_GREC_*, RT_SPEC_PRIO
#include "rt_launch.h"

#ifndef RT_FAST
// ---- one path per lane ----------------------------------------------------------
template <int BLOCK, bool HIT_LDS, bool BVH>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(RT_WAVES_PER_EU)))
rt_render_list_simple_kernel(rt_kparams K, rt_list_args L) {
    lane_loop<BLOCK, HIT_LDS, BVH, true, false>(K, rt_nee_args{nullptr, 0, 0}, L);
}

// ---- queued (rt_kernel_sorted.h's round loop over list items) ------------------
// One item per lane: the grid covers the worst case, every pixel listed, and a
// group whose first item lies behind the list returns before its first barrier.
// No launch-order feedback, no sky table.
template <int BLOCK, bool HIT_LDS, bool GREC, bool QUADS>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(GREC ? RT_GREC_WAVES : RT_WAVES_PER_EU)))
rt_render_list_kernel(rt_kparams K, rt_list_args L) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const long n_list = (long)*L.list_n;  // one scalar load
    if ((long)blockIdx.x * BLOCK >= n_list) return;  // group-uniform
    const float* hit_tab = K.hit;
    float* rec_base = smem;
    if (HIT_LDS) {
        rec_base = stage_hit_table<BLOCK>(K, smem, tid);
        hit_tab = smem;
    }
    // record levels as the sorted kernel's: 0 .. max_bounces-1 in LDS (GREC: the
    // shallow ones, the deep ones in global memory), the deepest folded from
    // the lane's own task slot
    const int levels = K.max_bounces;
    const int LL = GREC ? (levels < RT_GREC_LDS_LEVELS ? levels : RT_GREC_LDS_LEVELS) : levels;
    lds_float* rec = (lds_float*)(rec_base + tid);
    const int GL = levels - LL;
    float* grec = GREC ? K.rec + (long)blockIdx.x * 3 * GL * BLOCK + tid : rec_base;
    float* slots = rec_base + 3 * LL * BLOCK;
    int* counters = reinterpret_cast<int*>(slots + 13 * BLOCK);
    const long npix = (long)K.rows * K.width;
    if (tid < 4) counters[tid] = 0;
    __syncthreads();
#define LSLOT(f, i) slots[(f) * BLOCK + (i)]
#define LRES(f, i) slots[((f) < 4 ? (f) : (f) + 3) * BLOCK + (i)]

    PixelState px;
    load_list_item(K, L, npix, n_list, (long)blockIdx.x * BLOCK + tid, px);
    int mode = px.passes_left > 0 ? T_REGEN : T_NONE;

    f3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
    f3 hn = o;  // pending hit's normal (its point is o)
    int hid = 0, depth = 0;
    bool has_ray = false;
    int parity = 0;
    const f3 cam = mk(K.cam_pos[0], K.cam_pos[1], K.cam_pos[2]);

    // path end: fold, accumulate (Main.cu:299-304), next frame
    auto finish_path = [&](int slot) {
        float lx = K.bg[0], ly = K.bg[1], lz = K.bg[2];  // backgroundColor (Main.cu:209-211)
        if (depth > K.max_bounces)  // deepest level, parked in the slot
            fold_level(__float_as_int(LSLOT(6, slot)), LSLOT(4, slot), LSLOT(5, slot), hit_tab, lx, ly, lz);
        const int nrec = depth > K.max_bounces ? K.max_bounces : depth;
        if (GREC)
            for (int l = nrec - 1; l >= LL; --l) {
                const float* r = grec + 3 * (l - LL) * BLOCK;
                fold_level(__float_as_int(r[0]), r[BLOCK], r[2 * BLOCK], hit_tab, lx, ly, lz);
            }
        for (int l = (nrec < LL ? nrec : LL) - 1; l >= 0; --l) {
            const lds_float* r = rec + 3 * l * BLOCK;
            fold_level(__float_as_int(r[0]), r[BLOCK], r[2 * BLOCK], hit_tab, lx, ly, lz);
        }
        accumulate_frame(px, lx, ly, lz);
        mode = px.passes_left > 0 ? T_REGEN : T_NONE;
    };
    bool ended = false;  // path ended this round: finish_path() once, after the I-phase

    while (true) {
        const int task = mode;
        // every owner has read its previous task result out of the slots
        // before any wave overwrites them with this round's tasks
        __syncthreads();

        // ---- T-phase: enqueue (front: RANDDIR, back: SPEC)
        int* cnt = counters + 2 * parity;
        const bool front = task == T_REGEN || task == T_DIFF;
        const unsigned long long mf = __ballot(front);
        const unsigned long long mbk = __ballot(task == T_SPEC);
        int base_f = 0, base_b = 0;
        if (lane == 0) {
            if (mf) base_f = atomicAdd(&cnt[0], __popcll(mf));
            if (mbk) base_b = atomicAdd(&cnt[1], __popcll(mbk));
        }
        base_f = __builtin_amdgcn_readfirstlane(base_f);
        base_b = __builtin_amdgcn_readfirstlane(base_b);
        int slot = -1;
        if (front) slot = base_f + lanes_below(mf);
        if (task == T_SPEC) slot = BLOCK - 1 - (base_b + lanes_below(mbk));
        if (slot >= 0) {
            const f3 nrm = task == T_REGEN ? px.d0 : hn;
            LSLOT(0, slot) = nrm.x;
            LSLOT(1, slot) = nrm.y;
            LSLOT(2, slot) = nrm.z;
            LSLOT(3, slot) = d.x;
            LSLOT(4, slot) = d.y;
            LSLOT(5, slot) = d.z;
            // code: primitive id (bounce) or -1 (camera ray)
            LSLOT(6, slot) = __int_as_float(task == T_REGEN ? -1 : hid);
            RS_PUT(px.rs, LSLOT, 7, slot);
        }
        __syncthreads();
        // no task anywhere in the workgroup: the group is done
        const int nf = cnt[0], nb = cnt[1];
        if (nf + nb == 0) break;

        // ---- T-phase: execute slot `tid`
        {
            const bool do_front = tid < nf;
            const bool do_spec = tid >= BLOCK - nb;
#if RT_SPEC_PRIO
            const int wave_first = (int)__builtin_amdgcn_readfirstlane((unsigned)(tid & ~63));
            const bool spec_wave = wave_first + 63 >= BLOCK - nb;
            if (spec_wave) __builtin_amdgcn_s_setprio(RT_SPEC_PRIO);
#endif
            if (do_front || do_spec) {
                Xorwow rs;
                RS_GET(rs, LSLOT, 7, tid);
                const f3 nrm = mk(LSLOT(0, tid), LSLOT(1, tid), LSLOT(2, tid));
                const int code = __float_as_int(LSLOT(6, tid));
                f3 r;
                if (do_front) {
                    r = random_direction(rs, nrm);
                    if (code < 0) r = normalize3(add(nrm, scale(K.jitter, r)));  // camera jitter, Main.cu:291-292
                } else {
                    const f3 dd = mk(LSLOT(3, tid), LSLOT(4, tid), LSLOT(5, tid));
                    const float4 h2 = *reinterpret_cast<const float4*>(hit_tab + RT_HIT_FLOATS * code + 8);
                    float kspec;
                    r = specular_scatter(rs, dd, nrm, h2.x, h2.z, h2.y, kspec);
                    LRES(3, tid) = kspec;
                }
                LRES(0, tid) = r.x;
                LRES(1, tid) = r.y;
                LRES(2, tid) = r.z;
                RS_PUT(rs, LRES, 4, tid);
            }
        }
#if RT_SPEC_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
        __syncthreads();
        if (tid == 0) {
            counters[2 * (parity ^ 1)] = 0;
            counters[2 * (parity ^ 1) + 1] = 0;
        }
        parity ^= 1;

        // ---- owner: take the task result back
        if (slot >= 0) {
            d = mk(LRES(0, slot), LRES(1, slot), LRES(2, slot));
            RS_GET(px.rs, LRES, 4, slot);
            mode = T_NONE;
            if (task == T_REGEN) {
                o = cam;
                depth = 0;
                has_ray = true;
            } else {
                const int code = task == T_SPEC ? ~hid : hid;
                const float kspec = task == T_SPEC ? LRES(3, slot) : 0.0f;
                const float cosang = dot(d, hn);  // cosAngle, Main.cu:264
                if (depth < K.max_bounces) {
                    if (!GREC || depth < LL) {  // (separate stores: LDS and global address spaces)
                        lds_float* r = rec + 3 * depth * BLOCK;
                        r[0] = __int_as_float(code);
                        r[BLOCK] = kspec;
                        r[2 * BLOCK] = cosang;
                    } else {
                        float* r = grec + 3 * (depth - LL) * BLOCK;
                        r[0] = __int_as_float(code);
                        r[BLOCK] = kspec;
                        r[2 * BLOCK] = cosang;
                    }
                    has_ray = true;  // from the hit point o along d
                } else {  // next query would exceed maxBounces (Main.cu:210): the path ends
                    LSLOT(4, slot) = kspec;
                    LSLOT(5, slot) = cosang;
                    LSLOT(6, slot) = __int_as_float(code);
                    ended = true;
                }
                depth++;
            }
        }

        // ---- I-phase: closest hit + brdfChoice (Main.cu:214-245)
        float t = INFINITY;
        int id = -1;
        if (has_ray) closest_hit_brute<QUADS>(K, o, d, t, id);
        if (has_ray) {
            has_ray = false;
            if (id >= 0) {
                const float4 h0 = *reinterpret_cast<const float4*>(hit_tab + RT_HIT_FLOATS * id);
                o = add(o, scale(t, d));  // the hit point: the next ray's origin
                hn = mk(h0.x, h0.y, h0.z);
                if (h0.w != 0.0f) hn = normalize3(sub(o, hn));  // sphere normal
                hid = id;
                mode = rand_range(px.rs, 1.0f) < RT_SPECULAR_CHANCE ? T_SPEC : T_DIFF;
            } else {
                ended = true;
            }
        }
        if (ended) {
            ended = false;
            finish_path(slot);
        }
    }
    if (px.valid && px.passes_left == 0) store_list_pixel(K, npix, px);
#undef LSLOT
#undef LRES
}

namespace {
// which: 0 the policy, 1 the one-path-per-lane kernel, 2 the queued one
// (BWRT_ADAPTIVE_KERNEL; BVH scenes and samplesPerPixel > 1 always take 1)
template <int BLOCK, bool HIT_LDS, bool BVH>
hipError_t launch_list_simple(const rt_kparams& K0, const rt_list_args& L, size_t lds, int num_cus, hipStream_t stream) {
    rt_kparams K = K0;
    // persistent lanes: at most the resident groups (the list is usually a
    // fraction of the frame, and a group behind it returns at once)
    const long grid = rt_lane_grid(reinterpret_cast<const void*>(&rt_render_list_simple_kernel<BLOCK, HIT_LDS, BVH>), BLOCK,
                                   lds, (long)K.rows * K.width, 1, num_cus);
    K.rec = nullptr;
    K.group_cost = nullptr;
    K.group_order = nullptr;
    K.sky = nullptr;
    hipLaunchKernelGGL((rt_render_list_simple_kernel<BLOCK, HIT_LDS, BVH>), dim3((unsigned)grid), dim3(BLOCK), lds, stream,
                       K, L);
    std::snprintf(rt_launched_kernel, sizeof rt_launched_kernel, "rt_render_kernel<%d%s%s,list>", BLOCK,
                  HIT_LDS ? "" : ",hit_global", BVH ? ",bvh" : "");
    return hipGetLastError();
}

template <int BLOCK, bool HIT_LDS, bool GREC>
hipError_t launch_list_queued(const rt_kparams& K0, const rt_list_args& L, size_t lds, hipStream_t stream) {
    rt_kparams K = K0;
    const long npix = (long)K.rows * K.width;
    long grid = (npix + BLOCK - 1) / BLOCK;
    if (grid < 1) grid = 1;
    K.rec_stride = (int)(grid * BLOCK);
    K.group_cost = nullptr;
    K.group_order = nullptr;
    K.sky = nullptr;
    if (K.n_quad > 0)
        hipLaunchKernelGGL((rt_render_list_kernel<BLOCK, HIT_LDS, GREC, true>), dim3((unsigned)grid), dim3(BLOCK), lds,
                           stream, K, L);
    else
        hipLaunchKernelGGL((rt_render_list_kernel<BLOCK, HIT_LDS, GREC, false>), dim3((unsigned)grid), dim3(BLOCK), lds,
                           stream, K, L);
    std::snprintf(rt_launched_kernel, sizeof rt_launched_kernel, "rt_render_list_kernel<%d%s%s>", BLOCK,
                  HIT_LDS ? "" : ",hit_global", GREC ? ",grec" : "");
    return hipGetLastError();
}

template <int BLOCK>
hipError_t launch_list_queued_block(const rt_kparams& K, const rt_list_args& L, bool hit_lds, size_t lds, hipStream_t s) {
    if (K.rec)
        return hit_lds ? launch_list_queued<BLOCK, true, true>(K, L, lds, s)
                       : launch_list_queued<BLOCK, false, true>(K, L, lds, s);
    return hit_lds ? launch_list_queued<BLOCK, true, false>(K, L, lds, s)
                   : launch_list_queued<BLOCK, false, false>(K, L, lds, s);
}
}  // namespace

#ifdef RT_LIST_ROOT_BVH
// the BVH unit's instantiations (hit table in global memory, wave-synchronous walk)
hipError_t rt_launch_render_list_bvh(const rt_kparams& K, const rt_list_args& L, int block, size_t lds, int num_cus,
                                     hipStream_t s) {
    return block == 64 ? launch_list_simple<64, false, true>(K, L, lds, num_cus, s)
                       : launch_list_simple<256, false, true>(K, L, lds, num_cus, s);
}
#else
// Launch policy of an adaptive call's render: block size, hit-table and record
// placement as a uniform render's (rt_small_block, rt_hit_in_lds, K.rec from
// rt_render_wants_global_records, rt_render_lds_bytes).
bool rt_render_list_queued(const rt_kparams& K, int which) {
    return !K.bvh_nodes && K.spp_inner <= 1 && which != 1;
}
hipError_t rt_launch_render_list(const rt_kparams& K, const rt_list_args& L, int num_cus, int which, hipStream_t s) {
    const bool hit_lds = rt_hit_in_lds(K);
    const int block = rt_small_block(K) ? 64 : 256;
    if (!rt_render_list_queued(K, which)) {
        rt_kparams S = K;
        S.rec = nullptr;
        const size_t lds = rt_render_lds_bytes(S, block, hit_lds, false);
        if (K.bvh_nodes) return rt_launch_render_list_bvh(S, L, block, lds, num_cus, s);
        if (block == 64)
            return hit_lds ? launch_list_simple<64, true, false>(S, L, lds, num_cus, s)
                           : launch_list_simple<64, false, false>(S, L, lds, num_cus, s);
        return hit_lds ? launch_list_simple<256, true, false>(S, L, lds, num_cus, s)
                       : launch_list_simple<256, false, false>(S, L, lds, num_cus, s);
    }
    const size_t lds = rt_render_lds_bytes(K, block, hit_lds, true);
    return block == 64 ? launch_list_queued_block<64>(K, L, hit_lds, lds, s)
                       : launch_list_queued_block<256>(K, L, hit_lds, lds, s);
}
#endif
#endif  // !RT_FAST
