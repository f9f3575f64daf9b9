// rt_kernel_sorted.h — the sorted task-queue megakernel (the product path) and its sky groups.
#pragma once
#include "rt_hit.h"

// Divergence, not memory, bounds the simple one-path-per-lane kernel: in a
// wave, lanes that need a camera ray, a specular bounce or a diffuse bounce
// execute all three code paths one after the other (rocprof: 20 of 64 lanes
// active per VALU instruction).  Here each workgroup iterates in lock-step:
//
//   T-phase: every lane with pending work posts ONE task into an LDS queue:
//            RANDDIR tasks (camera-jitter direction for a new frame, or a
//            diffuse bounce: both are genRandomDirection, Main.cu:193-206)
//            fill slots from the front, SPEC tasks (Main.cu:245-255) from
//            the back; wave w then executes slots 64w..64w+63, so each wave
//            runs one task kind (at most one wave holds both).  The task
//            carries the lane's RNG state (6 x u32) and returns it updated,
//            so every pixel still consumes its own stream in reference order.
//   I-phase: every lane with a ray runs closest_hit (uniform code), draws its
//            brdfChoice, and posts the shading task for the next T-phase; a
//            miss (or the depth limit) folds the path's records, accumulates
//            the frame and schedules the pixel's next camera ray.
//
// LDS: [hit table][record stack 3 x levels x BLOCK]
//      [task slots 13 x BLOCK, field-major][2 x 2 queue counters]
// GREC: the record levels >= RT_GREC_LDS_LEVELS in global memory (deep paths
// and full frames, launch policy).  BVH scenes take the ray-refill kernel.
// RT_NT_GREC (A/B knob, default 0): a global record's one read, at the path's
// fold, non-temporal
#ifndef RT_NT_GREC
#define RT_NT_GREC 0
#endif
// occupancy target of the sorted kernel with global-memory records (LDS no
// longer bounds it): 7 waves/SIMD (config 4: 6.36 -> 6.08 ms vs the default
// target; 8 spills and gains nothing)
#ifndef RT_GREC_WAVES
#define RT_GREC_WAVES 7
#endif
// global-record launches keep this many shallow record levels in LDS
// (3 dwords per level per lane; 2 still fits 7 waves/SIMD of the sorted kernel)
#ifndef RT_GREC_LDS_LEVELS
#define RT_GREC_LDS_LEVELS 2
#endif
// s_setprio of the wave that runs SPEC tasks during the execute step (the
// longest wave there; measured 0.882 -> 0.876 ms); 0 disables
#ifndef RT_SPEC_PRIO
#define RT_SPEC_PRIO 3
#endif
namespace {
// A group whose wave tiles are all sky (rt_sky.h): every camera ray of its
// pixels misses, so a frame is the jitter's rejection loop (ball_try: the
// draws of genRandomDirection, Main.cu:193-197; its normalisation, the
// hemisphere flip and the camera ray draw nothing, and the miss discards
// them) and frameSum += backgroundColor with finish_path's operations.  No
// barrier, no LDS; the whole group takes it, so no wave is left at a barrier.
template <int BLOCK, bool ORDER>
__device__ __forceinline__ void render_sky_group(const rt_kparams& K, long group) {
    const int tid = threadIdx.x;
    unsigned t0 = 0u;
    if (ORDER) t0 = (unsigned)__builtin_amdgcn_s_memrealtime();
    const long npix = (long)K.rows * K.width;
    const long nitems = items_of(K, npix);
    PixelState px;
    load_item(K, npix, nitems, group * BLOCK + tid, px);  // (d0 is unused here: the compiler drops primary_dir)
    const float lx = K.bg[0], ly = K.bg[1], lz = K.bg[2];  // backgroundColor (Main.cu:209-211)
    // One loop over the draws, not one per frame: a lane whose point is
    // accepted starts its next frame's draws in the next trip instead of
    // waiting for the wave's slowest rejection loop (a wave then runs the
    // largest per-lane SUM of trips, about half the sum of per-frame maxima;
    // each lane's draws, tests and adds are the same sequence either way)
    while (px.passes_left > 0) {
        if (!ball_try(px.rs)) continue;
        accumulate_frame(px, lx, ly, lz);
    }
    if (px.valid && px.frame != K.first_frame) store_pixel(K, npix, px);
    // launch-order feedback: the group's span, as the round loop records it
    // (every wave of a sky group does the same work: wave 0's span stands for all)
    if (ORDER && tid == 0) K.group_cost[group] = (unsigned)__builtin_amdgcn_s_memrealtime() - t0;
}

// The call the kernel makes.  Not inlined: inlined, the sky path's address
// arithmetic shares and re-allocates the round loop's scalar registers (the
// product kernel went from 68 VGPRs and no spilled SGPR to 69 and 2, with 313
// changed stretches of its instruction stream, `make asm`).  A callee gets
// its arguments in vector registers and no kernel-argument base of its own,
// so the kernel passes the argument segment's address and the callee makes it
// scalar again (readfirstlane): the parameters then come through scalar loads.
typedef const __attribute__((address_space(4))) rt_kparams* kparams_ptr;
template <int BLOCK, bool ORDER>
__device__ __attribute__((noinline)) void render_sky_group_call(kparams_ptr kp_v, int group_v) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass has no address-space-4 copy)
    const unsigned long long a = (unsigned long long)kp_v;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const kparams_ptr kp = (kparams_ptr)(((unsigned long long)hi << 32) | lo);
    const rt_kparams K = *kp;
    render_sky_group<BLOCK, ORDER>(K, (long)__builtin_amdgcn_readfirstlane(group_v));
#endif
}
}  // namespace

RT_MODE_BEGIN
template <int BLOCK, bool HIT_LDS, bool GREC, bool ORDER = false, bool QUADS = true>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(GREC ? RT_GREC_WAVES : RT_WAVES_PER_EU)))
rt_render_sorted_kernel(rt_kparams K) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // sky groups (rt_sky.h): every tile of the group proven sky on the host.
    // Group-uniform (two scalar loads), decided before the first barrier
    if (K.sky) {
        constexpr unsigned WPB = BLOCK / 64, ALL = (1u << WPB) - 1u;
        const long sgroup = order_group<ORDER>(K);
        const unsigned first = (unsigned)sgroup * WPB;  // WPB divides 32: the bits lie in one word
        if (((K.sky[first >> 5] >> (first & 31)) & ALL) == ALL) {
            render_sky_group_call<BLOCK, ORDER>((kparams_ptr)__builtin_amdgcn_kernarg_segment_ptr(), (int)sgroup);
            return;
        }
    }
    const float* hit_tab = K.hit;
    float* rec_base = smem;
    if (HIT_LDS) {
        rec_base = stage_hit_table<BLOCK>(K, smem, tid);
        hit_tab = smem;
    }
    // levels 0 .. max_bounces-1 in LDS; the deepest level (max_bounces) ends
    // the path in the round it is made, so it is folded straight from the
    // lane's own task slot (fields 4..6, free once the result is taken)
    const int levels = K.max_bounces;
    // record stack: LDS [level][field][lane] (a level's three fields BLOCK
    // dwords apart: one per-lane address, the fields as immediate offsets);
    // GREC: only the shallow levels 0 .. LL-1 in LDS, the deep ones (rarely
    // reached) in global memory, [group][level - LL][field][lane] (each
    // group's records contiguous and coalesced), so LDS leaves room for
    // RT_GREC_WAVES waves and few records ever leave the CU
    const int LL = GREC ? (levels < RT_GREC_LDS_LEVELS ? levels : RT_GREC_LDS_LEVELS) : levels;
    // (an LDS-address-space pointer: 32-bit address arithmetic, no 64-bit
    // base held across the loop)
    lds_float* rec = (lds_float*)(rec_base + tid);
    const int GL = levels - LL;
    float* grec = GREC ? K.rec + (long)blockIdx.x * 3 * GL * BLOCK + tid : rec_base;
    float* slots = rec_base + 3 * LL * BLOCK;
    int* counters = reinterpret_cast<int*>(slots + 13 * BLOCK);
    // counters[0..3]: queue fronts/backs (2 parities)
    const long npix = (long)K.rows * K.width;
    const long nitems = items_of(K, npix);
    if (tid < 4) counters[tid] = 0;
    diag_group_start(K);
    __syncthreads();
#define SLOT(f, i) slots[(f) * BLOCK + (i)]
// task results {r.xyz, kspec, rng[6]}, written back over the slot's own
// fields {0..3, 7..12}
#define RES(f, i) slots[((f) < 4 ? (f) : (f) + 3) * BLOCK + (i)]

    // tile-group of this workgroup (launch-order feedback, rt_layout.h)
    // ORDER: launch-order feedback instantiation (the pointers it needs after
    // the loop cost SGPRs, so launches without feedback use the plain one)
    const long group = order_group_start<ORDER>(K, tid);
    PixelState px;
    // (tid < BLOCK always holds; the guard keeps the register allocation and
    // schedule of the measured kernel: without it the instruction stream
    // differs in 55 places, `make asm`)
    load_item(K, npix, nitems, tid < BLOCK ? group * BLOCK + tid : nitems, px);
    int mode = px.passes_left > 0 ? T_REGEN : T_NONE;

    f3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
    f3 hn = o;  // pending hit's normal (its point is o)
    int hid = 0, depth = 0;
    bool has_ray = false;
    int parity = 0;
    const f3 cam = mk(K.cam_pos[0], K.cam_pos[1], K.cam_pos[2]);

    // path end: fold, accumulate (Main.cu:299-304), next frame / next pixel
    auto finish_path = [&](int slot) {
        // L = emitted + (brdf * L) * cosAngle, innermost level first; `x`
        // reads each record value (identity; opaque in RT_PHASE_TWICE == 4)
        auto fold_path = [&](auto x, float& lx, float& ly, float& lz) {
            if (depth > K.max_bounces)  // deepest level, parked in the slot
                fold_level(__float_as_int(x(SLOT(6, slot))), x(SLOT(4, slot)), x(SLOT(5, slot)), hit_tab, lx, ly, lz);
            const int nrec = depth > K.max_bounces ? K.max_bounces : depth;
            if (GREC)
                for (int l = nrec - 1; l >= LL; --l) {
                    const float* r = grec + 3 * (l - LL) * BLOCK;
                    // (RT_NT_GREC: the record's last read, non-temporal)
                    auto ld = [](const float* a) { return RT_NT_GREC ? __builtin_nontemporal_load(a) : *a; };
                    fold_level(__float_as_int(x(ld(&r[0]))), x(ld(&r[BLOCK])), x(ld(&r[2 * BLOCK])), hit_tab, lx, ly, lz);
                }
            for (int l = (nrec < LL ? nrec : LL) - 1; l >= 0; --l) {
                const lds_float* r = rec + 3 * l * BLOCK;
                fold_level(__float_as_int(x(r[0])), x(r[BLOCK]), x(r[2 * BLOCK]), hit_tab, lx, ly, lz);
            }
        };
        float lx = K.bg[0], ly = K.bg[1], lz = K.bg[2];  // backgroundColor (Main.cu:209-211)
        fold_path(DiagIdent(), lx, ly, lz);
        RT_TWICE_FOLD(K, fold_path);
        accumulate_frame(px, lx, ly, lz);
        // one pixel per lane (the grid covers every work item): a finished
        // pixel is stored after the loop, by the whole wave at once, and the
        // camera set-up constants are not live inside the loop
        mode = px.passes_left > 0 ? T_REGEN : T_NONE;
    };
    bool ended = false;  // path ended this round: finish_path() once, after the I-phase

    SortedStamps dg;  // diagnostic builds only (rt_diag.h)
    while (true) {
        const int task = mode;
        dg.stamp(7);
        // every owner has read its previous task result out of the slots
        // before any wave overwrites them with this round's tasks
        __syncthreads();
        dg.stamp(0);

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
            SLOT(0, slot) = nrm.x;
            SLOT(1, slot) = nrm.y;
            SLOT(2, slot) = nrm.z;
            SLOT(3, slot) = d.x;
            SLOT(4, slot) = d.y;
            SLOT(5, slot) = d.z;
            // code: primitive id (bounce) or -1 (camera ray)
            SLOT(6, slot) = __int_as_float(task == T_REGEN ? -1 : hid);
            RS_PUT(px.rs, SLOT, 7, slot);
        }
        dg.stamp(1);
        __syncthreads();
        dg.stamp(2);
        // no task anywhere in the workgroup: every lane is idle (rays are
        // always consumed in the round that made them), so the group is done
        const int nf = cnt[0], nb = cnt[1];
        if (nf + nb == 0) break;

        // ---- T-phase: execute slot `tid`
        {
            const bool do_front = tid < nf;
            const bool do_spec = tid >= BLOCK - nb;
#if RT_SPEC_PRIO
            // the SPEC wave is the longest of the execute step: let it issue first
            const int wave_first = (int)__builtin_amdgcn_readfirstlane((unsigned)(tid & ~63));
            const bool spec_wave = wave_first + 63 >= BLOCK - nb;
            if (spec_wave) __builtin_amdgcn_s_setprio(RT_SPEC_PRIO);
#endif
            if (do_front || do_spec) {
                Xorwow rs;
                RS_GET(rs, SLOT, 7, tid);
                const f3 nrm = mk(SLOT(0, tid), SLOT(1, tid), SLOT(2, tid));
                const int code = __float_as_int(SLOT(6, tid));
                f3 r;
                if (do_front) {
                    RT_TWICE_RANDDIR(rs, nrm);
                    r = random_direction(rs, nrm, dg.rej_ptr());
                    if (code < 0) r = normalize3(add(nrm, scale(K.jitter, r)));  // camera jitter, Main.cu:291-292
                } else {
                    const f3 dd = mk(SLOT(3, tid), SLOT(4, tid), SLOT(5, tid));
                    const float4 h2 = *reinterpret_cast<const float4*>(hit_tab + RT_HIT_FLOATS * code + 8);
                    float kspec;
                    RT_TWICE_SPEC(rs, dd, nrm, h2);
                    r = specular_scatter(rs, dd, nrm, h2.x, h2.z, h2.y, kspec);
                    RES(3, tid) = kspec;
                }
                RES(0, tid) = r.x;
                RES(1, tid) = r.y;
                RES(2, tid) = r.z;
                RS_PUT(rs, RES, 4, tid);
            }
            dg.exec(do_front, do_spec);
        }
        dg.stamp(3);
#if RT_SPEC_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
        __syncthreads();
        dg.stamp(4);
        if (tid == 0) {
            counters[2 * (parity ^ 1)] = 0;
            counters[2 * (parity ^ 1) + 1] = 0;
        }
        parity ^= 1;

        // ---- owner: take the task result back.  The result direction goes
        // straight into d and the pending hit point already is o (I-phase),
        // so no ray registers are copied here
        if (slot >= 0) {
            d = mk(RES(0, slot), RES(1, slot), RES(2, slot));
            RS_GET(px.rs, RES, 4, slot);
            mode = T_NONE;
            if (task == T_REGEN) {
                o = cam;
                depth = 0;
                has_ray = true;
            } else {
                const int code = task == T_SPEC ? ~hid : hid;
                const float kspec = task == T_SPEC ? RES(3, slot) : 0.0f;
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
                    SLOT(4, slot) = kspec;
                    SLOT(5, slot) = cosang;
                    SLOT(6, slot) = __int_as_float(code);
                    ended = true;
                }
                depth++;
            }
        }

        dg.stamp(5);
        dg.rays(has_ray);
        // ---- I-phase: closest hit + brdfChoice (Main.cu:214-245)
        float t = INFINITY;
        int id = -1;
        if (has_ray) {
            RT_TWICE_HIT(QUADS, K, o, d);
            closest_hit_brute<QUADS>(K, o, d, t, id);
        }
        if (has_ray) {
            has_ray = false;
            if (id >= 0) {
                const float4 h0 = *reinterpret_cast<const float4*>(hit_tab + RT_HIT_FLOATS * id);
                o = add(o, scale(t, d));  // the hit point: the next ray's origin
                hn = mk(h0.x, h0.y, h0.z);
                if (h0.w != 0.0f) hn = normalize3(sub(o, hn));  // sphere normal
                hid = id;
                // brdfChoice (Main.cu:243): specular or diffuse bounce next round
                mode = rand_range(px.rs, 1.0f) < RT_SPECULAR_CHANCE ? T_SPEC : T_DIFF;
            } else {
                ended = true;
            }
        }
        if (ended) {
            ended = false;
            finish_path(slot);
        }
        dg.stamp(6);
    }
    if (px.valid && px.passes_left == 0 && px.frame != K.first_frame) store_pixel(K, npix, px);
    // the loop exit is group-uniform (the round that posts no task), so one
    // lane's clock after the loop closes the group's span
    if (ORDER && tid == 0) {
        // the pointers re-read from the kernel arguments (volatile), so they
        // are not held in SGPRs across the loop
        const volatile __attribute__((address_space(4))) rt_kparams* kp =
            (const volatile __attribute__((address_space(4))) rt_kparams*)__builtin_amdgcn_kernarg_segment_ptr();
        int* const ord = kp->group_order;
        unsigned* const cost = kp->group_cost;
        const long g = ord ? (long)__builtin_nontemporal_load(&ord[blockIdx.x]) : (long)blockIdx.x;
        cost[g] = (unsigned)__builtin_amdgcn_s_memrealtime() - cost[g];
    }
    diag_group_end<true>(K);
    dg.flush(K);
#undef SLOT
#undef RES
}
RT_MODE_END
