// rt_kernel_refill.h — the BVH units: the ray-refill kernel (large scenes) and the BVH launchers.
#pragma once
#include "rt_kernel_simple.h"

// One path per lane like rt_render_kernel, but the BVH walk is not a
// wave-synchronous call: each lane keeps its walk state (node, parked leaf,
// closest hit) across iterations, and once K.refill lanes of a wave have
// finished their walks, those lanes shade their hit and set up their next
// ray while the others stay parked mid-walk (persistent traversal with ray
// refill, Aila & Laine 2009), so the node loop runs on fuller waves instead
// of waiting for each round's slowest ray.  A ray's tests and their
// (t, RT_KEY) acceptance are exactly those of closest_hit_bvh (planes
// first, then every primitive of every leaf whose inflated box the ray may
// enter), so the result does not depend on when the lane walks.
// refill threshold K.refill (of 64, relative to the lanes that still hold a
// pixel; rt_layout.h RT_REFILL): with the spatial-split tree and leaf batches
// at 58 ready lanes, config 5 at 32 / 36 / 40 / 48: 96.4 / 95.0 / 94.9 / 97.8
// ms, its 1/8 shard 21.6 / 21.6 / 22.1 / 22.3 ms
// leaf-test batch threshold K.leaf_batch (lanes of 64 ready; rt_layout.h
// RT_LEAF_BATCH): with one parked leaf, config 5 at 52 / 54 / 56 / 58 / 60 /
// 62 / 64 (all lanes, Aila & Laine's rule): 102.2 / 99.1 / 98.1 / 97.3 / 98.2
// / 101.1 / 118.0 ms, its 1/8 shard 24.8 / 23.4 / 23.0 / 22.3 / 22.2 / 22.3 /
// 25.5 ms; with two, 60 / 62: 91.8 / 92.6 ms, 1/8 shard 21.3 / 20.2 ms
// fp16 bits -> float (exact)
__device__ __forceinline__ float h2f(unsigned bits) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)(bits & 0xffffu));
}

// N16: 16-byte nodes (rt_layout.h bvh_nodes16) — one gather per node visit
// instead of two; the walk, its tests and its order are the same.
// ORDER: launch-order feedback as in the sorted kernel (workgroup g renders
// tile-group group_order[g] and records its duration in group_cost[])
// Leaf records in vertex form (rt_layout.h bvh_leafvtx: 64 bytes, the plane
// and inner normals formed in the kernel): config 5 78.6 -> 75.6 ms, 1/2
// shard 43.0 -> 41.4, 1/8 17.63 -> 17.56 (profiles/r05h/ab_vtx_policy.txt);
// the kernel held to 5 waves per SIMD (96 VGPRs; 12 bytes of spills on the
// pixel-load and shading paths)
#ifndef RT_REFILL_WAVES
#define RT_REFILL_WAVES 5
#endif
#ifndef RT_NODE_PAIR
#define RT_NODE_PAIR 1
#endif
RT_MODE_BEGIN
template <int BLOCK, bool N16, bool ORDER = false>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(RT_REFILL_WAVES)))
rt_render_bvh_refill_kernel(rt_kparams K) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x;
    const float* hit_tab = K.hit;
    int* rec_code = reinterpret_cast<int*>(smem) + tid;
    float* rec_k = smem + (K.max_bounces + 1) * BLOCK + tid;
    float* rec_c = smem + 2 * (K.max_bounces + 1) * BLOCK + tid;
    const long npix = (long)K.rows * K.width;
    const long T = (long)gridDim.x * BLOCK;
    const long nitems = items_of(K, npix);
    const long group = order_group_start<ORDER>(K, tid);
    PixelState px;
    load_item(K, npix, nitems, group * BLOCK + tid, px);
    const f3 cam = mk(K.cam_pos[0], K.cam_pos[1], K.cam_pos[2]);
    diag_group_start(K);
    LaneDone lane_done;  // diagnostic builds only (rt_diag.h)

    f3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
    int depth = -1;          // -1: the next ray is a camera ray
    bool walking = false;    // a BVH walk is in flight
    bool pending = false;    // a finished query waits to be shaded
    bool idle = false;       // no pixel left
    int node = -1, leaf = -1, leaf2 = -1;  // two parked leaves per lane
    float best_t = INFINITY;
    int best_id = -1, best_key = -1;
    SlabRay sr;
    sr.inv = o;
    sr.oinv = o;
    sr.m = 0.0f;
    float a2 = 0.0f, a4 = 0.0f;
    const float* nodes = K.bvh_nodes;
    const unsigned* nodes16 = K.bvh_nodes16;
    const int nn = K.bvh_n_nodes;
    // a walk is live while its node indexes the array: -1 (done) and nn (past
    // a leaf that ends the array: a leaf's miss link is simply node + 1) fail
    // the same unsigned compare, and the leaf test reuses the decoded flag —
    // 39 -> 34 VALU per node step: config 5 86.5 -> 85.7 ms, its 1/8 shard
    // 20.1 -> 19.65 (profiles/r05h/ab_node_step.txt); the 16-byte step below
    // (one address instruction, ~w parked directly, one compare per parked
    // leaf) 34 -> 30 VALU, with leaf records loaded in six 16-byte loads
    // instead of seven (rt_path.h leaf_test): 84.8 -> 84.0 ms, 1/8 shard
    // 19.64 -> 19.36 (profiles/r05h/ab_node_step3.txt).  Keeping the parked
    // leaves as loop-carried lane masks (28 VALU) costs more in mask
    // bookkeeping than it saves: +3 %
#define NODE_LIVE(n) ((unsigned)(n) < (unsigned)nn)
    RefillStamps dg;  // diagnostic builds only (rt_diag.h)
    while (true) {
        dg.count(3);
        // (A) lanes without a walk: shade the finished query, start the next ray
        while (!walking && !idle) {
            if (pending) {
                pending = false;
                diag_bvh_check(K, o, d, best_t, best_id, depth);
                bool finished = true;
                if (best_id >= 0) {  // shade (Main.cu:237-264), as rt_render_kernel
                    const float* h = hit_tab + RT_HIT_FLOATS * best_id;
                    const float4 h0 = *reinterpret_cast<const float4*>(h);
                    const float4 h2 = *reinterpret_cast<const float4*>(h + 8);
                    const f3 P = add(o, scale(best_t, d));
                    f3 n = mk(h0.x, h0.y, h0.z);
                    if (h0.w != 0.0f) n = normalize3(sub(P, n));  // sphere: centre -> normal
                    f3 scatter;
                    int code = best_id;
                    float kspec = 0.0f;
                    const float choice = rand_range(px.rs, 1.0f);
                    if (choice < RT_SPECULAR_CHANCE) {
                        scatter = specular_scatter(px.rs, d, n, h2.x, h2.z, h2.y, kspec);
                        code = ~best_id;
                    } else {
                        scatter = random_direction(px.rs, n);  // brdf = 4 * albedo
                    }
                    rec_code[depth * BLOCK] = code;
                    rec_k[depth * BLOCK] = kspec;
                    rec_c[depth * BLOCK] = dot(scatter, n);  // cosAngle, Main.cu:264
                    depth++;
                    o = P;
                    d = scatter;
                    finished = depth > K.max_bounces;  // Main.cu:210
                }
                if (finished) {  // fold (Main.cu:262-268), accumulate (Main.cu:299-304)
                    float lx = K.bg[0], ly = K.bg[1], lz = K.bg[2];
                    for (int l = depth - 1; l >= 0; --l)
                        fold_level(rec_code[l * BLOCK], rec_k[l * BLOCK], rec_c[l * BLOCK], hit_tab, lx, ly, lz);
                    accumulate_frame(px, lx, ly, lz);
                    depth = -1;
                    if (px.passes_left == 0) {
                        store_pixel(K, npix, px);
                        load_item(K, npix, nitems, px.w + T, px);
                    }
                }
            }
            if (depth < 0) {
                if (px.passes_left <= 0) {
                    idle = true;
                    lane_done.mark(K);
                    break;
                }
                // jittered camera ray (Main.cu:290-292)
                const f3 jit = random_direction(px.rs, px.d0);
                d = normalize3(add(px.d0, scale(K.jitter, jit)));
                o = cam;
                depth = 0;
            }
            // set up the walk of (o, d): closest_hit_bvh's prologue
            best_t = INFINITY;
            best_id = -1;
            best_key = -1;
            if (!bvh_safe(K, o, d)) {  // NaN/inf rays, overflowing tests: the reference's interleaved loop
                closest_hit_brute(K, o, d, best_t, best_id);
                pending = true;
                continue;
            }
            const float a = dot(d, d);
            a4 = 4.0f * a;
            a2 = 2.0f * a;
            planes_first(K, o, d, best_t, best_id, best_key);  // planes are unbounded: always tested
            sr = slab_ray(o, d);
            const int order = ray_octant(K, d);
            if (N16)
                nodes16 = K.bvh_nodes16 + (size_t)order * nn * 4;
            else
                nodes = K.bvh_nodes + (size_t)order * K.bvh_order_stride;
            node = 0;
            leaf = -1;
            leaf2 = -1;
            walking = true;
        }
        dg.stamp(0);
        if (__ballot(walking) == 0ull) break;  // every lane idle

        // (B) walk until K.refill lanes are waiting for a new ray
        while (true) {
            while (true) {  // node steps; a lane parks the first two leaves its ray enters
                bool stalled = false;
                if (NODE_LIVE(node)) {  // (a live node implies a walk)
                    RT_BRANCH_COUNT(K, 5);
                    // branch-free step: miss -> skip the subtree; internal -> first
                    // child; leaf -> park it (or stall on a third one)
                    if (N16) {
#define RT_N16_STEP(q)                                                                                        \
    do {                                                                                                      \
        const int w = (int)(q).w; /* miss link (internal) or ~leaf (a leaf's miss link is node + 1) */        \
        const bool lnode = w < -1;                                                                            \
        const bool hit = slab_enter(h2f((q).x), h2f((q).x >> 16), h2f((q).y), h2f((q).y >> 16), h2f((q).z), \
                                    h2f((q).z >> 16), sr, best_t);                                            \
        const bool is_leaf = hit && lnode;                                                                    \
        const bool park = is_leaf && leaf2 < 0;                                                               \
        stalled = is_leaf != park;                                                                            \
        const bool first = park && leaf < 0;                                                                  \
        leaf2 = park != first ? ~w : leaf2;                                                                   \
        leaf = first ? ~w : leaf;                                                                             \
        node = !hit && !lnode ? w : (stalled ? node : node + 1);                                              \
    } while (0)
                        const uint4* nq = reinterpret_cast<const uint4*>(nodes16);
                        const uint4 q = nq[(unsigned)node];
#if RT_NODE_PAIR
                        // the next node in array order is loaded with this one:
                        // a step that moves to node + 1 (an internal hit, a
                        // parked or missed leaf) takes it without a second
                        // round trip — config 5 75.9 -> 74.6 ms, its 1/8
                        // shard flat (profiles/r05h/ab_node_pair.txt); the
                        // node after it too (node + 2): 80.0 ms
                        const int node0 = node;
                        const uint4 q1 = nq[min((unsigned)node + 1u, (unsigned)nn - 1u)];
                        RT_N16_STEP(q);
                        asm volatile("" ::"v"(q1.x), "v"(q1.y), "v"(q1.z), "v"(q1.w));
                        if (node == node0 + 1 && NODE_LIVE(node)) RT_N16_STEP(q1);
#else
                        RT_N16_STEP(q);
#endif
#undef RT_N16_STEP
                    } else {
                        const float4 lo = *reinterpret_cast<const float4*>(nodes + 8 * node);
                        const float4 hi = *reinterpret_cast<const float4*>(nodes + 8 * node + 4);
                        const bool hit = slab_enter(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, sr, best_t);
                        const int miss = __float_as_int(lo.w);
                        const int lf = __float_as_int(hi.w);
                        const bool is_leaf = hit && lf >= 0;
                        const bool park = is_leaf && leaf2 < 0;
                        stalled = is_leaf != park;
                        const bool first = park && leaf < 0;
                        leaf2 = park != first ? lf : leaf2;
                        leaf = first ? lf : leaf;
                        node = !hit || park ? miss : (is_leaf ? node : node + 1);
                    }
                }
                // test the parked leaves once K.leaf_batch of the 64 lanes are
                // ready (a leaf parked, the walk done or stalled, no walk);
                // the rest walk on and join a later batch
                dg.count(4);
                // (a lane without a walk has a dead node, and a stalled lane
                // has a parked leaf; two compare masks OR'd on the scalar
                // side: a ballot of anything but one compare costs a
                // v_cndmask + v_cmp per step — config 5 83.9 -> 81.3 ms, its
                // 1/8 shard 19.2 -> 18.3, profiles/r05h/ab_ballot.txt)
                if (__popcll(__ballot(leaf >= 0) | __ballot(!NODE_LIVE(node))) >= K.leaf_batch) break;
            }
            dg.stamp(1);
            dg.count(5);
            if (leaf >= 0) {
                const int first = leaf & 0xffffff, count = leaf >> 24;
                for (int k = 0; k < count; k++) {
                    RT_BRANCH_COUNT(K, 6);
                    leaf_test<true>(K, K.bvh_leafvtx + (size_t)RT_LEAF_VFLOATS * (first + k), o, d, a2, a4, best_t,
                                    best_id, best_key);
                }
                leaf = -1;
            }
            if (leaf2 >= 0) {
                const int first = leaf2 & 0xffffff, count = leaf2 >> 24;
                for (int k = 0; k < count; k++)
                    leaf_test<true>(K, K.bvh_leafvtx + (size_t)RT_LEAF_VFLOATS * (first + k), o, d, a2, a4, best_t,
                                    best_id, best_key);
                leaf2 = -1;
            }
            dg.stamp(2);
            if (walking && !NODE_LIVE(node)) {  // walk complete: the query result is best_t / best_id
                walking = false;
                pending = true;
            }
            const unsigned long long w = __ballot(walking);
            // K.refill of 64 relative to the lanes that still have a pixel, so a
            // wave's tail (pixels done, lanes idle) keeps refilling: config 5
            // 120.4 -> 117.4 ms, its 1/8 shard 26.6 -> 25.6 ms (absolute count)
            // (all 64 lanes are active here: the finished ones are ~w & ~idle)
            const unsigned long long live = ~__ballot(idle);
            if (w == 0ull || 64 * __popcll(~w & live) >= K.refill * __popcll(live)) break;
        }
    }
    if (ORDER && tid == 0) {  // the loop exit is wave-uniform (one wave per group)
        const long g = K.group_order ? (long)K.group_order[blockIdx.x] : (long)blockIdx.x;
        K.group_cost[g] = (unsigned)__builtin_amdgcn_s_memrealtime() - K.group_cost[g];
    }
    diag_group_end<false>(K);
    dg.flush(K);
#undef NODE_LIVE
}

// ---- launchers of the BVH units (-O3: the traversal loops want the full
// optimizer while the brute-force kernels are faster at -O1)
// the ray-refill kernel, 64-lane groups (no barriers), with launch-order feedback
hipError_t rt_launch_render_bvh_refill(const rt_kparams& K0, int num_cus, hipStream_t s) {
    constexpr int BLOCK = 64;
    const long nitems = launch_items(K0);
    const long grid = (nitems + BLOCK - 1) / BLOCK < 1 ? 1 : (nitems + BLOCK - 1) / BLOCK;
    const size_t lds = (size_t)3 * (K0.max_bounces + 1) * BLOCK * sizeof(float);
    const bool n16 = K0.bvh_nodes16 != nullptr;
    const void* ordered = n16 ? reinterpret_cast<const void*>(&rt_render_bvh_refill_kernel<BLOCK, true, true>)
                              : reinterpret_cast<const void*>(&rt_render_bvh_refill_kernel<BLOCK, false, true>);
    const void* plain = n16 ? reinterpret_cast<const void*>(&rt_render_bvh_refill_kernel<BLOCK, true>)
                            : reinterpret_cast<const void*>(&rt_render_bvh_refill_kernel<BLOCK, false>);
    rt_kparams K = rt_order_begin(K0, grid, ordered, BLOCK, lds, num_cus, false);
    const bool feedback = K.group_cost != nullptr;
    void* args[] = {&K};
    (void)hipLaunchKernel(feedback ? ordered : plain, dim3((unsigned)grid), dim3(BLOCK), args, lds, s);
    std::snprintf(rt_launched_kernel, sizeof rt_launched_kernel, "rt_render_bvh_refill_kernel<64%s%s>%s",
                  n16 ? ",n16" : "", RT_MODE_TAG, feedback ? "+order" : "");
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : rt_order_end(K0, K, grid, s);
}

// BVH scenes with samplesPerPixel > 1 (or BWRT_KERNEL=simple): the
// one-path-per-lane kernel with the wave-synchronous BVH walk
hipError_t rt_launch_render_bvh_simple(const rt_kparams& K, int block, size_t lds, int grid_mult, int num_cus,
                                       hipStream_t s) {
    return block == 64 ? launch_simple<64, false, true>(K, lds, grid_mult, num_cus, s)
                       : launch_simple<256, false, true>(K, lds, grid_mult, num_cus, s);
}
RT_MODE_END

#ifndef RT_FAST  // first-hit features: always the exact arithmetic
hipError_t rt_launch_aov_bvh(const rt_kparams& K, float4* ga, float4* gb, float4* alb, hipStream_t stream) {
    return launch_aov<true>(K, ga, gb, alb, stream);
}
#endif
