// rt_hit.h — the closest hit a render kernel calls per ray: the brute-force
// loop (rt_path.h closest_hit_brute, Main.cu:214-234 + Intersection.cuh) or
// the wave-synchronous BVH walk; and the first-hit feature kernel over it.
#pragma once
#include "rt_pixel.h"

namespace {
// ---- BVH closest hit (wave-synchronous walk; rt_path.h has the pieces) ----
__device__ __forceinline__ void closest_hit_bvh(const rt_kparams& K, f3 o, f3 d, float& best_t, int& best_id) {
    if (!bvh_safe(K, o, d)) {  // NaN/inf rays, overflowing tests: the reference's interleaved loop
        closest_hit_brute(K, o, d, best_t, best_id);
        return;
    }
    const float a = dot(d, d);
    const float a4 = 4.0f * a;
    const float a2 = 2.0f * a;
    best_t = INFINITY;
    best_id = -1;
    int best_key = -1;
    planes_first(K, o, d, best_t, best_id, best_key);
    const SlabRay sr = slab_ray(o, d);
    // node array of the ray's direction octant (near children first)
    const float* nodes = K.bvh_nodes + (size_t)ray_octant(K, d) * K.bvh_order_stride;
    // speculative while-while traversal (Aila & Laine): a lane that reaches a
    // leaf its ray enters parks it and walks on; the parked leaves are tested
    // together once every lane has one parked (or ran out of nodes, or
    // reached a second leaf, where it waits), so the primitive tests run on
    // full waves and no lane idles in the node loop while others search.
    int node = 0;
    while (true) {
        int leaf = -1;
        while (true) {
            bool stalled = false;
            if (node >= 0) {
                RT_BRANCH_COUNT(K, 5);
                const float4 lo = *reinterpret_cast<const float4*>(nodes + 8 * node);
                const float4 hi = *reinterpret_cast<const float4*>(nodes + 8 * node + 4);
                const bool hit = slab_enter(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, sr, best_t);
                const int miss = __float_as_int(lo.w);
                const int lf = __float_as_int(hi.w);
                if (!hit) {
                    node = miss;
                } else if (lf < 0) {
                    node = node + 1;
                } else if (leaf < 0) {
                    leaf = lf;  // park it, walk on
                    node = miss;
                } else {
                    stalled = true;  // second leaf: revisit after the parked one
                }
            }
            if (__all(leaf >= 0 || node < 0 || stalled)) break;
        }
        if (!__any(leaf >= 0)) break;
        if (leaf >= 0) {
            const int first = leaf & 0xffffff, count = leaf >> 24;
            for (int k = 0; k < count; k++) {
                RT_BRANCH_COUNT(K, 6);
                leaf_test(K, K.bvh_leafrec + (size_t)RT_LEAF_FLOATS * (first + k), o, d, a2, a4, best_t, best_id,
                          best_key);
            }
        }
    }
}

template <bool BVH, bool QUADS = true>
__device__ __forceinline__ void closest_hit(const rt_kparams& K, f3 o, f3 d, float& best_t, int& best_id) {
    if (BVH)
        closest_hit_bvh(K, o, d, best_t, best_id);
    else
        closest_hit_brute<QUADS>(K, o, d, best_t, best_id);
}
}  // namespace

// ---- first-hit feature buffers (rt_render_aov, the denoiser's guides) -------
// One lane per shard pixel: the closest hit of the un-jittered primary ray
// (no RNG draw) through the renders' own routines, shaded by aov_shade
// (rt_path.h), stored packed so that a filter tap is two 16-byte loads:
// ga = {n.xyz, prim as bits}, gb = {P.xyz, depth}; alb = {albedo, 0} (may be
// null).  Always the exact arithmetic: defined at global scope (outside the
// precision-mode namespace) and instantiated once, the brute-force loop in the
// shared unit (rt_kernels_shared.hip), the BVH walk in the exact BVH unit (-O3).
// closest_hit_bvh is wave-synchronous (__all / __any): a lane past the end of
// the shard stays in the call with a clamped pixel and only skips the stores.
template <bool BVH>
__global__ void __launch_bounds__(256) rt_aov_kernel(const rt_kparams K, float4* __restrict__ ga,
                                                     float4* __restrict__ gb, float4* __restrict__ alb) {
    const long npix = (long)K.rows * K.width;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < npix;
    const long p = valid ? i : npix - 1;
    const int j = (int)(p / K.width);
    const int x = (int)(p - (long)j * K.width);
    const int y = K.row_offset + j * K.row_stride;
    const f3 o = mk(K.cam_pos[0], K.cam_pos[1], K.cam_pos[2]);
    const f3 d = primary_dir(K, x, y);
    float t;
    int id;
    closest_hit<BVH>(K, o, d, t, id);
    const AovHit a = aov_shade(K, o, d, t, id);
    if (valid) {
        ga[p] = make_float4(a.n.x, a.n.y, a.n.z, __int_as_float(a.prim));
        gb[p] = make_float4(a.P.x, a.P.y, a.P.z, a.depth);
        if (alb) alb[p] = make_float4(a.albedo.x, a.albedo.y, a.albedo.z, 0.0f);
    }
}

template <bool BVH>
hipError_t launch_aov(const rt_kparams& K, float4* ga, float4* gb, float4* alb, hipStream_t stream) {
    const long npix = (long)K.rows * K.width;
    if (npix <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_aov_kernel<BVH>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, K, ga, gb, alb);
    return hipGetLastError();
}
