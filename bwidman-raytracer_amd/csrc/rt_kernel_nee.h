// rt_kernel_nee.h — the render kernel of next-event estimation
// (rt_set_light_sampling; rt_light.h has the estimator):
// one path per lane on persistent lanes, a copy of rt_kernel_simple.h's loop
// (and, LIST, of rt_kernel_list.h's item handling) that shares no fragment with
// them, so their instruction streams stay as they are.  Exact units only.
//
// Where the shadow ray is traced (measured):
//  * BVH instantiations: one closest_hit call site per loop iteration.  A lane
//    whose bounce took the NEE branch parks its scattered direction, spends its
//    next iteration on the shadow ray and then goes on with the scattered ray,
//    so the wave stays converged through the one wave-synchronous walk (c5:
//    221 ms against 279 ms with a second walk inside the diffuse branch).
//  * brute-force instantiations: a second call inside the diffuse branch (the
//    loop over a few primitives is cheap next to an iteration's fixed work:
//    headline frame 1.56 ms against 1.70 ms deferred, its 1/8 shard 0.45
//    against 0.46).
// RT_NEE_INLINE_BRUTE / RT_NEE_INLINE_BVH (A/B builds) choose per kind.
//
// LDS layout: [hit table, if HIT_LDS] then the record stack, 4 dwords per level
// per lane, lane-minor: code, k, cosang, aux (rt_light.h).
#pragma once
#include <cstdio>

#include "rt_hit.h"
#include "rt_launch.h"
#include "rt_light.h"

#ifndef RT_NEE_INLINE_BRUTE
#define RT_NEE_INLINE_BRUTE 1
#endif
#ifndef RT_NEE_INLINE_BVH
#define RT_NEE_INLINE_BVH 0
#endif
// occupancy target (waves per SIMD) of the NEE kernel
#ifndef RT_NEE_WAVES
#define RT_NEE_WAVES RT_WAVES_PER_EU
#endif

#ifndef RT_FAST
namespace {
// item i of an adaptive call's list (rt_kernel_list.h load_list_item, copied)
__device__ __forceinline__ void nee_load_list_item(const rt_kparams& K, const rt_list_args& L, long npix, long n_list,
                                                   long i, PixelState& s) {
    s.w = i;
    s.valid = i < n_list;
    s.passes_left = 0;
    s.frame = 0u;
    s.p = npix;
    if (!s.valid) return;
    const long p = (long)L.list[i];
    s.p = p;
    const int j = (int)(p / K.width);
    const int x = (int)(p - (long)j * K.width);
    const int y = K.row_offset + j * K.row_stride;
    s.rs.d = px_ld(&K.rng[0 * npix + p]);
    s.rs.v0 = px_ld(&K.rng[1 * npix + p]);
    s.rs.v1 = px_ld(&K.rng[2 * npix + p]);
    s.rs.v2 = px_ld(&K.rng[3 * npix + p]);
    s.rs.v3 = px_ld(&K.rng[4 * npix + p]);
    s.rs.v4 = px_ld(&K.rng[5 * npix + p]);
    s.ax = px_ld(&K.accum[0 * npix + p]);
    s.ay = px_ld(&K.accum[1 * npix + p]);
    s.az = px_ld(&K.accum[2 * npix + p]);
    s.d0 = primary_dir(K, x, y);
    s.frame = L.cnt[p].x + 1u;
    s.passes_left = K.samples;
}

// (the RGBA of a listed pixel is the resolve pass's)
__device__ __forceinline__ void nee_store_list_pixel(const rt_kparams& K, long npix, const PixelState& s) {
    const long p = s.p;
    px_st(&K.rng[0 * npix + p], s.rs.d);
    px_st(&K.rng[1 * npix + p], s.rs.v0);
    px_st(&K.rng[2 * npix + p], s.rs.v1);
    px_st(&K.rng[3 * npix + p], s.rs.v2);
    px_st(&K.rng[4 * npix + p], s.rs.v3);
    px_st(&K.rng[5 * npix + p], s.rs.v4);
    px_st(&K.accum[0 * npix + p], s.ax);
    px_st(&K.accum[1 * npix + p], s.ay);
    px_st(&K.accum[2 * npix + p], s.az);
}
}  // namespace

template <int BLOCK, bool HIT_LDS, bool BVH, bool LIST>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(RT_NEE_WAVES)))
rt_render_nee_kernel(rt_kparams K, rt_nee_args N, rt_list_args L) {
    constexpr bool INLINE = BVH ? RT_NEE_INLINE_BVH != 0 : RT_NEE_INLINE_BRUTE != 0;
    extern __shared__ float smem[];
    const int tid = threadIdx.x;
    long n_list = 0;
    if (LIST) {
        n_list = (long)*L.list_n;                        // one scalar load
        if ((long)blockIdx.x * BLOCK >= n_list) return;  // group-uniform, before the first barrier
    }
    const float* hit_tab = K.hit;
    float* rec_base = smem;
    if (HIT_LDS) {
        rec_base = stage_hit_table<BLOCK>(K, smem, tid);
        __syncthreads();
        hit_tab = smem;
    }
    const int levels = K.max_bounces + 1;
    int* rec_code = reinterpret_cast<int*>(rec_base) + tid;
    float* rec_k = rec_base + levels * BLOCK + tid;
    float* rec_c = rec_base + 2 * levels * BLOCK + tid;
    int* rec_aux = reinterpret_cast<int*>(rec_base) + 3 * levels * BLOCK + tid;

    const long npix = (long)K.rows * K.width;
    const long T = (long)gridDim.x * BLOCK;
    const long nitems = LIST ? n_list : items_of(K, npix);
    PixelState px;
    if (LIST)
        nee_load_list_item(K, L, npix, n_list, (long)blockIdx.x * BLOCK + tid, px);
    else
        load_item(K, npix, nitems, (long)blockIdx.x * BLOCK + tid, px);

    f3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
    int depth = -1;  // -1: needs a camera ray for its next frame
    const f3 cam = mk(K.cam_pos[0], K.cam_pos[1], K.cam_pos[2]);
    f3 dcam = d;
    int inner = 1;
    // NEE state of the lane: the ray (o, d) is the shadow ray of level
    // depth - 1 towards primitive shadow_prim (-1: an ordinary ray), whose
    // scattered direction waits in scat; nee_prim >= 0: (o, d) is the scattered
    // ray of an NEE level on that primitive (its point is o)
    f3 scat = d;
    int shadow_prim = -1, nee_prim = -1;

    while (true) {
        // (1) regenerate: jittered camera ray
        if (depth < 0 && px.passes_left > 0) {
            f3 jit = random_direction(px.rs, px.d0);
            d = normalize3(add(px.d0, scale(K.jitter, jit)));
            o = cam;
            depth = 0;
            dcam = d;
            inner = K.spp_inner;
        }
        const bool active = depth >= 0;
        if (__ballot(active) == 0ull) break;
        if (active) {
            // (2) closest hit (!INLINE: the only call of the loop)
            float t;
            int id;
            closest_hit<BVH>(K, o, d, t, id);

            if (!INLINE && shadow_prim >= 0) {
                // the shadow ray of level depth - 1: visible iff it ends on the light
                if (id == shadow_prim) rec_aux[(depth - 1) * BLOCK] |= RT_NEE_VISIBLE;
                shadow_prim = -1;
                d = scat;
                continue;
            }
            bool finished = true;
            if (id >= 0) {
                // (3) shade
                const float* h = hit_tab + RT_HIT_FLOATS * id;
                const float4 h0 = *reinterpret_cast<const float4*>(h);
                const float4 h2 = *reinterpret_cast<const float4*>(h + 8);
                const f3 P = add(o, scale(t, d));
                f3 n = mk(h0.x, h0.y, h0.z);
                if (h0.w != 0.0f) n = normalize3(sub(P, n));  // sphere: centre -> normal
                int aux = 0;
                if (nee_prim >= 0 && light_suppressed(K, N, o, nee_prim, id)) aux = RT_NEE_DROP;
                nee_prim = -1;
                f3 scatter;
                int code = id;
                float k = 0.0f;
                const float choice = rand_range(px.rs, 1.0f);
                if (choice < RT_SPECULAR_CHANCE) {
                    scatter = specular_scatter(px.rs, d, n, h2.x, h2.z, h2.y, k);
                    code = ~id;
                } else {
                    scatter = random_direction(px.rs, n);  // brdf = 4 * albedo
                    const int kind = nee_normal_kind(h0.w != 0.0f, n);
                    if (depth + 1 <= K.max_bounces && N.n_lights > 0 && kind) {
                        const NeeSample s = nee_sample(px.rs, N, P, n, id, kind);
                        aux |= RT_NEE_LEVEL | (s.j << RT_NEE_JSHIFT);
                        k = s.k;
                        nee_prim = id;
                        if (s.trace) {
                            if constexpr (INLINE) {
                                float ts;
                                int ids;
                                closest_hit<BVH>(K, P, s.wi, ts, ids);
                                if (ids == s.prim) aux |= RT_NEE_VISIBLE;
                            } else {
                                shadow_prim = s.prim;
                                scat = scatter;
                                scatter = s.wi;
                            }
                        }
                    }
                }
                rec_code[depth * BLOCK] = code;
                rec_k[depth * BLOCK] = k;
                // cosAngle of the scattered direction (parked in scat behind a shadow ray)
                rec_c[depth * BLOCK] = dot(shadow_prim >= 0 ? scat : scatter, n);
                rec_aux[depth * BLOCK] = aux;
                depth++;
                o = P;
                d = scatter;
                finished = depth > K.max_bounces;
            }
            if (finished) {
                // (4) fold the recursion innermost-first
                nee_prim = -1;
                float lx = K.bg[0], ly = K.bg[1], lz = K.bg[2];  // backgroundColor
                for (int l = depth - 1; l >= 0; --l)
                    fold_level_nee(rec_code[l * BLOCK], rec_k[l * BLOCK], rec_c[l * BLOCK], rec_aux[l * BLOCK], hit_tab, N,
                                   lx, ly, lz);
                if (inner > 1) {  // `pixel = tracePath(...)` again from the same camera ray
                    inner--;
                    o = cam;
                    d = dcam;
                    depth = 0;
                    continue;
                }
                if (K.spp_inner != 1) {  // pixel /= samplesPerPixel: (1.0f / k) * pixel
                    const float ki = rt_div(1.0f, (float)K.spp_inner);
                    lx = ki * lx;
                    ly = ki * ly;
                    lz = ki * lz;
                }
                // (5) progressive accumulation
                accumulate_frame(px, lx, ly, lz);
                depth = -1;
                if (px.passes_left == 0) {  // pixel done: write back, take the next item
                    if (LIST) {
                        nee_store_list_pixel(K, npix, px);
                        nee_load_list_item(K, L, npix, n_list, px.w + T, px);
                    } else {
                        store_pixel(K, npix, px);
                        load_item(K, npix, nitems, px.w + T, px);
                    }
                }
            }
        }
    }
}

namespace {
// Launch: the grid covers every item once, or with grid_mult > 0 (and always
// for a list, which is usually a fraction of the frame) at most the resident
// groups per CU x CUs.  No launch-order feedback, no sky table.
template <int BLOCK, bool HIT_LDS, bool BVH, bool LIST>
hipError_t launch_nee(const rt_kparams& K0, const rt_nee_args& N, const rt_list_args& L, size_t lds, int grid_mult,
                      int num_cus, hipStream_t stream) {
    rt_kparams K = K0;
    long grid = ((LIST ? (long)K.rows * K.width : launch_items(K)) + BLOCK - 1) / BLOCK;
    if (LIST && grid_mult <= 0) grid_mult = 1;
    if (grid_mult > 0) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &per_cu, reinterpret_cast<const void*>(&rt_render_nee_kernel<BLOCK, HIT_LDS, BVH, LIST>), BLOCK, lds) ==
                hipSuccess &&
            per_cu > 0) {
            const long cap = (long)per_cu * num_cus * grid_mult;
            if (grid > cap) grid = cap;
        }
    }
    if (grid < 1) grid = 1;
    K.rec = nullptr;
    K.rec_stride = (int)(grid * BLOCK);
    K.group_cost = nullptr;
    K.group_order = nullptr;
    K.sky = nullptr;
    hipLaunchKernelGGL((rt_render_nee_kernel<BLOCK, HIT_LDS, BVH, LIST>), dim3((unsigned)grid), dim3(BLOCK), lds, stream, K,
                       N, L);
    std::snprintf(rt_launched_kernel, sizeof rt_launched_kernel, "rt_render_nee_kernel<%d%s%s%s>", BLOCK,
                  HIT_LDS ? "" : ",hit_global", BVH ? ",bvh" : "", LIST ? ",list" : "");
    return hipGetLastError();
}

template <int BLOCK, bool HIT_LDS, bool BVH>
hipError_t launch_nee_form(const rt_kparams& K, const rt_nee_args& N, const rt_list_args* L, size_t lds, int grid_mult,
                           int num_cus, hipStream_t s) {
    if (L) return launch_nee<BLOCK, HIT_LDS, BVH, true>(K, N, *L, lds, grid_mult, num_cus, s);
    return launch_nee<BLOCK, HIT_LDS, BVH, false>(K, N, rt_list_args{nullptr, nullptr, nullptr}, lds, grid_mult, num_cus, s);
}
}  // namespace

#ifdef RT_NEE_ROOT_BVH
// the BVH unit's instantiations (hit table in global memory, wave-synchronous walk)
hipError_t rt_launch_render_nee_bvh(const rt_kparams& K, const rt_nee_args& N, const rt_list_args* L, int block, size_t lds,
                                    int grid_mult, int num_cus, hipStream_t s) {
    return block == 64 ? launch_nee_form<64, false, true>(K, N, L, lds, grid_mult, num_cus, s)
                       : launch_nee_form<256, false, true>(K, N, L, lds, grid_mult, num_cus, s);
}
#else
// 64-lane groups where the record stack of 256 lanes (4 dwords per level) would
// pass the 48 KB that rt_small_block allows the default kernels' stack
bool rt_nee_small_block(const rt_kparams& K) { return (size_t)4 * (K.max_bounces + 1) * 256 * sizeof(float) > 49152; }
size_t rt_nee_lds_bytes(const rt_kparams& K, int block, bool hit_lds) {
    const int n_prim = K.n_sph + K.n_pln + K.n_tri + K.n_quad;
    const size_t hit = hit_lds ? (size_t)((n_prim * RT_HIT_FLOATS + 3) & ~3) * sizeof(float) : 0;
    return hit + (size_t)4 * (K.max_bounces + 1) * block * sizeof(float);
}
// Launch policy of an NEE render (L non-null: an adaptive call's list): block
// size by the rule above, the hit table in LDS under rt_hit_in_lds
hipError_t rt_launch_render_nee(const rt_kparams& K, const rt_nee_args& N, const rt_list_args* L, int num_cus, int grid_mult,
                                hipStream_t s) {
    const bool hit_lds = rt_hit_in_lds(K);
    const int block = rt_nee_small_block(K) ? 64 : 256;
    const size_t lds = rt_nee_lds_bytes(K, block, hit_lds);
    if (K.bvh_nodes) return rt_launch_render_nee_bvh(K, N, L, block, lds, grid_mult, num_cus, s);
    if (block == 64)
        return hit_lds ? launch_nee_form<64, true, false>(K, N, L, lds, grid_mult, num_cus, s)
                       : launch_nee_form<64, false, false>(K, N, L, lds, grid_mult, num_cus, s);
    return hit_lds ? launch_nee_form<256, true, false>(K, N, L, lds, grid_mult, num_cus, s)
                   : launch_nee_form<256, false, false>(K, N, L, lds, grid_mult, num_cus, s);
}
#endif
#endif  // !RT_FAST
