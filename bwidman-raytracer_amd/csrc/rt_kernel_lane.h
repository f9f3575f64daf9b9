// rt_kernel_lane.h — one path per lane on persistent lanes, written once for the
// kernels that are not among the measured product kernels: the list render of
// an adaptive call (rt_kernel_list.h, LIST) and next-event estimation
// (rt_kernel_nee.h, NEE, with or without LIST).  Their __global__ entry points
// are one call of lane_loop each.  rt_kernel_simple.h's rt_render_kernel is the
// same loop without LIST and NEE and keeps its own text (see its header).
// Exact units only.
//
// The loop: regenerate, closest hit, shade, record, fold, accumulate, next item
// (lane g takes items g, g + T, ...).  LIST: item i is pixel list[i] of an
// adaptive call, which continues its own accumulation (rt_kernel_list.h).
//
// NEE (rt_light.h has the estimator) adds the lane's NEE
// state, the suppression, the three draws and the shadow ray.  Where the shadow
// ray is traced (measured):
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
// LDS layout: [hit table, if HIT_LDS] then the record stack,
// RT_LANE_REC_DWORDS(NEE) dwords per level per lane, lane-minor: code, k,
// cosang, and with NEE aux (rt_light.h).
#pragma once
#include "rt_hit.h"
#include "rt_light.h"

#ifndef RT_NEE_INLINE_BRUTE
#define RT_NEE_INLINE_BRUTE 1
#endif
#ifndef RT_NEE_INLINE_BVH
#define RT_NEE_INLINE_BVH 0
#endif

#ifndef RT_FAST
namespace {
// item i of an adaptive call's list (i >= n_list: none): the lane loads the
// pixel's RNG state and frameSum (always: n_p >= 2) and starts at frame n_p + 1
__device__ __forceinline__ void load_list_item(const rt_kparams& K, const rt_list_args& L, long npix, long n_list,
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
__device__ __forceinline__ void store_list_pixel(const rt_kparams& K, long npix, const PixelState& s) {
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

// The body of a one-path-per-lane kernel of BLOCK lanes.  N is read only with
// NEE, L only with LIST.  PICK (NEE only): how nee_sample picks its light
// (rt_light.h); the weighted pick walks the light table with a wave-uniform
// index, so its records come through the scalar data path; the tree pick
// (RT_PICK_TREE) descends the light tree with a node index of the lane's own,
// vector loads of a small cached table.  SHAPES (NEE only):
// RT_SHAPES_ALL where the table holds polygon lights (rt_set_light_shapes); the
// lanes of a wave then pick lights of both kinds, and what follows the sampled
// direction (the cs test, wc, k, the shadow ray) is nee_sample's one tail.
template <int BLOCK, bool HIT_LDS, bool BVH, bool LIST, bool NEE, int PICK = RT_PICK_UNIFORM, int SHAPES = RT_SHAPES_SPHERES>
__device__ __forceinline__ void lane_loop(const rt_kparams& K, const rt_nee_args& N, const rt_list_args& L) {
    constexpr bool INLINE = BVH ? RT_NEE_INLINE_BVH != 0 : RT_NEE_INLINE_BRUTE != 0;
    extern __shared__ float smem[];
    const int tid = threadIdx.x;
    long n_list = 0;
    if constexpr (LIST) {
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
    constexpr int REC = RT_LANE_REC_DWORDS(NEE);  // planes: code, k, cosang, and last aux (NEE)
    static_assert(REC == (NEE ? 4 : 3), "the record planes below");
    const int levels = K.max_bounces + 1;
    int* rec_code = reinterpret_cast<int*>(rec_base) + tid;
    float* rec_k = rec_base + levels * BLOCK + tid;
    float* rec_c = rec_base + 2 * levels * BLOCK + tid;
    [[maybe_unused]] int* rec_aux = reinterpret_cast<int*>(rec_base) + (REC - 1) * levels * BLOCK + tid;

    const long npix = (long)K.rows * K.width;
    const long T = (long)gridDim.x * BLOCK;
    const long nitems = LIST ? n_list : items_of(K, npix);
    PixelState px;
    if constexpr (LIST)
        load_list_item(K, L, npix, n_list, (long)blockIdx.x * BLOCK + tid, px);
    else
        load_item(K, npix, nitems, (long)blockIdx.x * BLOCK + tid, px);

    f3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
    int depth = -1;  // -1: needs a camera ray for its next frame
    const f3 cam = mk(K.cam_pos[0], K.cam_pos[1], K.cam_pos[2]);
    // samplesPerPixel (Main.cu:296-299): the frame's camera ray and the
    // paths still to trace from it
    f3 dcam = d;
    int inner = 1;
    // NEE state of the lane: the ray (o, d) is the shadow ray of level
    // depth - 1 towards primitive shadow_prim (-1: an ordinary ray), whose
    // scattered direction waits in scat; nee_prim >= 0: (o, d) is the scattered
    // ray of an NEE level on that primitive (its point is o)
    [[maybe_unused]] f3 scat = d;
    [[maybe_unused]] int shadow_prim = -1, nee_prim = -1;

    while (true) {
        // (1) regenerate: jittered camera ray (Main.cu:290-292)
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
            // (2) closest hit (Main.cu:214-234; NEE && !INLINE: the only call of the loop)
            float t;
            int id;
            closest_hit<BVH>(K, o, d, t, id);

            if constexpr (NEE && !INLINE) {
                if (shadow_prim >= 0) {
                    // the shadow ray of level depth - 1: visible iff it ends on the light
                    if (id == shadow_prim) rec_aux[(depth - 1) * BLOCK] |= RT_NEE_VISIBLE;
                    shadow_prim = -1;
                    d = scat;
                    continue;
                }
            }
            bool finished = true;
            if (id >= 0) {
                // (3) shade (Main.cu:237-264)
                const float* h = hit_tab + RT_HIT_FLOATS * id;
                const float4 h0 = *reinterpret_cast<const float4*>(h);
                const float4 h2 = *reinterpret_cast<const float4*>(h + 8);
                const f3 P = add(o, scale(t, d));
                f3 n = mk(h0.x, h0.y, h0.z);
                if (h0.w != 0.0f) n = normalize3(sub(P, n));  // sphere: centre -> normal
                [[maybe_unused]] int aux = 0;
                if constexpr (NEE) {
                    if (nee_prim >= 0 && light_suppressed<SHAPES>(K, N, o, nee_prim, id)) aux = RT_NEE_DROP;
                    nee_prim = -1;
                }
                f3 scatter;
                int code = id;
                float k = 0.0f;  // specular brdf scalar, or an NEE level's weight
                const float choice = rand_range(px.rs, 1.0f);
                if (choice < RT_SPECULAR_CHANCE) {
                    scatter = specular_scatter(px.rs, d, n, h2.x, h2.z, h2.y, k);
                    code = ~id;
                } else {
                    scatter = random_direction(px.rs, n);  // brdf = 4 * albedo
                    if constexpr (NEE) {
                        const int kind = nee_normal_kind(h0.w != 0.0f, n);
                        if (depth + 1 <= K.max_bounces && N.n_lights > 0 && kind) {
                            const NeeSample s = nee_sample<PICK, SHAPES>(px.rs, N, P, n, id, kind);
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
                }
                rec_code[depth * BLOCK] = code;
                rec_k[depth * BLOCK] = k;
                // cosAngle (Main.cu:264) of the scattered direction (parked in scat behind a shadow ray)
                if constexpr (NEE) {
                    rec_c[depth * BLOCK] = dot(shadow_prim >= 0 ? scat : scatter, n);
                    rec_aux[depth * BLOCK] = aux;
                } else {
                    rec_c[depth * BLOCK] = dot(scatter, n);
                }
                depth++;
                o = P;
                d = scatter;
                finished = depth > K.max_bounces;  // Main.cu:210
            }
            if (finished) {
                // (4) fold the recursion innermost-first (Main.cu:262-268)
                float lx = K.bg[0], ly = K.bg[1], lz = K.bg[2];  // backgroundColor
                if constexpr (NEE) {
                    nee_prim = -1;
                    for (int l = depth - 1; l >= 0; --l)
                        fold_level_nee(rec_code[l * BLOCK], rec_k[l * BLOCK], rec_c[l * BLOCK], rec_aux[l * BLOCK], hit_tab, N,
                                       lx, ly, lz);
                } else {
                    for (int l = depth - 1; l >= 0; --l)
                        fold_level(rec_code[l * BLOCK], rec_k[l * BLOCK], rec_c[l * BLOCK], hit_tab, lx, ly, lz);
                }
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
                // (5) progressive accumulation (Main.cu:299-304)
                accumulate_frame(px, lx, ly, lz);
                depth = -1;
                if (px.passes_left == 0) {  // pixel done: write back, take the next item
                    if constexpr (LIST) {
                        store_list_pixel(K, npix, px);
                        load_list_item(K, L, npix, n_list, px.w + T, px);
                    } else {
                        store_pixel(K, npix, px);
                        load_item(K, npix, nitems, px.w + T, px);
                    }
                }
            }
        }
    }
}
}  // namespace
#endif  // !RT_FAST
