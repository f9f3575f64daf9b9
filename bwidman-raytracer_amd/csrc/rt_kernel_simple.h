// rt_kernel_simple.h — one path per lane: the A/B reference of the queued
// kernels, the only kernel with samplesPerPixel > 1 or (BVH units) the
// wave-synchronous BVH walk.
// Hot path of the reference (bwidman-raytracer/src):
//   launchRaytracer  Main.cu:274-315   -> rt_render_kernel
//   tracePath        Main.cu:208-272   -> iterative bounce loop + LDS record fold
//   BRDF helpers     Main.cu:111-206   -> rt_path.h
//   intersections    Intersection.cuh  -> closest_hit()
// In-lane path regeneration: a lane whose path terminated (miss or depth
// limit) starts its next frame's camera ray in the very next iteration
// instead of idling until the wave's longest path ends; a wave-wide ballot
// decides when the wave is done.  Each pixel still consumes its RNG stream
// and accumulates its frames strictly in order, so results are identical to
// the frame-by-frame reference.
//
// The list and NEE kernels run the same loop from one text, rt_kernel_lane.h's
// lane_loop.  This kernel is not routed through it: it is the A/B reference of
// the product kernels in both precision modes, held to "identical instruction
// stream or put back" (profiles/kernel_split/dropped.txt), and it inlines the
// microfacet bounce where lane_loop calls specular_scatter, which changes its
// stream in all four units (dropped.txt item 2; profiles/lane_loop/simple_kernel.txt).
// Shared with them: the per-pixel helpers of rt_pixel.h and rt_path.h, the
// record layout (RT_LANE_REC_DWORDS(false) = the 3 dwords below, sized by
// rt_lane_lds_bytes) and the grid rule (rt_lane_grid).
#pragma once
#include <cstdio>

#include "rt_hit.h"
#include "rt_launch.h"

// LDS layout: [hit table, n_prim*12 floats, if HIT_LDS] then the record stack
// of the recursion, 3 dwords per level per lane, lane-minor:
//   code[l][lane] (int: primitive id, ~id for a specular bounce),
//   kspec[l][lane] (specular brdf scalar), cosang[l][lane]
// (bank = lane: conflict-free for any per-lane depth).
//
// Persistent lanes: the grid covers the GPU once (occupancy-sized); lane g
// renders pixels g, g+T, g+2T, ... (T = lanes in the grid), each for all
// K.samples frames, regenerating its next path in the iteration after the
// previous one ends.  A wave ends when all its lanes ran out of pixels.
RT_MODE_BEGIN
template <int BLOCK, bool HIT_LDS, bool BVH>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(RT_WAVES_PER_EU)))
rt_render_kernel(rt_kparams K) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x;
    const float* hit_tab = K.hit;
    float* rec_base = smem;
    if (HIT_LDS) {
        rec_base = stage_hit_table<BLOCK>(K, smem, tid);
        __syncthreads();
        hit_tab = smem;
    }
    int* rec_code = reinterpret_cast<int*>(rec_base) + tid;
    float* rec_k = rec_base + (K.max_bounces + 1) * BLOCK + tid;
    float* rec_c = rec_base + 2 * (K.max_bounces + 1) * BLOCK + tid;

    const long npix = (long)K.rows * K.width;
    const long T = (long)gridDim.x * BLOCK;
    const long nitems = items_of(K, npix);
    PixelState px;
    load_item(K, npix, nitems, (long)blockIdx.x * BLOCK + tid, px);

    f3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
    int depth = -1;  // -1: needs a camera ray for its next frame
    const f3 cam = mk(K.cam_pos[0], K.cam_pos[1], K.cam_pos[2]);
    // samplesPerPixel (Main.cu:296-299): the frame's camera ray and the
    // paths still to trace from it
    f3 dcam = d;
    int inner = 1;

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
            // (2) closest hit (Main.cu:214-234)
            float t;
            int id;
            closest_hit<BVH>(K, o, d, t, id);

            bool finished = true;
            if (id >= 0) {
                // (3) shade (Main.cu:237-264)
                const float* h = hit_tab + RT_HIT_FLOATS * id;
                const float4 h0 = *reinterpret_cast<const float4*>(h);
                const float4 h1 = *reinterpret_cast<const float4*>(h + 4);
                const float4 h2 = *reinterpret_cast<const float4*>(h + 8);
                const f3 P = add(o, scale(t, d));
                f3 n = mk(h0.x, h0.y, h0.z);
                if (h0.w != 0.0f) n = normalize3(sub(P, n));  // sphere: centre -> normal
                const f3 albedo = mk(h1.x, h1.y, h1.z);
                const float rough = h2.x, ior2m1 = h2.y, rough2 = h2.z;

                f3 scatter;
                int code = id;
                float kspec = 0.0f;
                const float choice = rand_range(px.rs, 1.0f);
                if (choice < RT_SPECULAR_CHANCE) {
                    // genMicrofacetNormal (Main.cu:170-185)
                    const float e1 = rand_range(px.rs, 1.0f);
                    const float e2 = rand_range(px.rs, 1.0f);
                    const float theta = atan_nn(rt_div(rough * rt_sqrt(e1), rt_sqrt(1.0f - e1)));
                    const float phi = 2.0f * RT_PI * e2;
                    float st, ct, sp, cp;
                    rt_sincos(theta, st, ct);
                    rt_sincos(phi, sp, cp);
                    const f3 mloc = mk(st * cp, st * sp, ct);
                    // baseAroundNormalToRegular (Main.cu:149-168)
                    f3 some = mk(1.0f, 0.0f, 0.0f);
                    if (fabsf(dot(n, some)) < 1.0f - RT_NEAR_ZERO) some = mk(0.0f, 1.0f, 0.0f);
                    const f3 t1 = cross(n, some);
                    const f3 t2 = cross(n, t1);
                    const f3 m = mk(dot(mk(t1.x, t2.x, n.x), mloc), dot(mk(t1.y, t2.y, n.y), mloc),
                                    dot(mk(t1.z, t2.z, n.z), mloc));
                    scatter = sub(d, scale(2.0f * dot(d, m), m));  // reflect, Main.cu:187-191
                    const f3 inc = scale(-1.0f, d);
                    const float fr = fresnel(inc, m, ior2m1);
                    const float sw = specular_weight(inc, scatter, n, m, rough2);
                    kspec = rt_div_spec_chance(sw * fr);  // brdf = (s*F/0.5) * {1,1,1}
                    code = ~id;
                } else {
                    scatter = random_direction(px.rs, n);  // brdf = 4 * albedo
                }
                (void)albedo;
                rec_code[depth * BLOCK] = code;
                rec_k[depth * BLOCK] = kspec;
                rec_c[depth * BLOCK] = dot(scatter, n);  // cosAngle, Main.cu:264
                depth++;
                o = P;
                d = scatter;
                finished = depth > K.max_bounces;  // Main.cu:210
            }
            if (finished) {
                // (4) fold the recursion innermost-first (Main.cu:262-268):
                //     L = emitted + (brdf * L) * cosAngle
                float lx = K.bg[0], ly = K.bg[1], lz = K.bg[2];  // backgroundColor
                for (int l = depth - 1; l >= 0; --l)
                    fold_level(rec_code[l * BLOCK], rec_k[l * BLOCK], rec_c[l * BLOCK], hit_tab, lx, ly, lz);
                if (inner > 1) {  // `pixel = tracePath(...)` again from the same camera ray
                    inner--;
                    o = cam;
                    d = dcam;
                    depth = 0;
                    continue;
                }
                if (K.spp_inner != 1) {  // pixel /= samplesPerPixel: (1.0f / k) * pixel
                    const float k = rt_div(1.0f, (float)K.spp_inner);
                    lx = k * lx;
                    ly = k * ly;
                    lz = k * lz;
                }
                // (5) progressive accumulation (Main.cu:299-304)
                accumulate_frame(px, lx, ly, lz);
                depth = -1;
                if (px.passes_left == 0) {  // pixel done: write back, take the next one
                    store_pixel(K, npix, px);
                    load_item(K, npix, nitems, px.w + T, px);
                }
            }
        }
    }
}

namespace {
// Launch of the one-path-per-lane kernel: the grid covers every item once, or
// with grid_mult > 0 (persistent lanes) at most grid_mult x resident groups
// per CU x CUs (rt_lane_grid).  It takes no launch-order feedback.
template <int BLOCK, bool HIT_LDS, bool BVH>
hipError_t launch_simple(const rt_kparams& K0, size_t lds, int grid_mult, int num_cus, hipStream_t stream) {
    rt_kparams K = K0;
    const long grid = rt_lane_grid(reinterpret_cast<const void*>(&rt_render_kernel<BLOCK, HIT_LDS, BVH>), BLOCK, lds,
                                   launch_items(K), grid_mult, num_cus);
    K.rec_stride = (int)(grid * BLOCK);
    K.group_cost = nullptr;
    K.group_order = nullptr;
    hipLaunchKernelGGL((rt_render_kernel<BLOCK, HIT_LDS, BVH>), dim3((unsigned)grid), dim3(BLOCK), lds, stream, K);
    std::snprintf(rt_launched_kernel, sizeof rt_launched_kernel, "rt_render_kernel<%d%s%s%s>", BLOCK,
                  HIT_LDS ? "" : ",hit_global", BVH ? ",bvh" : "", RT_MODE_TAG);
    return hipGetLastError();
}
}  // namespace
RT_MODE_END
