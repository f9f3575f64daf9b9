// rt_kernel_nee.h — the render kernel of next-event estimation
// (rt_set_light_sampling; rt_light.h has the estimator):
// one path per lane on persistent lanes.  Exact units only.
//
// The kernel is rt_kernel_lane.h's lane_loop with NEE (and LIST for an adaptive
// call's list): the loop, the list helpers and the record layout are the ones
// the list render takes.  What is this header's own: the entry point with its
// occupancy target (RT_NEE_WAVES), the launch policy with its 4-dword block-size
// rule, the kernel's name, and the choice between the uniform, the weighted and
// the tree instantiation (PICK, rt_set_light_picking and rt_set_light_hierarchy;
// DESIGN.md sections 24 and 29) and between
// the sphere-only and the polygon-aware one (SHAPES, rt_set_light_shapes;
// DESIGN.md section 25).  It shares
// no text with rt_kernel_simple.h's rt_render_kernel, whose instruction stream
// stays as it is (see there).
#pragma once
#include <cstdio>

#include "rt_kernel_lane.h"
#include "rt_launch.h"

// occupancy target (waves per SIMD) of the NEE kernel
#ifndef RT_NEE_WAVES
#define RT_NEE_WAVES RT_WAVES_PER_EU
#endif

#ifndef RT_FAST
template <int BLOCK, bool HIT_LDS, bool BVH, bool LIST, int PICK = RT_PICK_UNIFORM, int SHAPES = RT_SHAPES_SPHERES>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(RT_NEE_WAVES)))
rt_render_nee_kernel(rt_kparams K, rt_nee_args N, rt_list_args L) {
    lane_loop<BLOCK, HIT_LDS, BVH, LIST, true, PICK, SHAPES>(K, N, L);
}

namespace {
// Launch: the grid covers every item once, or with grid_mult > 0 (and always
// for a list, which is usually a fraction of the frame) at most the resident
// groups per CU x CUs (rt_lane_grid).  No launch-order feedback, no sky table.
// PICK: N.pick, which the kernel takes at compile time (rt_set_light_picking;
// RT_PICK_TREE where rt_set_light_hierarchy acts, rt_context::nee_args).
// SHAPES: RT_SHAPES_ALL iff the table the render sees holds a polygon record.
template <int BLOCK, bool HIT_LDS, bool BVH, bool LIST, int PICK, int SHAPES>
hipError_t launch_nee(const rt_kparams& K0, const rt_nee_args& N, const rt_list_args& L, size_t lds, int grid_mult,
                      int num_cus, hipStream_t stream) {
    rt_kparams K = K0;
    if (LIST && grid_mult <= 0) grid_mult = 1;
    const long grid = rt_lane_grid(reinterpret_cast<const void*>(&rt_render_nee_kernel<BLOCK, HIT_LDS, BVH, LIST, PICK, SHAPES>), BLOCK, lds,
                                   LIST ? (long)K.rows * K.width : launch_items(K), grid_mult, num_cus);
    K.rec = nullptr;
    K.rec_stride = (int)(grid * BLOCK);
    K.group_cost = nullptr;
    K.group_order = nullptr;
    K.sky = nullptr;
    hipLaunchKernelGGL((rt_render_nee_kernel<BLOCK, HIT_LDS, BVH, LIST, PICK, SHAPES>), dim3((unsigned)grid), dim3(BLOCK), lds,
                       stream, K, N, L);
    std::snprintf(rt_launched_kernel, sizeof rt_launched_kernel, "rt_render_nee_kernel<%d%s%s%s%s%s>", BLOCK,
                  HIT_LDS ? "" : ",hit_global", BVH ? ",bvh" : "", LIST ? ",list" : "",
                  PICK == RT_PICK_WEIGHTED ? ",weighted" : PICK == RT_PICK_TREE ? ",tree" : "", SHAPES == RT_SHAPES_ALL ? ",polygons" : "");
    return hipGetLastError();
}

template <int BLOCK, bool HIT_LDS, bool BVH, int SHAPES>
hipError_t launch_nee_pick(const rt_kparams& K, const rt_nee_args& N, const rt_list_args* L, size_t lds, int grid_mult,
                           int num_cus, hipStream_t s) {
    const rt_list_args none = {nullptr, nullptr, nullptr};
    if (N.pick == RT_PICK_TREE) {
        if (L) return launch_nee<BLOCK, HIT_LDS, BVH, true, RT_PICK_TREE, SHAPES>(K, N, *L, lds, grid_mult, num_cus, s);
        return launch_nee<BLOCK, HIT_LDS, BVH, false, RT_PICK_TREE, SHAPES>(K, N, none, lds, grid_mult, num_cus, s);
    }
    if (N.pick == RT_PICK_WEIGHTED) {
        if (L) return launch_nee<BLOCK, HIT_LDS, BVH, true, RT_PICK_WEIGHTED, SHAPES>(K, N, *L, lds, grid_mult, num_cus, s);
        return launch_nee<BLOCK, HIT_LDS, BVH, false, RT_PICK_WEIGHTED, SHAPES>(K, N, none, lds, grid_mult, num_cus, s);
    }
    if (L) return launch_nee<BLOCK, HIT_LDS, BVH, true, RT_PICK_UNIFORM, SHAPES>(K, N, *L, lds, grid_mult, num_cus, s);
    return launch_nee<BLOCK, HIT_LDS, BVH, false, RT_PICK_UNIFORM, SHAPES>(K, N, none, lds, grid_mult, num_cus, s);
}

// (a table without a polygon record, whatever the mode: the sphere-only kernel)
template <int BLOCK, bool HIT_LDS, bool BVH>
hipError_t launch_nee_form(const rt_kparams& K, const rt_nee_args& N, const rt_list_args* L, size_t lds, int grid_mult,
                           int num_cus, hipStream_t s) {
    if (N.n_lights > N.n_sphere_lights)
        return launch_nee_pick<BLOCK, HIT_LDS, BVH, RT_SHAPES_ALL>(K, N, L, lds, grid_mult, num_cus, s);
    return launch_nee_pick<BLOCK, HIT_LDS, BVH, RT_SHAPES_SPHERES>(K, N, L, lds, grid_mult, num_cus, s);
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
bool rt_nee_small_block(const rt_kparams& K) {
    return (size_t)RT_LANE_REC_DWORDS(true) * (K.max_bounces + 1) * 256 * sizeof(float) > 49152;
}
// Launch policy of an NEE render (L non-null: an adaptive call's list): block
// size by the rule above, the hit table in LDS under rt_hit_in_lds
hipError_t rt_launch_render_nee(const rt_kparams& K, const rt_nee_args& N, const rt_list_args* L, int num_cus, int grid_mult,
                                hipStream_t s) {
    const bool hit_lds = rt_hit_in_lds(K);
    const int block = rt_nee_small_block(K) ? 64 : 256;
    const size_t lds = rt_lane_lds_bytes(K, block, hit_lds, true);
    if (K.bvh_nodes) return rt_launch_render_nee_bvh(K, N, L, block, lds, grid_mult, num_cus, s);
    if (block == 64)
        return hit_lds ? launch_nee_form<64, true, false>(K, N, L, lds, grid_mult, num_cus, s)
                       : launch_nee_form<64, false, false>(K, N, L, lds, grid_mult, num_cus, s);
    return hit_lds ? launch_nee_form<256, true, false>(K, N, L, lds, grid_mult, num_cus, s)
                   : launch_nee_form<256, false, false>(K, N, L, lds, grid_mult, num_cus, s);
}
#endif
#endif  // !RT_FAST
