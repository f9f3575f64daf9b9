// rt_launch.h — the launchers of the render units (rt_kernels*.hip), declared
// once for the host units (rt_context.h) and the kernel units.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_layout.h"

// ---- per precision mode (rt_launch_brute.h; rt_fast: the reference-fast units)
bool rt_render_wants_global_records(const rt_kparams& K, int num_cus);
hipError_t rt_launch_render(const rt_kparams& K, int num_cus, int grid_mult, bool simple, int block_req,
                            hipStream_t stream, int pair_req);
namespace rt_fast {
bool rt_render_wants_global_records(const rt_kparams& K, int num_cus);
hipError_t rt_launch_render(const rt_kparams& K, int num_cus, int grid_mult, bool simple, int block_req,
                            hipStream_t stream, int pair_req);
}  // namespace rt_fast

// ---- the list render of an adaptive call (rt_kernel_list.h; exact units only)
// which: 0 the policy, 1 the one-path-per-lane kernel, 2 the queued one; BVH
// scenes and samplesPerPixel > 1 take the one-path-per-lane kernel whatever it says
bool rt_render_list_queued(const rt_kparams& K, int which);
hipError_t rt_launch_render_list(const rt_kparams& K, const rt_list_args& L, int num_cus, int which, hipStream_t s);
hipError_t rt_launch_render_list_bvh(const rt_kparams& K, const rt_list_args& L, int block, size_t lds, int num_cus,
                                     hipStream_t s);

// ---- next-event estimation (rt_kernel_nee.h; exact units only) ------------------
// L null: a uniform render; non-null: the list of an adaptive call
hipError_t rt_launch_render_nee(const rt_kparams& K, const rt_nee_args& N, const rt_list_args* L, int num_cus, int grid_mult,
                                hipStream_t s);
hipError_t rt_launch_render_nee_bvh(const rt_kparams& K, const rt_nee_args& N, const rt_list_args* L, int block, size_t lds,
                                    int grid_mult, int num_cus, hipStream_t s);

// rt_light_pick_probabilities (rt_light_probs.hip): one point {P.xyz, n.xyz} on primitive prims[i] per lane,
// out count x N.n_lights; device pointers, count > 0, N.n_lights > 0
hipError_t rt_launch_pick_probabilities(const rt_nee_args& N, int n_sph, const float* points, const int* prims, int count,
                                        float* out, hipStream_t s);

// ---- the same in both modes (rt_kernels_shared.hip) -----------------------------
// launch policy: hit table in LDS, 64-lane groups (very deep paths), pair
// kernel (pair_req: 1 / 0 forces it on / off, BWRT_SPREAD; -1 the policy)
bool rt_hit_in_lds(const rt_kparams& K);
bool rt_small_block(const rt_kparams& K);
bool rt_takes_pair(const rt_kparams& K, bool hit_lds, int num_cus, int block_req, int pair_req);
// Whether rt_launch_render takes the sorted brute-force kernel for K (K.rec
// as the launch will have it): the only kernel that reads K.sky
bool rt_render_takes_sorted(const rt_kparams& K, int num_cus, bool simple, int block_req, int pair_req);
// The grid of a one-path-per-lane kernel (rt_render_kernel, the list and NEE
// kernels): `items` work items in groups of `block` lanes, or with grid_mult > 0
// (persistent lanes) at most grid_mult x resident groups per CU x CUs; at least 1
long rt_lane_grid(const void* kernel, int block, size_t lds, long items, int grid_mult, int num_cus);
// launch-order feedback around a launch of `grid` groups: the launch's
// parameters, and the sort behind it (K: what begin returned)
rt_kparams rt_order_begin(const rt_kparams& K0, long grid, const void* kernel, int block, size_t lds, int num_cus,
                          bool always);
hipError_t rt_order_end(const rt_kparams& K0, const rt_kparams& K, long grid, hipStream_t stream);
// the grid of the last launch that sorted its tile-group costs into group_order
// (0 = none; the context resets it before each launch and keeps the value)
extern thread_local long rt_order_groups_last;
// the render kernel the last launch on this thread took (rt_last_kernel_name)
extern thread_local char rt_launched_kernel[96];
size_t rt_render_rec_floats(const rt_kparams& K);
size_t rt_render_lds_bytes(const rt_kparams& K, int block, bool hit_lds, bool sorted);
size_t rt_lane_lds_bytes(const rt_kparams& K, int block, bool hit_lds, bool nee);
size_t rt_pair_lds_bytes(const rt_kparams& K);
hipError_t rt_launch_order_groups(const unsigned* cost, int* order, long n, hipStream_t stream);
hipError_t rt_launch_init_rand(unsigned* rng, int width, int rows, int row_offset, int row_stride,
                               hipStream_t stream);
hipError_t rt_launch_deinterleave(const unsigned* gathered, unsigned* image, int width, int height,
                                  int shards, int rows_per_shard, int max_blocks, hipStream_t stream);
// first-hit features: the brute-force loop; the BVH walk (rt_kernels_bvh.hip)
hipError_t rt_launch_aov(const rt_kparams& K, float4* ga, float4* gb, float4* alb, hipStream_t stream);
hipError_t rt_launch_aov_bvh(const rt_kparams& K, float4* ga, float4* gb, float4* alb, hipStream_t stream);
