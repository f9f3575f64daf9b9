// rt_launch_brute.h — launchers and launch policy of the brute-force render kernels (rt_kernels.hip and
// its reference-fast twin); the decisions that do not depend on the mode are rt_kernels_shared.hip's.
#pragma once
#include "rt_kernel_pair.h"
#include "rt_kernel_simple.h"
#include "rt_kernel_sorted.h"
#include "rt_launch.h"

RT_MODE_BEGIN
// the mode's BVH unit (rt_kernel_refill.h)
hipError_t rt_launch_render_bvh_simple(const rt_kparams& K, int block, size_t lds, int grid_mult, int num_cus,
                                       hipStream_t s);
hipError_t rt_launch_render_bvh_refill(const rt_kparams& K, int num_cus, hipStream_t s);

namespace {
// The queued kernels: the sorted task-queue kernel (full frames) and the pair
// kernel (small frames and shards: 128 lanes for 64 pixels).  Their grid
// covers every item once, so they take launch-order feedback (pair launches
// always: their grid is about one generation, and the order still helped
// there: c3 1/8 0.212 -> 0.206 ms, 1/16 0.187 -> 0.183,
// profiles/r04/spread/ab_pair.txt vs ab_prio.txt) in the ORDER instantiation;
// scenes without quads take the one with the quad tests compiled out.
template <bool PAIR, int BLOCK, bool HIT_LDS, bool GREC, bool ORDER, bool QUADS>
const void* queued_kernel() {
    if constexpr (PAIR)
        return reinterpret_cast<const void*>(&rt_render_pair_kernel<HIT_LDS, ORDER, QUADS>);
    else
        return reinterpret_cast<const void*>(&rt_render_sorted_kernel<BLOCK, HIT_LDS, GREC, ORDER, QUADS>);
}

template <bool PAIR, int BLOCK, bool HIT_LDS, bool GREC = false>
hipError_t launch_queued(const rt_kparams& K0, size_t lds, int num_cus, hipStream_t stream) {
    static_assert(!PAIR || (BLOCK == 128 && HIT_LDS && !GREC), "pair launches: 128 lanes, 64 pixels");
    constexpr int OWN = PAIR ? 64 : BLOCK;  // pixels per workgroup
    long grid = (launch_items(K0) + OWN - 1) / OWN;
    if (grid < 1) grid = 1;
    rt_kparams K =
        rt_order_begin(K0, grid, queued_kernel<PAIR, BLOCK, HIT_LDS, GREC, false, true>(), BLOCK, lds, num_cus, PAIR);
    K.rec_stride = (int)(grid * OWN);
    const bool feedback = K.group_cost != nullptr, quads = K.n_quad > 0;
    const void* kernel = feedback ? (quads ? queued_kernel<PAIR, BLOCK, HIT_LDS, GREC, true, true>()
                                           : queued_kernel<PAIR, BLOCK, HIT_LDS, GREC, true, false>())
                                  : (quads ? queued_kernel<PAIR, BLOCK, HIT_LDS, GREC, false, true>()
                                           : queued_kernel<PAIR, BLOCK, HIT_LDS, GREC, false, false>());
    void* args[] = {&K};
    (void)hipLaunchKernel(kernel, dim3((unsigned)grid), dim3(BLOCK), args, lds, stream);
    std::snprintf(rt_launched_kernel, sizeof rt_launched_kernel, "%s<%d%s%s%s>%s%s",
                  PAIR ? "rt_render_pair_kernel" : "rt_render_sorted_kernel", BLOCK, HIT_LDS ? "" : ",hit_global",
                  GREC ? ",grec" : "", RT_MODE_TAG, feedback ? "+order" : "", !PAIR && K.sky ? "+sky" : "");
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : rt_order_end(K0, K, grid, stream);
}

// the sorted kernel of a block size: record stack in global memory when the
// launch has one (K.rec)
template <int BLOCK>
hipError_t launch_sorted(const rt_kparams& K, bool hit_lds, size_t lds, int num_cus, hipStream_t s) {
    if (K.rec)
        return hit_lds ? launch_queued<false, BLOCK, true, true>(K, lds, num_cus, s)
                       : launch_queued<false, BLOCK, false, true>(K, lds, num_cus, s);
    return hit_lds ? launch_queued<false, BLOCK, true>(K, lds, num_cus, s)
                   : launch_queued<false, BLOCK, false>(K, lds, num_cus, s);
}

// the simple kernel of a block size; BVH scenes: the BVH unit's instantiation
// (hit table in global memory, wave-synchronous walk)
template <int BLOCK>
hipError_t launch_simple_block(const rt_kparams& K, bool hit_lds, size_t lds, int grid_mult, int num_cus, hipStream_t s) {
    if (K.bvh_nodes) return rt_launch_render_bvh_simple(K, BLOCK, lds, grid_mult, num_cus, s);
    return hit_lds ? launch_simple<BLOCK, true, false>(K, lds, grid_mult, num_cus, s)
                   : launch_simple<BLOCK, false, false>(K, lds, grid_mult, num_cus, s);
}
}  // namespace

// Launch policy for the sorted kernel's record stack: global memory when the
// LDS stack (3 dwords per level per lane) would hold the brute-force kernel
// below RT_WAVES_PER_EU waves per SIMD, i.e. deep paths.  Measured: config
// 4 (maxBounces 6) 4 -> 7 waves/SIMD, 7.61 -> 6.34 ms.
// Also when global records let more 256-lane groups reside per CU (runtime
// occupancy of both instantiations) and the frame runs at least
// RT_GREC_MIN_GEN generations of them: config 3 (maxBounces 4) 6 -> 7
// waves/SIMD, 0.816 -> 0.801 ms (three alternating runs); re-measured in
// round 5 on its row shards (`profiles/r05b/ab_grec_shards.txt`): 1/2 (2.26
// generations) 0.460 -> 0.453 ms, 1/3 (1.51) 0.335 -> 0.322, but 1/4 (1.13)
// 0.270 -> 0.277; config 2 gains no group.  A third shape, one LDS level at
// 8 waves per SIMD (64 VGPRs, 8-byte spill), makes the 1/4 shard one resident
// generation (0.99) instead of 1.32, and loses there: 0.298 vs 0.270 ms with
// LDS records, 1/2 0.455 vs 0.42, full frame flat (round 6, two alternating
// runs, profiles/r06a/ab_grec.txt; the code: profiles/r06a/grec8_shape.diff)
#ifndef RT_GREC_MIN_GEN
#define RT_GREC_MIN_GEN 1.4
#endif
bool rt_render_wants_global_records(const rt_kparams& K, int num_cus) {
    if (K.bvh_nodes || K.max_bounces <= 0) return false;
    const bool hit_lds = rt_hit_in_lds(K);
    rt_kparams L = K;
    L.rec = nullptr;
    const size_t lds = rt_render_lds_bytes(L, 256, hit_lds, true);
    const long groups = (long)(160 * 1024) / (long)(lds ? lds : 1);  // 256-lane groups per CU: 1 wave per SIMD each
    if (groups < RT_WAVES_PER_EU) return true;
    // resident 256-lane groups per CU with LDS / global records
    L.rec = reinterpret_cast<float*>(&L);  // any non-null: the global-record LDS size
    const size_t lds_g = rt_render_lds_bytes(L, 256, hit_lds, true);
    int occ_l = 0, occ_g = 0;
    const void* kl = hit_lds ? queued_kernel<false, 256, true, false, false, true>()
                             : queued_kernel<false, 256, false, false, false, true>();
    const void* kg = hit_lds ? queued_kernel<false, 256, true, true, false, true>()
                             : queued_kernel<false, 256, false, true, false, true>();
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_l, kl, 256, lds) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_g, kg, 256, lds_g) != hipSuccess || occ_g <= occ_l)
        return false;
    const double gens = (double)((long)K.rows * K.width) / (256.0 * occ_g * (num_cus > 0 ? num_cus : 1));
    return gens >= RT_GREC_MIN_GEN;
}

// Host-side launch policy: BVH scenes take the ray-refill kernel; otherwise
// 256-lane workgroups (64 when the record stack of very deep paths would not
// fit), hit table in LDS when it fits in 16 KB, sorted task-queue kernel
// unless `simple` (one pixel per lane: its grid always covers every item);
// for the simple kernel grid_mult > 0 caps the grid at grid_mult x resident
// workgroups per CU (persistent lanes).  Small frames and shards take the
// pair kernel (rt_takes_pair, rt_kernels_shared.hip).
#ifndef RT_SORTED_BLOCK
#define RT_SORTED_BLOCK 256
#endif
hipError_t rt_launch_render(const rt_kparams& K, int num_cus, int grid_mult, bool simple, int block_req,
                            hipStream_t stream, int pair_req) {
    // samplesPerPixel > 1 (the reference's in-frame loop, off by default):
    // only the one-path-per-lane kernel implements it
    simple = simple || K.spp_inner > 1;
    if (K.bvh_nodes && !simple) return rt_launch_render_bvh_refill(K, num_cus, stream);
    const bool hit_lds = rt_hit_in_lds(K);
    const bool small_block = rt_small_block(K);
    const size_t lds = rt_render_lds_bytes(K, small_block ? 64 : 256, hit_lds, !simple);
    if (simple)
        return small_block ? launch_simple_block<64>(K, hit_lds, lds, grid_mult, num_cus, stream)
                           : launch_simple_block<256>(K, hit_lds, lds, grid_mult, num_cus, stream);
    if (small_block) return launch_sorted<64>(K, hit_lds, lds, num_cus, stream);
    const long items = (long)K.rows * K.width;
    if (rt_takes_pair(K, hit_lds, num_cus, block_req, pair_req))
        return launch_queued<true, 128, true>(K, rt_pair_lds_bytes(K), num_cus, stream);
    if (block_req == 64 || block_req == 128 || block_req == 256) {  // explicit (BWRT_BLOCK)
        const size_t lds_r = rt_render_lds_bytes(K, block_req, hit_lds, true);
        if (lds_r <= 65536) {
            if (block_req == 64) return launch_sorted<64>(K, hit_lds, lds_r, num_cus, stream);
            if (block_req == 128) return launch_sorted<128>(K, hit_lds, lds_r, num_cus, stream);
            return launch_sorted<256>(K, hit_lds, lds_r, num_cus, stream);
        }
    }
    const size_t lds_s = rt_render_lds_bytes(K, RT_SORTED_BLOCK, hit_lds, true);
    // deep paths (large max_bounces) make the LDS record stack big: take
    // 128-lane groups when they keep more waves resident per CU (LDS 160 KB,
    // VGPR-bound at 4 x RT_WAVES_PER_EU waves)
    auto waves_per_cu = [](size_t lds_bytes, int block) {
        const long by_lds = (long)(160 * 1024 / (lds_bytes ? lds_bytes : 1)) * (block / 64);
        return by_lds < 4L * RT_WAVES_PER_EU ? by_lds : 4L * RT_WAVES_PER_EU;
    };
    // small frames / shards (one rank of an 8-GPU frame): fewer than 4
    // full-size groups per CU leave CUs with unequal shares of the critical
    // path (every group is resident at once); 128-lane groups spread it
    // (measured on c3 row shards of 1/8: 0.249 vs 0.264 ms; 1/4: 0.312 vs
    // 0.291), and the pair kernel (above) spreads it further
    const bool few_groups = items < (long)num_cus * 4 * RT_SORTED_BLOCK;
    if (RT_SORTED_BLOCK > 128 &&
        (few_groups ||
         waves_per_cu(rt_render_lds_bytes(K, 128, hit_lds, true), 128) > waves_per_cu(lds_s, RT_SORTED_BLOCK))) {
        const size_t lds_128 = rt_render_lds_bytes(K, 128, hit_lds, true);
        return launch_sorted<128>(K, hit_lds, lds_128, num_cus, stream);
    }
    return launch_sorted<RT_SORTED_BLOCK>(K, hit_lds, lds_s, num_cus, stream);
}
RT_MODE_END
