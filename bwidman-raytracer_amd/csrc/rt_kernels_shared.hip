// rt_kernels_shared.hip — what the render units share whatever their precision mode, compiled once
// with the exact flags: the float-free kernels, the brute-force feature kernel, LDS sizes, and the
// launch policy's decisions that touch no render kernel (rt_launch.h).
#include <type_traits>

#include "rt_kernel_pair.h"    // RT_PAIR_FIELDS
#include "rt_kernel_sorted.h"  // RT_GREC_LDS_LEVELS
#include "rt_launch.h"

// Launch-order feedback: one workgroup turns the last launch's tile-group
// durations into the next launch's order, most expensive first (longest
// processing time first: the frame's last workgroups are then the cheap
// ones, so the chip drains quickly).  Counting sort over 512 logarithmic cost
// buckets (exponent and top 4 mantissa bits of float(cost): 1/16-octave
// steps, no max pass); the order within a bucket is whatever the LDS
// atomics give, which is harmless: every pixel's result is independent of
// when its group runs.
__device__ __forceinline__ int order_bucket(unsigned cost) {
    const int k = (int)(__float_as_uint((float)cost + 1.0f) >> 19) - (127 << 4);  // 0 .. 512
    return 511 - min(k, 511);
}

__global__ void __launch_bounds__(1024) rt_order_groups_kernel(const unsigned* __restrict__ cost,
                                                               int* __restrict__ order, int n) {
    __shared__ unsigned hist[512];
    __shared__ unsigned wsum[8];
    const int tid = threadIdx.x;
    if (tid < 512) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) atomicAdd(&hist[order_bucket(cost[i])], 1u);
    __syncthreads();
    // exclusive scan of the 512 buckets: waves 0..7, one bucket per lane
    unsigned v = 0, incl = 0;
    if (tid < 512) {
        v = hist[tid];
        incl = v;
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned u = __shfl_up(incl, m);
            if ((tid & 63) >= m) incl += u;
        }
        if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    }
    __syncthreads();
    if (tid < 512) {
        unsigned base = 0;
        for (int w = 0; w < (tid >> 6); w++) base += wsum[w];
        hist[tid] = base + incl - v;
    }
    __syncthreads();
    for (int i = tid; i < n; i += 1024) order[atomicAdd(&hist[order_bucket(cost[i])], 1u)] = i;
}

// initializeRand (Main.cu:369-380): curand_init(y*W + x, 0, 0)
__global__ void __launch_bounds__(256) rt_init_rand_kernel(unsigned* rng, int width, int rows,
                                                           int row_offset, int row_stride) {
    const long npix = (long)rows * width;
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const int j = (int)(p / width);
    const int x = (int)(p - (long)j * width);
    const int y = row_offset + j * row_stride;
    const Xorwow s = xorwow_seed(pixel_seed(x, y, width));
    rng[0 * npix + p] = s.d;
    rng[1 * npix + p] = s.v0;
    rng[2 * npix + p] = s.v1;
    rng[3 * npix + p] = s.v2;
    rng[4 * npix + p] = s.v3;
    rng[5 * npix + p] = s.v4;
}

// Multi-GPU gather epilogue: block r of `gathered` holds rows r, r+G, ...
// VEC = 4: 16 bytes (4 pixels) per lane (width % 4 == 0, 16-byte aligned
// buffers); a grid-stride loop, so the launch may cap its grid and leave the
// CUs to a render running beside it
template <int VEC>
__global__ void __launch_bounds__(256) rt_deinterleave_kernel(const unsigned* __restrict__ gathered,
                                                              unsigned* __restrict__ image, int width,
                                                              int height, int shards, int rows_per_shard) {
    typedef typename std::conditional<VEC == 4, uint4, unsigned>::type word;
    const int wv = width / VEC;
    const long n = (long)height * wv;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long)gridDim.x * blockDim.x) {
        const int y = (int)(q / wv);
        const int x = (int)(q - (long)y * wv);
        const int r = y % shards;
        const int j = y / shards;
        reinterpret_cast<word*>(image)[q] = reinterpret_cast<const word*>(gathered)[((long)r * rows_per_shard + j) * wv + x];
    }
}

// ---- launch policy ------------------------------------------------------------
bool rt_hit_in_lds(const rt_kparams& K) {
#ifdef RT_NO_HIT_LDS  // A/B builds: hit table read from global memory
    return false;
#endif
    const int n_prim = K.n_sph + K.n_pln + K.n_tri + K.n_quad;
    return !K.bvh_nodes && (size_t)n_prim * RT_HIT_FLOATS * sizeof(float) <= 16384;
}
bool rt_small_block(const rt_kparams& K) {
    return (size_t)RT_LANE_REC_DWORDS(false) * (K.max_bounces + 1) * 256 * sizeof(float) > 49152;
}

// Frames and shards of at most RT_SPREAD_PIX pixels per CU (about 1.5
// generations of 7 waves per SIMD, 32 pixels per wave) take 128-lane pair
// groups owning 64 pixels each.  Measured on c3 row shards: 1/8 0.252 ->
// 0.194 ms, 1/16 0.254 -> 0.167 (profiles/r04g/shards_c3.txt); 1/4 (2,025
// pixels per CU) keeps the sorted kernel
#ifndef RT_SPREAD_PIX
#define RT_SPREAD_PIX 1400
#endif
// (the pair kernel shortens long per-pixel chains: frames of at most
// RT_PAIR_MIN_CHAIN queries per pixel keep the sorted kernel — config 1,
// 1 frame x 2 queries: 10.3 vs 10.9 us, profiles/r05c/session.txt)
#ifndef RT_PAIR_MIN_CHAIN
#define RT_PAIR_MIN_CHAIN 8
#endif
bool rt_takes_pair(const rt_kparams& K, bool hit_lds, int num_cus, int block_req, int pair_req) {
    const long items = (long)K.rows * K.width;
    return hit_lds && !K.rec && (block_req == 0 || block_req == 128) &&
           (pair_req > 0 || (pair_req < 0 && block_req == 0 && items <= (long)num_cus * RT_SPREAD_PIX &&
                             (long)K.samples * (K.max_bounces + 1) >= RT_PAIR_MIN_CHAIN));
}

bool rt_render_takes_sorted(const rt_kparams& K, int num_cus, bool simple, int block_req, int pair_req) {
    if (simple || K.spp_inner > 1 || K.bvh_nodes) return false;
    return rt_small_block(K) || !rt_takes_pair(K, rt_hit_in_lds(K), num_cus, block_req, pair_req);
}

long rt_lane_grid(const void* kernel, int block, size_t lds, long items, int grid_mult, int num_cus) {
    long grid = (items + block - 1) / block;
    if (grid_mult > 0) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds) == hipSuccess && per_cu > 0) {
            const long cap = (long)per_cu * num_cus * grid_mult;
            if (grid > cap) grid = cap;
        }
    }
    return grid < 1 ? 1 : grid;
}

// launch-order feedback applies to grids of more than RT_ORDER_MIN_GEN
// generations of resident groups: 1.5 -> 1.1 turns it on for the c3 1/4
// shard (1.32 generations: 0.297 -> 0.285 ms, two rounds, tools/shard_sweep.py;
// c2 / c3 / c4 at the other shard sizes unchanged within noise)
#ifndef RT_ORDER_MIN_GEN
#define RT_ORDER_MIN_GEN 1.1
#endif
rt_kparams rt_order_begin(const rt_kparams& K0, long grid, const void* kernel, int block, size_t lds, int num_cus,
                          bool always) {
    rt_kparams K = K0;
    // only where the grid covers every item once (group g <-> tile-group g) and the buffers hold the
    // grid, and only where the grid runs in more than RT_ORDER_MIN_GEN generations of resident groups:
    // LPT order shortens the drain at the end of a multi-generation grid, while a grid that is resident
    // all at once only gets its expensive groups packed onto the same CUs (c3 at 1/8: 0.264 vs 0.243 ms
    // with the order; 1/2: 0.493 vs 0.522)
    bool feedback = K.group_cost && K.group_order && grid <= K.order_cap;
    if (feedback && !always) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds) != hipSuccess || per_cu <= 0)
            per_cu = 1;
        feedback = (double)grid > RT_ORDER_MIN_GEN * (double)per_cu * num_cus;
    }
    if (!feedback) {
        K.group_cost = nullptr;
        K.group_order = nullptr;
    } else if (K.order_n != grid) {
        K.group_order = nullptr;  // no order for this grid yet: blockIdx order
    }
    return K;
}

hipError_t rt_order_end(const rt_kparams& K0, const rt_kparams& K, long grid, hipStream_t stream) {
    // the sort runs when asked, and always for a grid without an order yet
    if (!K.group_cost || !(K0.order_sort || K0.order_n != grid)) return hipSuccess;
    const hipError_t e = rt_launch_order_groups(K0.group_cost, K0.group_order, grid, stream);
    if (e == hipSuccess) rt_order_groups_last = grid;
    return e;
}

// ---- sizes ----------------------------------------------------------------------
// LDS bytes of one pair-kernel group (hit table in LDS)
size_t rt_pair_lds_bytes(const rt_kparams& K) {
    const int n_prim = K.n_sph + K.n_pln + K.n_tri + K.n_quad;
    return (size_t)((n_prim * RT_HIT_FLOATS + 3) & ~3) * sizeof(float) +
           (size_t)(3 * (K.max_bounces > 0 ? K.max_bounces : 0) + RT_PAIR_FIELDS) * 64 * sizeof(float) + 4 * sizeof(int);
}

// Floats of a global-memory record stack for one launch: 3 dwords per level kept in global memory
// (levels RT_GREC_LDS_LEVELS .. max_bounces-1; the shallow ones stay in LDS) per lane of the grid (the
// grid covers every work item, rounded up to the largest workgroup), [group][level][field][lane].  At
// least one float, so a forced global-record launch with no global level still gets a buffer.
size_t rt_render_rec_floats(const rt_kparams& K) {
    const long nitems = launch_items(K);
    const int lds_levels = K.max_bounces < RT_GREC_LDS_LEVELS ? K.max_bounces : RT_GREC_LDS_LEVELS;
    const size_t planes = (size_t)3 * (K.max_bounces - lds_levels);
    return planes ? planes * (size_t)((nitems + 255) / 256 * 256) : 1;
}

// LDS bytes of one workgroup of a one-path-per-lane kernel (rt_render_kernel,
// rt_kernel_lane.h; nee: next-event estimation): hit table (if staged) + the
// record stack of max_bounces + 1 levels
size_t rt_lane_lds_bytes(const rt_kparams& K, int block, bool hit_lds, bool nee) {
    const int n_prim = K.n_sph + K.n_pln + K.n_tri + K.n_quad;
    const size_t hit = hit_lds ? (size_t)((n_prim * RT_HIT_FLOATS + 3) & ~3) * sizeof(float) : 0;
    const int levels = K.max_bounces + 1;
    return hit + (size_t)RT_LANE_REC_DWORDS(nee) * (levels > 0 ? levels : 0) * block * sizeof(float);
}

// LDS bytes of one workgroup.  Sorted: hit table (if staged) + 3 record dwords
// per level per lane (max_bounces levels) + 13 task-slot dwords per lane and 4
// queue counters; else rt_lane_lds_bytes.
size_t rt_render_lds_bytes(const rt_kparams& K, int block, bool hit_lds, bool sorted) {
    if (!sorted) return rt_lane_lds_bytes(K, block, hit_lds, false);
    const int n_prim = K.n_sph + K.n_pln + K.n_tri + K.n_quad;
    const size_t hit = hit_lds ? (size_t)((n_prim * RT_HIT_FLOATS + 3) & ~3) * sizeof(float) : 0;
    const int lds_levels = K.rec ? (K.max_bounces < RT_GREC_LDS_LEVELS ? K.max_bounces : RT_GREC_LDS_LEVELS) : K.max_bounces;
    return hit + (size_t)3 * (lds_levels > 0 ? lds_levels : 0) * block * sizeof(float) +
           (size_t)13 * block * sizeof(float) + 8 * sizeof(int);  // + queue counters
}

thread_local long rt_order_groups_last = 0;
thread_local char rt_launched_kernel[96] = "";

hipError_t rt_launch_order_groups(const unsigned* cost, int* order, long n, hipStream_t stream) {
    hipLaunchKernelGGL(rt_order_groups_kernel, dim3(1), dim3(1024), 0, stream, cost, order, (int)n);
    return hipGetLastError();
}

hipError_t rt_launch_init_rand(unsigned* rng, int width, int rows, int row_offset, int row_stride,
                               hipStream_t stream) {
    const long npix = (long)rows * width;
    const unsigned grid = (unsigned)((npix + 255) / 256);
    hipLaunchKernelGGL(rt_init_rand_kernel, dim3(grid), dim3(256), 0, stream, rng, width, rows,
                       row_offset, row_stride);
    return hipGetLastError();
}

// max_blocks > 0 caps the grid (the loop strides over the rest)
hipError_t rt_launch_deinterleave(const unsigned* gathered, unsigned* image, int width, int height,
                                  int shards, int rows_per_shard, int max_blocks, hipStream_t stream) {
    const bool vec = width % 4 == 0 && ((reinterpret_cast<uintptr_t>(gathered) | reinterpret_cast<uintptr_t>(image)) & 15) == 0;
    const long n = (long)height * (vec ? width / 4 : width);
    long grid = (n + 255) / 256;
    if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
    if (vec)
        hipLaunchKernelGGL(rt_deinterleave_kernel<4>, dim3((unsigned)grid), dim3(256), 0, stream, gathered, image,
                           width, height, shards, rows_per_shard);
    else
        hipLaunchKernelGGL(rt_deinterleave_kernel<1>, dim3((unsigned)grid), dim3(256), 0, stream, gathered, image,
                           width, height, shards, rows_per_shard);
    return hipGetLastError();
}

hipError_t rt_launch_aov(const rt_kparams& K, float4* ga, float4* gb, float4* alb, hipStream_t stream) {
    return launch_aov<false>(K, ga, gb, alb, stream);
}
