// rt_pixel.h — what every render kernel (rt_kernel_*.h) shares on the device: the unit's
// precision mode, the per-lane pixel state, the launch order (work item -> pixel),
// hit-table staging, frame accumulation, the launch-order feedback prologue.
//
// Design of the render kernels:
//  * one ray per lane (wave64), one pixel per lane;
//  * ALL `samples` progressive frames of a pixel run in ONE launch: the RNG
//    state (6 x u32) and the frameSum accumulator stay in VGPRs across
//    frames, so HBM sees 24+12 B read and 24+12+4 B written per pixel per
//    launch instead of per frame;
//  * the recursion's per-depth (emitted, brdf, cos) records live in an LDS
//    stack (conflict-free: bank = lane) and are folded innermost-first when
//    the path ends:
//        L = e_k + (b_k * L) * c_k   (Main.cu:268 evaluated by recursion)
//    which reproduces the recursive evaluation order bit for bit;
//  * the primitive loop index is wave-uniform, so primitive data come
//    through scalar loads (SGPR operands of the VALU tests), not VGPRs;
//  * every float op is one IEEE rounding in reference order (built with
//    -ffp-contract=off; correctly rounded div/sqrt); no MFMA (branchy
//    per-ray math, not a contraction).  The opt-in reference-fast units
//    ("Precision modes" below) trade that for the reference's own fast-math.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_diag.h"
#include "rt_layout.h"
#include "rt_path.h"

// Precision modes.  The render kernels are compiled four times: the exact
// brute-force and BVH translation units (rt_kernels.hip, rt_kernels_bvh.hip)
// and their reference-fast twins (rt_kernels_fast.hip,
// rt_kernels_bvh_fast.hip: RT_FAST, built with -ffp-contract=fast; rt_path.h
// has the arithmetic).  The render kernels are templates: the same
// instantiation from an exact and a fast unit would be one weak symbol with
// two bodies, and the linker would keep either.  So the fast units put
// every render kernel and its launchers into namespace rt_fast; the exact
// units keep them at global scope, their symbols and code unchanged.
// What does not depend on the mode is in rt_kernels_shared.hip, compiled once.
#ifdef RT_FAST
#define RT_MODE_BEGIN namespace rt_fast {
#define RT_MODE_END }
#define RT_MODE_TAG ",fast"
#else
#define RT_MODE_BEGIN
#define RT_MODE_END
#define RT_MODE_TAG ""
#endif

// occupancy target of the simple and the sorted kernel (the Makefile sets it per unit)
#ifndef RT_WAVES_PER_EU
#define RT_WAVES_PER_EU 1
#endif

enum { T_NONE = 0, T_REGEN = 1, T_DIFF = 2, T_SPEC = 3 };  // a lane's next task (sorted and pair kernels)

namespace {
// Per-lane pixel state ------------------------------------------------------
// RT_NT_PIXEL (default 3): the pixel-state streams (RNG, frameSum, RGBA8;
// each touched once per launch) as non-temporal loads (bit 0) and stores
// (bit 1).  Steady-state A/B (profiles/r06q, r06s): c3 -0.28 %, c4 -0.27 %,
// c5 -0.23 % kernel time, shards flat; HBM bytes +10 % (not the bound)
#ifndef RT_NT_PIXEL
#define RT_NT_PIXEL 3
#endif
template <typename T>
__device__ __forceinline__ T px_ld(const T* a) {
    if (RT_NT_PIXEL & 1) return __builtin_nontemporal_load(a);
    return *a;
}
template <typename T>
__device__ __forceinline__ void px_st(T* a, T v) {
    if (RT_NT_PIXEL & 2) __builtin_nontemporal_store(v, a);
    else *a = v;
}
struct PixelState {
    long w;         // work item (lane slot in the tiled launch order)
    long p;         // shard pixel index
    bool valid;
    Xorwow rs;
    float ax, ay, az;  // frameSum
    f3 d0;          // normalize(rot * pixelPosition): the same every frame
    int passes_left;
    unsigned frame;
};

__device__ __forceinline__ void load_pixel(const rt_kparams& K, long npix, long p, PixelState& s) {
    s.p = p;
    s.valid = p < npix;
    s.passes_left = 0;
    s.frame = K.first_frame;
    if (!s.valid) return;
    const int j = (int)(p / K.width);
    const int x = (int)(p - (long)j * K.width);
    const int y = K.row_offset + j * K.row_stride;
    s.rs.d = px_ld(&K.rng[0 * npix + p]);
    s.rs.v0 = px_ld(&K.rng[1 * npix + p]);
    s.rs.v1 = px_ld(&K.rng[2 * npix + p]);
    s.rs.v2 = px_ld(&K.rng[3 * npix + p]);
    s.rs.v3 = px_ld(&K.rng[4 * npix + p]);
    s.rs.v4 = px_ld(&K.rng[5 * npix + p]);
    s.ax = s.ay = s.az = 0.0f;
    if (K.first_frame != 1u) {
        s.ax = px_ld(&K.accum[0 * npix + p]);
        s.ay = px_ld(&K.accum[1 * npix + p]);
        s.az = px_ld(&K.accum[2 * npix + p]);
    }
    s.d0 = primary_dir(K, x, y);  // Main.cu:287-290
    s.passes_left = K.samples;
}

// Launch order: work item w -> pixel.  Items come in groups of 64 (one
// wave) covering a tile_w x (64/tile_w) pixel tile, tiles row-major over the
// shard; tile_w = 0 keeps the linear order (item = pixel).  Square-ish tiles
// keep a wave's rays spatially coherent (a pixel-scrambled order costs +45 %).
// tile_sq: every 4 consecutive waves form a 2 x 2 block of tiles (a 4-wave
// group then covers a square-ish patch), the tile grid padded to even sizes
__host__ __device__ inline long launch_items(const rt_kparams& K) {
    if (K.tile_w <= 0) return (long)K.rows * K.width;
    const int tw = K.tile_w, th = 64 / K.tile_w;
    long tiles_x = (K.width + tw - 1) / tw, tiles_y = (K.rows + th - 1) / th;
    if (K.tile_sq) {
        tiles_x += tiles_x & 1;
        tiles_y += tiles_y & 1;
    }
    return tiles_x * tiles_y * 64;
}

__device__ __forceinline__ long items_of(const rt_kparams& K, long npix) {
    return K.tile_w <= 0 ? npix : launch_items(K);
}

__device__ __forceinline__ long item_to_pixel(const rt_kparams& K, long npix, long w) {
    if (K.tile_w <= 0) return w < npix ? w : npix;
    const int tw = K.tile_w, th = 64 / K.tile_w;
    const long tiles_x = (K.width + tw - 1) / tw;
    const long wave = w >> 6;
    const int l = (int)(w & 63);
    long tx, ty;
    if (K.tile_sq) {
        const long sx = (tiles_x + 1) >> 1, sw = wave >> 2;
        tx = (sw % sx) * 2 + (wave & 1);
        ty = (sw / sx) * 2 + ((wave >> 1) & 1);
    } else {
        tx = wave % tiles_x;
        ty = wave / tiles_x;
    }
    const long x = tx * tw + (l % tw);
    const long j = ty * th + (l / tw);
    if (x >= K.width || j >= K.rows) return npix;
    return j * K.width + x;
}

__device__ __forceinline__ void load_item(const rt_kparams& K, long npix, long nitems, long w, PixelState& s) {
    load_pixel(K, npix, w < nitems ? item_to_pixel(K, npix, w) : npix, s);
    s.w = w;
}

__device__ __forceinline__ void store_pixel(const rt_kparams& K, long npix, const PixelState& s) {
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
    if (K.rgba) px_st(&K.rgba[p], tone_map(s.ax, s.ay, s.az, s.frame - 1u));
}

// progressive accumulation of one finished frame (Main.cu:299-304)
__device__ __forceinline__ void accumulate_frame(PixelState& px, float lx, float ly, float lz) {
    if (px.frame == 1u) {
        px.ax = 0.0f;
        px.ay = 0.0f;
        px.az = 0.0f;
    }
    px.ax = px.ax + lx;
    px.ay = px.ay + ly;
    px.az = px.az + lz;
    px.frame++;
    px.passes_left--;
}

typedef __attribute__((address_space(3))) float lds_float;

// A lane's RNG state to / from six consecutive dword fields F(f0 ..) of an LDS
// slot; F is the kernel's field macro, the arguments after f0 its slot index
#define RS_PUT(rs, F, f0, ...)                                   \
    do {                                                         \
        F((f0) + 0, ##__VA_ARGS__) = __uint_as_float((rs).d);    \
        F((f0) + 1, ##__VA_ARGS__) = __uint_as_float((rs).v0);   \
        F((f0) + 2, ##__VA_ARGS__) = __uint_as_float((rs).v1);   \
        F((f0) + 3, ##__VA_ARGS__) = __uint_as_float((rs).v2);   \
        F((f0) + 4, ##__VA_ARGS__) = __uint_as_float((rs).v3);   \
        F((f0) + 5, ##__VA_ARGS__) = __uint_as_float((rs).v4);   \
    } while (0)
#define RS_GET(rs, F, f0, ...)                                   \
    do {                                                         \
        (rs).d = __float_as_uint(F((f0) + 0, ##__VA_ARGS__));    \
        (rs).v0 = __float_as_uint(F((f0) + 1, ##__VA_ARGS__));   \
        (rs).v1 = __float_as_uint(F((f0) + 2, ##__VA_ARGS__));   \
        (rs).v2 = __float_as_uint(F((f0) + 3, ##__VA_ARGS__));   \
        (rs).v3 = __float_as_uint(F((f0) + 4, ##__VA_ARGS__));   \
        (rs).v4 = __float_as_uint(F((f0) + 5, ##__VA_ARGS__));   \
    } while (0)

// The hit table (n_prim x RT_HIT_FLOATS) staged at the start of the group's
// LDS by its BLOCK lanes; returns the first float behind it (16-byte aligned).
// The caller's next barrier publishes it.
template <int BLOCK>
__device__ __forceinline__ float* stage_hit_table(const rt_kparams& K, float* smem, int tid) {
    const int n_prim = K.n_sph + K.n_pln + K.n_tri + K.n_quad;
    for (int i = tid; i < n_prim * RT_HIT_FLOATS; i += BLOCK) smem[i] = K.hit[i];
    return smem + ((n_prim * RT_HIT_FLOATS + 3) & ~3);
}

// Launch-order feedback (rt_layout.h): workgroup g renders tile-group
// group_order[g] (ORDER instantiations with an order; blockIdx order
// otherwise) and leaves the group's duration in group_cost[].  (The pair
// kernel keeps its own copy of this and of the staging: through the helpers
// its instruction stream differs, profiles/kernel_split/dropped.txt)
template <bool ORDER>
__device__ __forceinline__ long order_group(const rt_kparams& K) {
    return ORDER && K.group_order ? (long)K.group_order[blockIdx.x] : (long)blockIdx.x;
}
// (the start time is parked in group_cost[] itself: nothing stays live
// across the kernel's loop)
template <bool ORDER>
__device__ __forceinline__ long order_group_start(const rt_kparams& K, int tid) {
    const long group = order_group<ORDER>(K);
    if (ORDER && tid == 0) K.group_cost[group] = (unsigned)__builtin_amdgcn_s_memrealtime();
    return group;
}
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                          __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// RT_KEY of a primitive id (spheres, planes, triangles, quads in turn); -1 for -1
__device__ __forceinline__ int prim_key(const rt_kparams& K, int id) {
    const int e_pln = K.n_sph, e_tri = e_pln + K.n_pln, e_quad = e_tri + K.n_tri;
    return id < 0 ? -1
                  : id < e_pln ? RT_KEY(0, id)
                               : id < e_tri ? RT_KEY(1, id - e_pln)
                                            : id < e_quad ? RT_KEY(2, id - e_tri) : RT_KEY(3, id - e_quad);
}

}  // namespace
