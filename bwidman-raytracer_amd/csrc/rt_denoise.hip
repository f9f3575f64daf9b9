// rt_denoise.hip — the a-trous filter kernels (gfx950), one launch per level.
//
// rt_denoise.h has the arithmetic (shared with the CPU backend); this unit is
// built once with the exact flags (-ffp-contract=off, no RT_FAST), whatever
// precision mode the context renders in.
//
// Level 0 reads frameSum (three planes) and applies 1/n, the last level also
// stores the tone-mapped RGBA8: there are no conversion passes.  The colour
// ping-pongs between two float4 buffers; a tap reads {colour, guide a, guide
// b} = 3 x 16 bytes.
//
// direct: one lane per pixel, 32 x 8 pixel workgroups, the 25 taps straight
//   from global memory (L1 / L2 serve the overlap between neighbours).
// tiled:  one workgroup stages the taps of 64 contiguous pixels in x by 8
//   LATTICE rows in LDS.  Rows with the same y mod s form an independent
//   step-1 problem in y, so a tile of rows y0 + r s (r = -2 .. 9) needs only
//   2 halo rows each side at any step, and its x range (64 + 4 s pixels) stays
//   contiguous, so the staging loads are coalesced.  (64 + 4 s) x 12 texels of
//   48 bytes: 38 KiB at s = 1, 108 KiB at s = 32.  Loads per output pixel:
//   1.6 (s = 1) to 4.5 (s = 32) instead of 25.  Colour, guide a and guide b
//   are three separate float4 planes in LDS: a wave's ds_read_b128 then reads
//   64 consecutive 16-byte words (no bank conflict beyond the 4-pass minimum).
#include <hip/hip_runtime.h>

#include "rt_denoise.h"

namespace {

constexpr int kDirectW = 32, kDirectH = 8;
constexpr int kTileW = 64, kTileH = 8;

template <bool FIRST>
__global__ void __launch_bounds__(256) rt_denoise_direct_kernel(const rt_dn_level L, const int tiles_x) {
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int x = tx * kDirectW + (int)(threadIdx.x & (kDirectW - 1));
    const int y = ty * kDirectH + (int)(threadIdx.x / kDirectW);
    if (x >= L.width || y >= L.height) return;
    const DnGlobalFetch<FIRST> fetch{L};
    dn_store(L, (long)y * L.width + x, dn_pixel(L, x, y, fetch));
}

// taps from the workgroup's LDS tile: texel (qx - x_lo, r + dy + 2)
struct DnLdsFetch {
    const float4* col;
    const float4* ga;
    const float4* gb;
    int pitch, x_lo, row;  // row = the lane's lattice row in the tile (0 .. kTileH - 1)
    __device__ __forceinline__ void operator()(int, int dy, int qx, int, f3& c, float4& a, float4& b) const {
        const int i = (row + dy + 2) * pitch + (qx - x_lo);
        a = ga[i];
        b = gb[i];
        const float4 cc = col[i];
        c = mk(cc.x, cc.y, cc.z);
    }
};

template <bool FIRST>
__global__ void __launch_bounds__(256) rt_denoise_tiled_kernel(const rt_dn_level L, const int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) float4 dn_tile[];  // no static LDS: the base stays 16-byte aligned
    const int s = L.step;
    const int pitch = kTileW + 4 * s, trows = kTileH + 4;
    float4* col = dn_tile;
    float4* ga = col + pitch * trows;
    float4* gb = ga + pitch * trows;
    // tile (tx, ty): ty = (band, phase): lattice rows y0 + r s with
    // y0 = band * kTileH * s + phase, phase = 0 .. s - 1
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int band = ty / s, phase = ty - band * s;
    const int y0 = band * kTileH * s + phase;
    const int x0 = tx * kTileW, x_lo = x0 - 2 * s;
    for (int i = (int)threadIdx.x; i < pitch * trows; i += 256) {
        const int r = i / pitch, cx = i - r * pitch;
        const int qx = x_lo + cx, qy = y0 + (r - 2) * s;
        if (qx >= 0 && qx < L.width && qy >= 0 && qy < L.height) {  // texels outside the image are never read
            const long q = (long)qy * L.width + qx;
            const f3 c = dn_color<FIRST>(L, q);
            col[i] = make_float4(c.x, c.y, c.z, 0.0f);
            ga[i] = L.ga[q];
            gb[i] = L.gb[q];
        }
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & (kTileW - 1)), row = (int)(threadIdx.x / kTileW);
#pragma unroll 1
    for (int rr = row; rr < kTileH; rr += 256 / kTileW) {
        const int x = x0 + lx, y = y0 + rr * s;
        if (x < L.width && y < L.height) {
            const DnLdsFetch fetch{col, ga, gb, pitch, x_lo, rr};
            dn_store(L, (long)y * L.width + x, dn_pixel(L, x, y, fetch));
        }
    }
}

// iterations == 0: colour and RGBA of the unfiltered frame
__global__ void __launch_bounds__(256) rt_denoise_convert_kernel(const rt_dn_level L) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)L.width * L.height) return;
    dn_store(L, p, dn_color<true>(L, p));
}

}  // namespace

size_t rt_denoise_tiled_lds_bytes(int step) { return (size_t)(kTileW + 4 * step) * (kTileH + 4) * 3 * sizeof(float4); }

// One level (L.step >= 1) or, with L.step == 0, the conversion pass.
hipError_t rt_launch_denoise_level(const rt_dn_level& L, bool tiled, hipStream_t stream) {
    if (L.width <= 0 || L.height <= 0) return hipErrorInvalidValue;
    if (L.step == 0) {
        const long blocks = ((long)L.width * L.height + 255) / 256;
        hipLaunchKernelGGL(rt_denoise_convert_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, L);
        return hipGetLastError();
    }
    if (tiled) {
        const size_t lds = rt_denoise_tiled_lds_bytes(L.step);
        const long tiles_x = (L.width + kTileW - 1) / kTileW;
        // bands of kTileH * s rows, s phases each (the last band's phases past the frame end early)
        const long bands = (L.height + (long)kTileH * L.step - 1) / ((long)kTileH * L.step);
        const long blocks = tiles_x * bands * L.step;
        if (blocks > 0x7fffffffl) return hipErrorInvalidValue;
        auto k = L.first ? rt_denoise_tiled_kernel<true> : rt_denoise_tiled_kernel<false>;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), lds, stream, L, (int)tiles_x);
        return hipGetLastError();
    }
    const long tiles_x = (L.width + kDirectW - 1) / kDirectW, tiles_y = (L.height + kDirectH - 1) / kDirectH;
    if (tiles_x * tiles_y > 0x7fffffffl) return hipErrorInvalidValue;
    auto k = L.first ? rt_denoise_direct_kernel<true> : rt_denoise_direct_kernel<false>;
    hipLaunchKernelGGL(k, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, stream, L, (int)tiles_x);
    return hipGetLastError();
}
