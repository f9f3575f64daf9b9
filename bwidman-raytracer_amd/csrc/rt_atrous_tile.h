// rt_atrous_tile.h — the two kernel shapes of the post-render passes (gfx950,
// device only) and their launchers, shared by rt_denoise.hip,
// rt_denoise_var.hip and rt_temporal.hip.
//
// pixels: one lane per pixel, 32 x 8 pixel workgroups; whatever a pixel reads
//   comes straight from global memory (L1 / L2 serve the overlap between
//   neighbours).
// tiled:  one level of an a-trous filter (rt_atrous.h).  A workgroup stages the
//   taps of 64 contiguous pixels in x by 8 LATTICE rows in LDS.  Rows with the
//   same y mod s form an independent step-1 problem in y, so a tile of rows
//   y0 + r s (r = -2 .. 9) needs only 2 halo rows each side at any step, and
//   its x range (64 + 4 s pixels) stays contiguous, so the staging loads are
//   coalesced.  (64 + 4 s) x 12 texels of 48 bytes: 38 KiB at s = 1, 108 KiB
//   at s = 32.  Loads per output pixel: 1.6 (s = 1) to 4.5 (s = 32) instead of
//   25.  Colour, guide a and guide b are three separate float4 planes in LDS:
//   a wave's ds_read_b128 then reads 64 consecutive 16-byte words (no bank
//   conflict beyond the 4-pass minimum).
#pragma once
#include <hip/hip_runtime.h>

#include "rt_atrous.h"

namespace {

constexpr int kPixW = 32, kPixH = 8;
constexpr int kTileW = 64, kTileH = 8;

// Op::run(A, x, y) for every pixel of A's Op::size(A) = {width, height} image (A: Op::Args)
template <class Op>
__global__ void __launch_bounds__(256) at_pixel_kernel(const typename Op::Args A, const int tiles_x) {
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int x = tx * kPixW + (int)(threadIdx.x & (kPixW - 1));
    const int y = ty * kPixH + (int)(threadIdx.x / kPixW);
    if (x >= Op::size(A).x || y >= Op::size(A).y) return;
    Op::run(A, x, y);
}

template <class Op>
hipError_t at_launch_pixels(const typename Op::Args& A, hipStream_t stream) {
    const int width = Op::size(A).x, height = Op::size(A).y;
    if (width <= 0 || height <= 0) return hipErrorInvalidValue;
    const long tiles_x = (width + kPixW - 1) / kPixW, tiles_y = (height + kPixH - 1) / kPixH;
    if (tiles_x * tiles_y > 0x7fffffffl) return hipErrorInvalidValue;
    hipLaunchKernelGGL(at_pixel_kernel<Op>, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, stream, A,
                       (int)tiles_x);
    return hipGetLastError();
}

// a level of filter P with the taps from global memory, as an Op
template <class P>
struct AtDirect {
    using Args = typename P::Args;
    static RT_HD int2 size(const Args& A) { return make_int2(A.f.width, A.f.height); }
    static __device__ __forceinline__ void run(const Args& A, int x, int y) { at_run_direct<P>(A, x, y); }
};

// taps from the workgroup's LDS tile: texel (qx - x_lo, row + dy + 2)
struct AtLdsFetch {
    const float4* col;
    const float4* ga;
    const float4* gb;
    int pitch, x_lo, row;  // row = the lane's lattice row in the tile (0 .. kTileH - 1)
    __device__ __forceinline__ void operator()(int, int dy, int qx, int, float4& c, float4& a, float4& b) const {
        const int i = (row + dy + 2) * pitch + (qx - x_lo);
        a = ga[i];
        b = gb[i];
        c = col[i];
    }
};

template <class P>
__global__ void __launch_bounds__(256) at_tiled_kernel(const typename P::Args A, const int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) float4 at_tile[];  // no static LDS: the base stays 16-byte aligned
    const rt_at_frame& F = A.f;
    const int s = F.step;
    const int pitch = kTileW + 4 * s, trows = kTileH + 4;
    float4* col = at_tile;
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
        if (qx >= 0 && qx < F.width && qy >= 0 && qy < F.height) {  // texels outside the image are never read
            const long q = (long)qy * F.width + qx;
            col[i] = P::texel(A, q);
            ga[i] = F.ga[q];
            gb[i] = F.gb[q];
        }
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & (kTileW - 1)), row = (int)(threadIdx.x / kTileW);
#pragma unroll 1
    for (int rr = row; rr < kTileH; rr += 256 / kTileW) {
        const int x = x0 + lx, y = y0 + rr * s;
        if (x < F.width && y < F.height) {
            const AtLdsFetch fetch{col, ga, gb, pitch, x_lo, rr};
            P::run(A, x, y, fetch);
        }
    }
}

// one level (A.f.step = 1 .. 32) of filter P by the tiled kernel
template <class P>
hipError_t at_launch_tiled(const typename P::Args& A, hipStream_t stream) {
    const rt_at_frame& F = A.f;
    if (F.width <= 0 || F.height <= 0 || F.step < 1 || F.step > 32) return hipErrorInvalidValue;
    const size_t lds = (size_t)(kTileW + 4 * F.step) * (kTileH + 4) * 3 * sizeof(float4);
    const long tiles_x = (F.width + kTileW - 1) / kTileW;
    // bands of kTileH * s rows, s phases each (the last band's phases past the frame end early)
    const long bands = (F.height + (long)kTileH * F.step - 1) / ((long)kTileH * F.step);
    const long blocks = tiles_x * bands * F.step;
    if (blocks > 0x7fffffffl) return hipErrorInvalidValue;
    // (above 64 KiB of dynamic LDS the kernel needs the attribute)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(at_tiled_kernel<P>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(at_tiled_kernel<P>, dim3((unsigned)blocks), dim3(256), lds, stream, A, (int)tiles_x);
    return hipGetLastError();
}

}  // namespace
