// rt_denoise_var.hip — the variance-guided a-trous filter kernels (gfx950).
//
// rt_denoise_var.h has the arithmetic (shared with the CPU backend); this unit
// is built once with the exact flags (-ffp-contract=off, no RT_FAST), whatever
// precision mode the context renders in.
//
// One call launches the input stage, then per level a sigma pass and the level:
// input:  one lane per pixel, 32 x 8 pixel workgroups.  Tracked: frameSum and
//   the moments of the pixel alone.  Spatial: the 7 x 7 window straight from
//   global memory (frameSum planes and both guides; L1 / L2 serve the overlap).
// sigma:  one lane per pixel, the .w of the 3 x 3 unit-step neighbours; writes
//   the 4-byte plane rs.  It stays a pass of its own: the tiled level kernel
//   holds lattice rows y0 + r s, not a pixel's unit-step neighbours.
// level:  the two variants of rt_denoise.hip with the same shapes and the same
//   LDS footprint: the tile's colour plane carries v in the .w that the plain
//   filter leaves 0, and rs is read from global memory for the centre only.
#include <hip/hip_runtime.h>

#include "rt_denoise_var.h"

namespace {

constexpr int kDirectW = 32, kDirectH = 8;
constexpr int kTileW = 64, kTileH = 8;

__device__ __forceinline__ bool dv_direct_xy(const rt_dv_args& A, int tiles_x, int& x, int& y) {
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    x = tx * kDirectW + (int)(threadIdx.x & (kDirectW - 1));
    y = ty * kDirectH + (int)(threadIdx.x / kDirectW);
    return x < A.width && y < A.height;
}

__global__ void __launch_bounds__(256) rt_denoise_var_input_kernel(const rt_dv_args A, const int tiles_x) {
    int x, y;
    if (!dv_direct_xy(A, tiles_x, x, y)) return;
    dv_store(A, (long)y * A.width + x, dv_input(A, x, y));
}

__global__ void __launch_bounds__(256) rt_denoise_var_sigma_kernel(const rt_dv_args A, const int tiles_x) {
    int x, y;
    if (!dv_direct_xy(A, tiles_x, x, y)) return;
    A.rs[(long)y * A.width + x] = dv_sigma(A, x, y);
}

__global__ void __launch_bounds__(256) rt_denoise_var_direct_kernel(const rt_dv_args A, const int tiles_x) {
    int x, y;
    if (!dv_direct_xy(A, tiles_x, x, y)) return;
    const DvGlobalFetch fetch{A};
    dv_store(A, (long)y * A.width + x, dv_pixel(A, x, y, fetch));
}

// taps from the workgroup's LDS tile: texel (qx - x_lo, r + dy + 2)
struct DvLdsFetch {
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

// (the tile of rt_denoise.hip's tiled kernel: rows y0 + r s, r = -2 .. 9, of
// 64 + 4 s contiguous pixels, three float4 planes)
__global__ void __launch_bounds__(256) rt_denoise_var_tiled_kernel(const rt_dv_args A, const int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) float4 dv_tile[];  // no static LDS: the base stays 16-byte aligned
    const int s = A.step;
    const int pitch = kTileW + 4 * s, trows = kTileH + 4;
    float4* col = dv_tile;
    float4* ga = col + pitch * trows;
    float4* gb = ga + pitch * trows;
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int band = ty / s, phase = ty - band * s;
    const int y0 = band * kTileH * s + phase;
    const int x0 = tx * kTileW, x_lo = x0 - 2 * s;
    for (int i = (int)threadIdx.x; i < pitch * trows; i += 256) {
        const int r = i / pitch, cx = i - r * pitch;
        const int qx = x_lo + cx, qy = y0 + (r - 2) * s;
        if (qx >= 0 && qx < A.width && qy >= 0 && qy < A.height) {  // texels outside the image are never read
            const long q = (long)qy * A.width + qx;
            col[i] = A.src[q];
            ga[i] = A.ga[q];
            gb[i] = A.gb[q];
        }
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & (kTileW - 1)), row = (int)(threadIdx.x / kTileW);
#pragma unroll 1
    for (int rr = row; rr < kTileH; rr += 256 / kTileW) {
        const int x = x0 + lx, y = y0 + rr * s;
        if (x < A.width && y < A.height) {
            const DvLdsFetch fetch{col, ga, gb, pitch, x_lo, rr};
            dv_store(A, (long)y * A.width + x, dv_pixel(A, x, y, fetch));
        }
    }
}

size_t tiled_lds_bytes(int step) { return (size_t)(kTileW + 4 * step) * (kTileH + 4) * 3 * sizeof(float4); }

}  // namespace

// stage 0: the input stage, 1: a sigma pass, 2: a level (A.step >= 1; `tiled`
// picks the variant)
hipError_t rt_launch_denoise_var(const rt_dv_args& A, int stage, bool tiled, hipStream_t stream) {
    if (A.width <= 0 || A.height <= 0 || stage < 0 || stage > 2) return hipErrorInvalidValue;
    if (stage == 2 && (A.step < 1 || A.step > 32)) return hipErrorInvalidValue;
    if (stage == 2 && tiled) {
        const size_t lds = tiled_lds_bytes(A.step);
        const long tiles_x = (A.width + kTileW - 1) / kTileW;
        // bands of kTileH * s rows, s phases each (the last band's phases past the frame end early)
        const long bands = (A.height + (long)kTileH * A.step - 1) / ((long)kTileH * A.step);
        const long blocks = tiles_x * bands * A.step;
        if (blocks > 0x7fffffffl) return hipErrorInvalidValue;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rt_denoise_var_tiled_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(rt_denoise_var_tiled_kernel, dim3((unsigned)blocks), dim3(256), lds, stream, A,
                           (int)tiles_x);
        return hipGetLastError();
    }
    const long tiles_x = (A.width + kDirectW - 1) / kDirectW, tiles_y = (A.height + kDirectH - 1) / kDirectH;
    if (tiles_x * tiles_y > 0x7fffffffl) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(tiles_x * tiles_y));
    if (stage == 0)
        hipLaunchKernelGGL(rt_denoise_var_input_kernel, grid, dim3(256), 0, stream, A, (int)tiles_x);
    else if (stage == 1)
        hipLaunchKernelGGL(rt_denoise_var_sigma_kernel, grid, dim3(256), 0, stream, A, (int)tiles_x);
    else
        hipLaunchKernelGGL(rt_denoise_var_direct_kernel, grid, dim3(256), 0, stream, A, (int)tiles_x);
    return hipGetLastError();
}
