// rt_temporal.hip — the temporal reprojection kernel (gfx950), one launch.
//
// rt_temporal.h has the arithmetic (shared with the CPU backend); this unit is
// built once with the exact flags (-ffp-contract=off, no RT_FAST), whatever
// precision mode the context renders in.
//
// One lane per pixel, 32 x 8 pixel workgroups.  A lane reads its two guide
// words (2 x 16 bytes) and frameSum (3 planes), decides miss / behind /
// off-screen before any history load, then reads up to four taps of {guide a,
// guide b, colour + length} = 3 x 16 bytes each, every one behind the test
// that needs it (a tap of another primitive costs one load).  Neighbouring
// lanes' footprints overlap: L1 / L2 serve the taps, no LDS.  It writes the
// pending colour + length, the copy of the guides and, when no spatial filter
// follows, the RGBA: there is no conversion pass.
#include <hip/hip_runtime.h>

#include "rt_temporal.h"

namespace {

constexpr int kTileW = 32, kTileH = 8;

__global__ void __launch_bounds__(256) rt_temporal_kernel(const rt_tp_args T, const int tiles_x) {
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int x = tx * kTileW + (int)(threadIdx.x & (kTileW - 1));
    const int y = ty * kTileH + (int)(threadIdx.x / kTileW);
    if (x >= T.width || y >= T.height) return;
    tp_run_pixel(T, x, y);
}

}  // namespace

hipError_t rt_launch_temporal(const rt_tp_args& T, hipStream_t stream) {
    if (T.width <= 0 || T.height <= 0) return hipErrorInvalidValue;
    const long tiles_x = (T.width + kTileW - 1) / kTileW, tiles_y = (T.height + kTileH - 1) / kTileH;
    if (tiles_x * tiles_y > 0x7fffffffl) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_temporal_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, stream, T,
                       (int)tiles_x);
    return hipGetLastError();
}
