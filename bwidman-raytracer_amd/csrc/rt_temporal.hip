// rt_temporal.hip — the temporal reprojection kernel (gfx950), one launch.
//
// rt_temporal.h has the arithmetic (shared with the CPU backend); this unit is
// built once with the exact flags (-ffp-contract=off, no RT_FAST), whatever
// precision mode the context renders in.
//
// One lane per pixel (rt_atrous_tile.h).  A lane reads its two guide
// words (2 x 16 bytes) and frameSum (3 planes), decides miss / behind /
// off-screen before any history load, then reads up to four taps of {guide a,
// guide b, colour + length} = 3 x 16 bytes each, every one behind the test
// that needs it (a tap of another primitive costs one load).  Neighbouring
// lanes' footprints overlap: L1 / L2 serve the taps, no LDS.  It writes the
// pending colour + length, the copy of the guides and, when no spatial filter
// follows, the RGBA: there is no conversion pass.
#include <hip/hip_runtime.h>

#include "rt_atrous_tile.h"
#include "rt_temporal.h"

namespace {

struct TpPixel {
    using Args = rt_tp_uniform;
    static RT_HD int2 size(const rt_tp_uniform& T) { return make_int2(T.width, T.height); }
    static __device__ __forceinline__ void run(const rt_tp_uniform& T, int x, int y) { tp_run_pixel(T, x, y); }
};

// the non-uniform state: the lane's count (8 bytes) in place of the uniform n, inv
struct TpPixelCnt : TpPixel {
    using Args = rt_tp_args;
    static __device__ __forceinline__ void run(const rt_tp_args& T, int x, int y) { tp_run_pixel_cnt(T, x, y); }
};

}  // namespace

hipError_t rt_launch_temporal(const rt_tp_args& T, hipStream_t stream) {
    if (T.cnt) return at_launch_pixels<TpPixelCnt>(T, stream);
    return at_launch_pixels<TpPixel>(T, stream);
}
