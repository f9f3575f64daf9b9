// rt_temporal_var.hip — the moment-carrying reprojection kernel and the input
// stage of the variance-guided levels behind it (gfx950), one launch each.
//
// rt_temporal_var.h has the arithmetic (shared with the CPU backend); this unit
// is built once with the exact flags (-ffp-contract=off, no RT_FAST), whatever
// precision mode the context renders in.
//
// reprojection: one lane per pixel (rt_atrous_tile.h), no LDS: rt_temporal.hip's
//   kernel with three more accesses.  The pixel's own {M, M2} is read only when
//   the frame's moments are tracked (M2 alone is used, and the compiler narrows
//   the load to it); a tap's {s2, dof} is one 8-byte load (tv_load2), made only
//   once the tap has passed every test of the colour path and only when the
//   history set has a moment plane; the pending {s2, dof} is one 8-byte store.
//   Uniform scalars (n, dof_c, the history camera) come from the kernel
//   arguments.  Per pixel: 44 B read + 56 B written (60 with the RGBA) without history, up to
//   4 x 56 B of taps more with one (L1 / L2 serve the overlap of neighbouring
//   lanes' footprints: about 56 B per pixel reach HBM).  On a non-uniform frame
//   (TvPixelCnt) the lane's {n_p, J_p} is one 8-byte load more.
// input: one lane per pixel.  Temporal source: the pending colour + length and
//   moments of the pixel alone (24 B read, 16 B written).  Spatial source: the
//   7 x 7 window of rt_denoise_var's input stage over the pending colours
//   (one 16-byte load per tap where that stage reads three planes).
#include <hip/hip_runtime.h>

#include "rt_atrous_tile.h"
#include "rt_temporal_var.h"

namespace {

struct TvPixel {
    using Args = rt_tv_args;
    static RT_HD int2 size(const rt_tv_args& V) { return make_int2(V.t.width, V.t.height); }
    static __device__ __forceinline__ void run(const rt_tv_args& V, int x, int y) { tv_run_pixel(V, x, y); }
};

// a non-uniform frame: the lane's {n_p, J_p} (8 bytes) in place of the uniform
// n, inv and dof_c; the counts' pointer lies behind TvPixel's arguments
struct TvPixelCnt {
    using Args = rt_tv_cnt_args;
    static RT_HD int2 size(const rt_tv_cnt_args& V) { return make_int2(V.t.width, V.t.height); }
    static __device__ __forceinline__ void run(const rt_tv_cnt_args& V, int x, int y) { tv_run_pixel_cnt(V, x, y); }
};

struct TvInput {
    using Args = rt_tv_input;
    static RT_HD int2 size(const rt_tv_input& A) { return make_int2(A.f.width, A.f.height); }
    static __device__ __forceinline__ void run(const rt_tv_input& A, int x, int y) {
        at_store(A.f, (long)y * A.f.width + x, tv_input(A, x, y));
    }
};

}  // namespace

hipError_t rt_launch_temporal_var(const rt_tv_cnt_args& V, hipStream_t stream) {
    if (V.cnt) return at_launch_pixels<TvPixelCnt>(V, stream);
    return at_launch_pixels<TvPixel>(V, stream);
}

hipError_t rt_launch_temporal_var_input(const rt_tv_input& A, hipStream_t stream) {
    return at_launch_pixels<TvInput>(A, stream);
}
