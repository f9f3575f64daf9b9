// rt_denoise_var.hip — the variance-guided a-trous filter kernels (gfx950).
//
// rt_denoise_var.h has the arithmetic (shared with the CPU backend); this unit
// is built once with the exact flags (-ffp-contract=off, no RT_FAST), whatever
// precision mode the context renders in.
//
// One call launches the input stage, then per level a sigma pass and the level:
// input:  one lane per pixel (rt_atrous_tile.h).  Tracked: frameSum and the
//   moments of the pixel alone.  Spatial: the 7 x 7 window straight from global
//   memory (frameSum planes and both guides; L1 / L2 serve the overlap).
// sigma:  one lane per pixel, the .w of the 3 x 3 unit-step neighbours; writes
//   the 4-byte plane rs.  It stays a pass of its own: the tiled level kernel
//   holds lattice rows y0 + r s, not a pixel's unit-step neighbours.
// level:  the direct and the tiled kernel of rt_atrous_tile.h with DvFilter for
//   their filter: the tile's colour plane carries v in the .w that the plain
//   filter does not read, and rs is read from global memory for the centre only.
#include <hip/hip_runtime.h>

#include "rt_atrous_tile.h"
#include "rt_denoise_var.h"

namespace {

struct DvOp {  // a one-lane-per-pixel pass over the frame
    using Args = rt_dv_uniform;
    static RT_HD int2 size(const rt_dv_uniform& A) { return make_int2(A.f.width, A.f.height); }
};

struct DvInput : DvOp {
    static __device__ __forceinline__ void run(const rt_dv_uniform& A, int x, int y) {
        at_store(A.f, (long)y * A.f.width + x, dv_input(A, x, y));
    }
};

// the input stage in the non-uniform state: a lane branches on its own J_p
// between the tracked source (count, frameSum, moments of the pixel alone) and
// the 7 x 7 window, whose taps read their counts beside their frameSum
struct DvInputCnt : DvOp {
    using Args = rt_dv_args;
    static __device__ __forceinline__ void run(const rt_dv_args& A, int x, int y) {
        at_store(A.f, (long)y * A.f.width + x, dv_input_cnt(A, x, y));
    }
};

struct DvSigma : DvOp {
    static __device__ __forceinline__ void run(const rt_dv_uniform& A, int x, int y) {
        A.rs[(long)y * A.f.width + x] = dv_sigma(A, x, y);
    }
};

}  // namespace

// stage 0: the input stage, 1: a sigma pass, 2: a level (A.f.step >= 1; `tiled`
// picks the variant)
hipError_t rt_launch_denoise_var(const rt_dv_args& A, int stage, bool tiled, hipStream_t stream) {
    if (stage < 0 || stage > 2) return hipErrorInvalidValue;
    if (stage == 2 && (A.f.step < 1 || A.f.step > 32)) return hipErrorInvalidValue;
    if (stage == 2 && tiled) return at_launch_tiled<DvFilter>(A, stream);
    if (stage == 0 && A.cnt) return at_launch_pixels<DvInputCnt>(A, stream);
    return stage == 0   ? at_launch_pixels<DvInput>(A, stream)
           : stage == 1 ? at_launch_pixels<DvSigma>(A, stream)
                        : at_launch_pixels<AtDirect<DvFilter>>(A, stream);
}
