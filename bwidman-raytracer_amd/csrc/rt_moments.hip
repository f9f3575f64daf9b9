// rt_moments.hip — the luminance moment update kernel (gfx950), one launch per
// render call of a context with tracking on (rt_set_moments).
//
// rt_moments.h has the arithmetic (shared with the CPU backend); this unit is
// built once with the exact flags (-ffp-contract=off, no RT_FAST), whatever
// precision mode the context renders in.
//
// One lane per pixel, no neighbours: it reads frameSum (3 planes), the copy of
// frameSum before the batch (3 planes) and {M, M2} (8 bytes), and writes the
// copy and {M, M2}: 52 bytes per pixel, every access coalesced (the first batch
// of an accumulation reads frameSum only: 32 bytes).
#include <hip/hip_runtime.h>

#include "rt_moments.h"

namespace {

__global__ void __launch_bounds__(256) rt_moments_kernel(const rt_mom_args A) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.npix) return;
    mom_update(A, p);
}

}  // namespace

hipError_t rt_launch_moments(const rt_mom_args& A, hipStream_t stream) {
    if (A.npix <= 0 || !A.accum || !A.prev || !A.mom) return hipErrorInvalidValue;
    const long blocks = (A.npix + 255) / 256;
    if (blocks > 0x7fffffffl) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_moments_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, A);
    return hipGetLastError();
}
