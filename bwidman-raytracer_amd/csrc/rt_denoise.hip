// rt_denoise.hip — the a-trous filter kernels (gfx950), one launch per level.
//
// rt_denoise.h has the arithmetic (shared with the CPU backend); this unit is
// built once with the exact flags (-ffp-contract=off, no RT_FAST), whatever
// precision mode the context renders in.
//
// Level 0 reads frameSum (three planes) and applies 1/n, the last level also
// stores the tone-mapped RGBA8: there are no conversion passes.  The colour
// ping-pongs between two float4 buffers; a tap reads {colour, guide a, guide
// b} = 3 x 16 bytes.  The two variants of a level, direct (one lane per pixel,
// the 25 taps from global memory) and tiled (the taps staged in LDS), are the
// kernels of rt_atrous_tile.h with DnFilter for their filter.  In the
// non-uniform state (L.cnt) level 0 and the conversion pass take DnFilterCnt:
// a texel then costs the pixel's count (8 bytes) on top of frameSum's 12, once
// per staged texel in the tiled kernel; there is no resolve pre-pass.
#include <hip/hip_runtime.h>

#include "rt_atrous_tile.h"
#include "rt_denoise.h"

namespace {

// iterations == 0: colour and RGBA of the unfiltered frame
__global__ void __launch_bounds__(256) rt_denoise_convert_kernel(const rt_dn_level L) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)L.f.width * L.f.height) return;
    at_store(L.f, p, DnFilter<true>::texel(L, p));
}

// the same in the non-uniform state: every pixel's own count (one 8-byte load
// more per pixel than the uniform kernel's 12 + 16)
__global__ void __launch_bounds__(256) rt_denoise_convert_cnt_kernel(const rt_dn_level L) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)L.f.width * L.f.height) return;
    at_store(L.f, p, DnFilterCnt::texel(L, p));
}

template <class P>
hipError_t launch_level(const typename P::Args& L, bool tiled, hipStream_t stream) {
    return tiled ? at_launch_tiled<P>(L, stream) : at_launch_pixels<AtDirect<P>>(L, stream);
}

}  // namespace

// One level (L.f.step >= 1) or, with L.f.step == 0, the conversion pass.
hipError_t rt_launch_denoise_level(const rt_dn_level& L, bool tiled, hipStream_t stream) {
    if (L.f.step == 0) {
        if (L.f.width <= 0 || L.f.height <= 0) return hipErrorInvalidValue;
        const long blocks = ((long)L.f.width * L.f.height + 255) / 256;
        hipLaunchKernelGGL(L.cnt ? rt_denoise_convert_cnt_kernel : rt_denoise_convert_kernel, dim3((unsigned)blocks),
                           dim3(256), 0, stream, L);
        return hipGetLastError();
    }
    if (!L.first) return launch_level<DnFilter<false>>(L, tiled, stream);
    return L.cnt ? launch_level<DnFilterCnt>(L, tiled, stream) : launch_level<DnFilter<true>>(L, tiled, stream);
}
