// rt_light_probs.hip — rt_light_pick_probabilities on a GPU context: one
// shading point per lane, each writing its row of n_lights probabilities through
// rt_light.h's nee_pick_probabilities, the functions nee_sample picks with.
// Built with the flags of rt_kernels_nee.hip (see Makefile).  Exact arithmetic
// only.  An introspection kernel: nothing of the render kernels' tuning applies.
#include "rt_launch.h"
#include "rt_light.h"

namespace {
template <int SHAPES>
__global__ void __launch_bounds__(64) rt_pick_probabilities_kernel(rt_nee_args N, int n_sph, const float* points, const int* prims,
                                                                   int count, float* out) {
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const float* q = points + 6 * i;
    const int prim = prims[i];
    nee_pick_probabilities<SHAPES>(N, mk(q[0], q[1], q[2]), mk(q[3], q[4], q[5]), prim, prim >= 0 && prim < n_sph,
                                   out + (size_t)i * N.n_lights);
}
}  // namespace

// points: count x {P.xyz, n.xyz}; out: count x N.n_lights (device pointers); count > 0, N.n_lights > 0
hipError_t rt_launch_pick_probabilities(const rt_nee_args& N, int n_sph, const float* points, const int* prims, int count,
                                        float* out, hipStream_t s) {
    const unsigned grid = (unsigned)(((long)count + 63) / 64);
    if (N.n_lights > N.n_sphere_lights)
        hipLaunchKernelGGL(rt_pick_probabilities_kernel<RT_SHAPES_ALL>, dim3(grid), dim3(64), 0, s, N, n_sph, points, prims, count, out);
    else
        hipLaunchKernelGGL(rt_pick_probabilities_kernel<RT_SHAPES_SPHERES>, dim3(grid), dim3(64), 0, s, N, n_sph, points, prims, count,
                           out);
    return hipGetLastError();
}
