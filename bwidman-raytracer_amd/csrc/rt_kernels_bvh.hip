// rt_kernels_bvh.hip — the exact BVH render kernels (ray refill, and the simple
// kernel's BVH instantiation) with their launchers, and the BVH feature-buffer
// kernel, compiled at -O3 in their own translation unit (see Makefile).
#include "rt_kernel_refill.h"
