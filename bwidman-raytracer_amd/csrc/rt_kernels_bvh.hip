// rt_kernels_bvh.hip — the exact BVH render kernels (ray refill, and the simple
// kernel's BVH instantiation) with their launchers, and the BVH feature-buffer
// kernel, compiled at -O3 in their own translation unit (see Makefile).
// The one-path-per-lane list kernel's BVH instantiation (rt_kernel_list.h) too.
#include "rt_kernel_refill.h"
#define RT_LIST_ROOT_BVH
#include "rt_kernel_list.h"
