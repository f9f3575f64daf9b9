// rt_kernels_nee_bvh.hip — the BVH instantiations of the next-event estimation
// kernel (rt_kernel_nee.h: hit table in global memory, wave-synchronous walk),
// compiled at -O3 like rt_kernels_bvh.hip (see Makefile).
#define RT_NEE_ROOT_BVH
#include "rt_kernel_nee.h"
