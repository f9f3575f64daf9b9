// rt_kernels_bvh_fast.hip — the reference-fast BVH instantiations
// (rt_fast::rt_launch_render_bvh_*): rt_kernels_bvh.hip's flags plus
// -ffp-contract=fast (see rt_kernels_fast.hip).
#define RT_FAST
#include "rt_kernel_refill.h"
