// rt_kernels_fast.hip — the reference-fast instantiations of the brute-force
// render kernels (rt_fast::rt_launch_render; RT_PRECISION_REFERENCE_FAST),
// compiled with -ffp-contract=fast in their own translation unit: hardware
// rcp / sqrt / rsq / sin / cos and contracted FMAs, as the reference's own
// --use_fast_math build (rt_path.h, rt_sqrt.h).  Never -ffast-math: the isnan
// guard of specular_weight must survive.
#define RT_FAST
#include "rt_launch_brute.h"
