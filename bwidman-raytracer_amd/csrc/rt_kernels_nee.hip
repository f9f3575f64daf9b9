// rt_kernels_nee.hip — the render kernel of next-event estimation
// (rt_kernel_nee.h; rt_set_light_sampling) over the brute-force loop, with its
// launch policy, built with the flags of rt_kernels.hip (see Makefile).  Exact
// arithmetic only: there is no reference-fast twin.
#include "rt_kernel_nee.h"
