// rt_kernels.hip — the exact brute-force render kernels (simple, sorted with
// its sky groups, pair) with their launch policy, at -O1 (see Makefile).
// The list kernels of an adaptive call (rt_kernel_list.h) live here too.
#include "rt_launch_brute.h"
#include "rt_kernel_list.h"
