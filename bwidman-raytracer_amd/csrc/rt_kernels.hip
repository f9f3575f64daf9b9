// rt_kernels.hip — the exact brute-force render kernels (simple, sorted with
// its sky groups, pair) with their launch policy, at -O1 (see Makefile).
#include "rt_launch_brute.h"
