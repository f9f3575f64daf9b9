// rt_moments.h — luminance moment tracking: one weighted Welford step per
// render call, shared by the HIP kernel (rt_moments.hip, device pass) and the
// CPU backend (rt_cpu.cpp, host pass).  Every float operation is one rounding
// in the order written (both passes built with -ffp-contract=off), so the two
// backends agree bit for bit.
//
// A render call adds a batch of k frames f0 .. f0 + k - 1 to frameSum
// (n0 = f0 - 1 frames before it).  With a = frameSum after the call:
//   d  = a - prev                          per channel
//   L  = (0.2126 d.x + 0.7152 d.y) + 0.0722 d.z
//   l  = L invk                            the batch's mean luminance
//   dl = l - M
//   M' = M + dl kw                         kw = k / (n0 + k)
//   M2' = M2 + (kf dl) (l - M')
//   prev' = a
// (prev, M, M2 = 0 at f0 == 1, without reading them).  This is Welford's
// update with weights k_j: after J batches M is the pixel's mean luminance
// over all n frames and M2 = sum_j k_j (l_j - M)^2.  A batch mean l_j has
// variance sigma^2 / k_j (sigma^2: the variance of one frame's luminance), so
// E[M2] = sigma^2 (J - 1) for batches of any sizes, and
//   var = M2 / ((J - 1) n)
// is an unbiased estimate of sigma^2 / n: the variance of the pixel's MEAN
// luminance after n frames (not of one sample).
#pragma once
#include "rt_path.h"

namespace {

// Rec. 709 luminance, the sum in this order
RT_HD float mom_lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

RT_HD void mom_update(const rt_mom_args& A, long p) {
    const float ax = A.accum[p], ay = A.accum[A.npix + p], az = A.accum[2 * A.npix + p];
    float px = 0.0f, py = 0.0f, pz = 0.0f, M = 0.0f, M2 = 0.0f;
    if (!A.first) {
        px = A.prev[p];
        py = A.prev[A.npix + p];
        pz = A.prev[2 * A.npix + p];
        const float2 m = A.mom[p];
        M = m.x;
        M2 = m.y;
    }
    const float L = mom_lum(ax - px, ay - py, az - pz);
    const float l = L * A.invk;
    const float dl = l - M;
    const float M1 = M + dl * A.kw;
    const float M2n = M2 + (A.kf * dl) * (l - M1);
    A.prev[p] = ax;
    A.prev[A.npix + p] = ay;
    A.prev[2 * A.npix + p] = az;
    A.mom[p] = make_float2(M1, M2n);
}

}  // namespace
