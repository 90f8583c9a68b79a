// projective.h -- where a 3 x 3 matrix of doubles sends a pixel, with the division (include/pwc_hip.h, "projective motion"): the
// one rule of the projective residual, warp, plate and plate difference (pwc_motion.hip, pwc_plate.hip).
//   FINITE     all nine entries are finite;
//   POSITION   D = ((m6 x) + (m7 y)) + m8; where D > 0 (a NaN fails): sx = (((m0 x) + (m1 y)) + m2) / D, sy = (((m3 x) + (m4 y)) + m5) / D;
//              elsewhere there is none.
// For a last row of exactly 0 0 1, D is exactly 1 and the quotients have the bits of the affine path's sums.  A tiny positive D
// gives a huge or infinite position, which the callers' in-frame comparisons reject -- what keeps their corner reads inside.
#pragma once
#include "flow_record.h"

#pragma clang fp contract(off)

__device__ __forceinline__ bool pwc_projective_finite(const double* m, double* e) {
    bool good = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) { e[j] = m[j]; good = good && pwc_finite(e[j]); }
    return good;
}

__device__ __forceinline__ bool pwc_projective_position(const double* m, double x, double y, double& sx, double& sy) {
    const double D = ((m[6] * x) + (m[7] * y)) + m[8];
    if (!(D > 0.0)) return false;
    sx = (((m[0] * x) + (m[1] * y)) + m[2]) / D;
    sy = (((m[3] * x) + (m[4] * y)) + m[5]) / D;
    return true;
}
