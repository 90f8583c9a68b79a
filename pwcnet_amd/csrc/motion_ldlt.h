// motion_ldlt.h -- the one elimination the parametric fits share (pwc_motion.hip: 3 x 3 and 4 x 4; pwc_homography.hip: 8 x 8), so
// that its order of operations is written once (include/pwc_hip.h, "dominant motion"; tests/motion_ref.py's ldlt restates it).
#pragma once
#include "pwc_common.h"

#pragma clang fp contract(off)

// L D L^T elimination of the symmetric K x K system A (lower triangle read) with R right-hand sides, no pivoting:
//   column j:  t_ij = A_ij - l_i0 t_j0 - ... - l_i,j-1 t_j,j-1 (left to right), i = j .. K - 1;  d_j = t_jj;  l_ij = t_ij / d_j
//   per side:  z_i = r_i - l_i0 z_0 - ... - l_i,i-1 z_i-1;  y_i = z_i / d_i;  x_i = y_i - l_i+1,i x_i+1 - ... - l_K-1,i x_K-1
// false where a pivot fails d_j > tol (a NaN fails); the solutions overwrite r.
template <int K, int R>
__device__ __forceinline__ bool motion_ldlt(const double (&A)[K][K], double (&r)[R][K], double tol) {
    double t[K][K], l[K][K], d[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int i = j; i < K; ++i) {
            double v = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - (l[i][k] * t[j][k]);
            t[i][j] = v;
        }
        d[j] = t[j][j];
        if (!(d[j] > tol)) return false;
#pragma unroll
        for (int i = j + 1; i < K; ++i) l[i][j] = t[i][j] / d[j];
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
        double z[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double v = r[q][i];
#pragma unroll
            for (int k = 0; k < i; ++k) v = v - (l[i][k] * z[k]);
            z[i] = v;
        }
#pragma unroll
        for (int i = K - 1; i >= 0; --i) {
            double v = z[i] / d[i];
#pragma unroll
            for (int k = i + 1; k < K; ++k) v = v - (l[k][i] * r[q][k]);
            r[q][i] = v;
        }
    }
    return true;
}
