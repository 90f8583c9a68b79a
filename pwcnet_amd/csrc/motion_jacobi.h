// motion_jacobi.h -- the one symmetric eigen-decomposition of the epipolar fit (pwc_fundamental.hip: 9 x 9 for the matrix, 3 x 3 for
// its rank), so that its order of operations is written once (include/pwc_hip.h, "epipolar motion"; tests/fundamental_ref.py's
// jacobi restates it as a scalar loop).
#pragma once
#include "pwc_common.h"

#pragma clang fp contract(off)

#define MOTION_JACOBI_SWEEPS 10   // six bring the off-diagonal part of the test scene's matrix to 1e-13 of the trace, four do not

// Cyclic Jacobi decomposition of the symmetric K x K matrix A: only the entries A[i][j] with i <= j are read and written, every
// index is a compile-time constant (the three loops unroll), so A and V live in registers.  MOTION_JACOBI_SWEEPS sweeps over
// (p, q), p < q, in row order; an entry A[p][q] that is exactly 0 is skipped; else
//   theta = (A[q][q] - A[p][p]) / (2 A[p][q]);  t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt((theta theta) + 1));
//   c = 1 / sqrt((t t) + 1);  s = t c;
//   k != p, q:  A[k][p] <- (c A[k][p]) - (s A[k][q]);  A[k][q] <- (s A[k][p]) + (c A[k][q])   (both from the old values)
//   A[p][p] <- A[p][p] - (t A[p][q]);  A[q][q] <- A[q][q] + (t A[p][q]);  A[p][q] <- 0
//   every k:    V[k][p] <- (c V[k][p]) - (s V[k][q]);  V[k][q] <- (s V[k][p]) + (c V[k][q])
// V starts as the identity.  On return A[j][j] is eigenvalue j and column j of V its eigenvector.  sqrt is the only library call.
#define MOTION_JACOBI_AT(A, i, j) A[(i) < (j) ? (i) : (j)][(i) < (j) ? (j) : (i)]
template <int K>
__device__ __forceinline__ void motion_jacobi(double (&A)[K][K], double (&V)[K][K]) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
#pragma unroll
        for (int j = 0; j < K; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    }
#pragma unroll 1
    for (int sweep = 0; sweep < MOTION_JACOBI_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < K - 1; ++p) {
#pragma unroll
            for (int q = p + 1; q < K; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt((theta * theta) + 1.0));
                const double c = 1.0 / sqrt((t * t) + 1.0);
                const double s = t * c;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (k == p || k == q) continue;
                    const double akp = MOTION_JACOBI_AT(A, k, p), akq = MOTION_JACOBI_AT(A, k, q);
                    MOTION_JACOBI_AT(A, k, p) = (c * akp) - (s * akq);
                    MOTION_JACOBI_AT(A, k, q) = (s * akp) + (c * akq);
                }
                A[p][p] = A[p][p] - (t * apq);
                A[q][q] = A[q][q] + (t * apq);
                A[p][q] = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = (c * vkp) - (s * vkq);
                    V[k][q] = (s * vkp) + (c * vkq);
                }
            }
        }
    }
}

// The column of V whose eigenvalue A[j][j] is the smallest, ties to the lowest column, leaving out column `skip` (-1: none);
// returns the eigenvalue.  `which` gets the column (as a value; no array is indexed with it).
template <int K>
__device__ __forceinline__ double motion_jacobi_smallest(const double (&A)[K][K], const double (&V)[K][K], int skip, double (&col)[K],
                                                         int& which) {
    double best = 0.0;
    which = -1;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j != skip && (which < 0 || A[j][j] < best)) {
            best = A[j][j];
            which = j;
#pragma unroll
            for (int k = 0; k < K; ++k) col[k] = V[k][j];
        }
    }
    return best;
}
