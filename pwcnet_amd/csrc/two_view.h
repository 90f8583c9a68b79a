// two_view.h -- the per-pixel core that the cheirality vote and the depth kernel of pwc_pose.hip, pwc_trajectory.hip and the sums of
// pwc_pose_refine.hip share, so that its order of operations is written once (include/pwc_hip.h, "relative pose and depth" and
// "pose refinement"; tests/pose_ref.py and tests/pose_refine_ref.py restate it in numpy): SAMPSON, which pwc_fundamental.hip's
// weights and residual use too, the ray of a pixel, the triangulation of a pixel pair under a candidate pose, the
// epipolar residual on the rays and the tangent basis of a translation.
#pragma once
#include "flow_record.h"

#pragma clang fp contract(off)

// SAMPSON of "epipolar motion": r = p'^T F p and g = l0^2 + l1^2 + l'0^2 + l'1^2 with l = F p, l' = F^T p'.
__device__ __forceinline__ void two_view_sampson(const double* f, double x, double y, double xp, double yp, double& r, double& g) {
    const double l0 = ((f[0] * x) + (f[1] * y)) + f[2];
    const double l1 = ((f[3] * x) + (f[4] * y)) + f[5];
    const double l2 = ((f[6] * x) + (f[7] * y)) + f[8];
    r = ((xp * l0) + (yp * l1)) + l2;
    const double m0 = ((f[0] * xp) + (f[3] * yp)) + f[6];
    const double m1 = ((f[1] * xp) + (f[4] * yp)) + f[7];
    g = (((l0 * l0) + (l1 * l1)) + (m0 * m0)) + (m1 * m1);
}

// fx, fy, cx, cy usable: all finite, both focal lengths positive.
__device__ __forceinline__ bool two_view_intrinsics_fine(const double* k) {
    return pwc_finite(k[0]) && pwc_finite(k[1]) && pwc_finite(k[2]) && pwc_finite(k[3]) && k[0] > 0.0 && k[1] > 0.0;
}

// What a pixel pair says under the pose (R, t), X' = R X + t.  d0 = K^-1 p = (d0x, d0y, 1) and d1 = K^-1 p' = (d1x, d1y, 1) are
// the rays; a = R d0 is the first ray in the second camera's frame.  Z1 d1 = Z0 a + t, crossed with d1: Z0 (d1 x a) = -(d1 x t).
struct TwoViewPoint {
    double a0, a1, a2;        // R d0
    double den;               // |d1 x a|^2
    double z0, z1;            // the depths in the first and the second camera, in baselines
};

// a = R d0, c = d1 x a and e = d1 x t, the three vectors everything below is made of.
struct TwoViewVectors {
    double a0, a1, a2, c0, c1, c2, e0, e1, e2;
};

__device__ __forceinline__ TwoViewVectors two_view_vectors(const double* R, const double* t, double d0x, double d0y, double d1x,
                                                           double d1y) {
    TwoViewVectors v;
    v.a0 = ((R[0] * d0x) + (R[1] * d0y)) + R[2];
    v.a1 = ((R[3] * d0x) + (R[4] * d0y)) + R[5];
    v.a2 = ((R[6] * d0x) + (R[7] * d0y)) + R[8];
    v.c0 = (d1y * v.a2) - v.a1; v.c1 = v.a0 - (d1x * v.a2); v.c2 = (d1x * v.a1) - (d1y * v.a0);
    v.e0 = (d1y * t[2]) - t[1]; v.e1 = t[0] - (d1x * t[2]); v.e2 = (d1x * t[1]) - (d1y * t[0]);
    return v;
}

__device__ __forceinline__ TwoViewPoint two_view_triangulate(const double* R, const double* t, double d0x, double d0y, double d1x,
                                                             double d1y) {
    const TwoViewVectors v = two_view_vectors(R, t, d0x, d0y, d1x, d1y);
    TwoViewPoint p;
    p.a0 = v.a0; p.a1 = v.a1; p.a2 = v.a2;
    p.den = ((v.c0 * v.c0) + (v.c1 * v.c1)) + (v.c2 * v.c2);
    p.z0 = -(((v.c0 * v.e0) + (v.c1 * v.e1)) + (v.c2 * v.e2)) / p.den;
    p.z1 = (p.z0 * p.a2) + t[2];
    return p;
}

// EPIPOLAR of "pose refinement": the epipolar residual of a pixel pair under the pose (R, t) on the rays, and its gradient taken to
// pixels.  With E = [t]x R: r = d1 . (E d0) = e . a; l = E d0 = t x a and m = E^T d1 = R^T e, of which the first two entries are used.
struct TwoViewEpipolar {
    double a0, a1, a2, c0, c1, c2, e0, e1, e2;
    double r, g;
};

__device__ __forceinline__ TwoViewEpipolar two_view_epipolar(const double* R, const double* t, double fx, double fy, double d0x,
                                                             double d0y, double d1x, double d1y) {
    const TwoViewVectors v = two_view_vectors(R, t, d0x, d0y, d1x, d1y);
    TwoViewEpipolar q;
    q.a0 = v.a0; q.a1 = v.a1; q.a2 = v.a2; q.c0 = v.c0; q.c1 = v.c1; q.c2 = v.c2; q.e0 = v.e0; q.e1 = v.e1; q.e2 = v.e2;
    q.r = ((v.e0 * v.a0) + (v.e1 * v.a1)) + (v.e2 * v.a2);
    const double l0 = ((t[1] * v.a2) - (t[2] * v.a1)) / fx, l1 = ((t[2] * v.a0) - (t[0] * v.a2)) / fy;
    const double m0 = (((R[0] * v.e0) + (R[3] * v.e1)) + (R[6] * v.e2)) / fx;
    const double m1 = (((R[1] * v.e0) + (R[4] * v.e1)) + (R[7] * v.e2)) / fy;
    q.g = (((l0 * l0) + (l1 * l1)) + (m0 * m0)) + (m1 * m1);
    return q;
}

// BASIS of "pose refinement": an orthonormal basis b1, b2 of the plane across the unit vector t.  b1 = (e_i x t) / |e_i x t| for the
// entry i of t smallest in magnitude (ties to the lowest index), b2 = t x b1.
__device__ __forceinline__ void two_view_tangent_basis(const double* t, double* b1, double* b2) {
    const double m0 = fabs(t[0]), m1 = fabs(t[1]), m2 = fabs(t[2]);
    int i = 0;
    double least = m0;
    if (m1 < least) { i = 1; least = m1; }
    if (m2 < least) i = 2;
    // the two entries of e_i x t that are not zero: (p, q) with e_0 x t = (0, -t2, t1), e_1 x t = (t2, 0, -t0), e_2 x t = (-t1, t0, 0)
    const double p = i == 0 ? t[2] : (i == 1 ? t[2] : t[1]), q = i == 0 ? t[1] : t[0];
    const double nrm = sqrt((p * p) + (q * q));
    b1[0] = i == 0 ? 0.0 : (i == 1 ? p / nrm : (-p) / nrm);
    b1[1] = i == 0 ? (-p) / nrm : (i == 1 ? 0.0 : q / nrm);
    b1[2] = i == 0 ? q / nrm : (i == 1 ? (-q) / nrm : 0.0);
    b2[0] = (t[1] * b1[2]) - (t[2] * b1[1]);
    b2[1] = (t[2] * b1[0]) - (t[0] * b1[2]);
    b2[2] = (t[0] * b1[1]) - (t[1] * b1[0]);
}
