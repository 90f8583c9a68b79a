// two_view.h -- the per-pixel core that the cheirality vote and the depth kernel of pwc_pose.hip share, so that its order of
// operations is written once (include/pwc_hip.h, "relative pose and depth"; tests/pose_ref.py restates it in numpy): the flow
// loads and the known-pixel rule of pwc_fundamental.hip, SAMPSON as that file has it, the ray of a pixel and the triangulation of
// a pixel pair under a candidate pose.
#pragma once
#include "pwc_common.h"

#pragma clang fp contract(off)

template <bool VEC>
__device__ __forceinline__ void two_view_load2(const float* p, float& a, float& b) {
    if (VEC) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(p);
        a = v[0]; b = v[1];
    } else {
        a = p[0]; b = p[1];
    }
}

__device__ __forceinline__ bool two_view_known(float a, float b) { return fabsf(a) <= 1e9f && fabsf(b) <= 1e9f; }
__device__ __forceinline__ bool two_view_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (false for a NaN)

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
    return two_view_finite(k[0]) && two_view_finite(k[1]) && two_view_finite(k[2]) && two_view_finite(k[3]) && k[0] > 0.0 && k[1] > 0.0;
}

// What a pixel pair says under the pose (R, t), X' = R X + t.  d0 = K^-1 p = (d0x, d0y, 1) and d1 = K^-1 p' = (d1x, d1y, 1) are
// the rays; a = R d0 is the first ray in the second camera's frame.  Z1 d1 = Z0 a + t, crossed with d1: Z0 (d1 x a) = -(d1 x t).
struct TwoViewPoint {
    double a0, a1, a2;        // R d0
    double den;               // |d1 x a|^2
    double z0, z1;            // the depths in the first and the second camera, in baselines
};

__device__ __forceinline__ TwoViewPoint two_view_triangulate(const double* R, const double* t, double d0x, double d0y, double d1x,
                                                             double d1y) {
    TwoViewPoint p;
    p.a0 = ((R[0] * d0x) + (R[1] * d0y)) + R[2];
    p.a1 = ((R[3] * d0x) + (R[4] * d0y)) + R[5];
    p.a2 = ((R[6] * d0x) + (R[7] * d0y)) + R[8];
    const double c0 = (d1y * p.a2) - p.a1, c1 = p.a0 - (d1x * p.a2), c2 = (d1x * p.a1) - (d1y * p.a0);
    const double e0 = (d1y * t[2]) - t[1], e1 = t[0] - (d1x * t[2]), e2 = (d1x * t[1]) - (d1y * t[0]);
    p.den = ((c0 * c0) + (c1 * c1)) + (c2 * c2);
    p.z0 = -(((c0 * e0) + (c1 * e1)) + (c2 * e2)) / p.den;
    p.z1 = (p.z0 * p.a2) + t[2];
    return p;
}
