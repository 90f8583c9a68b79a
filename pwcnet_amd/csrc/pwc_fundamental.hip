// pwc_fundamental.hip -- epipolar camera motion: the fundamental matrix that explains most of a flow field, by the reweighted
// normalised eight-point fit, and the Sampson distance of every pixel to it, wholly on the device (gfx950; C ABI and every
// operation's order in include/pwc_hip.h, "epipolar motion"; launch plan and figures in DESIGN.md 27).
//
//   pwc_fundamental_fit_workspace_bytes   8 (N parts 36 + N 9) + 4 N parts, rounded up to 8: the parts' sums and counts, F^ per image
//   pwc_fundamental_fit_f64               matrices (N, 3, 3) doubles, ok (N) bytes, count (N) int32, weight_sum (N), eigen (N, 2) and
//                                         epipole (N, 3) doubles
//   pwc_epipolar_residual_f32             distance (N, H, W) floats and inlier (N, H, W) bytes
//
// The pass structure is pwc_homography_fit_f64's: iters + 1 passes of two launches each on the caller's stream, the device reading
// what the pass before wrote.
//   sums    grid (parts, N), loss_common.h's partition.  A known pixel (pwc_motion.hip's rule) has xh, yh, x', y' as the homography
//           fit has them and contributes w a a^T, a = (x' xh, x' yh, x', y' xh, y' yh, y', xh, yh, 1).  The 45 entries of the lower
//           triangle are 36 distinct monomials, {1, x', y', x'x', x'y', y'y'} x {1, xh, yh, xh xh, xh yh, yh yh}: 36 sums, ONE tree
//           round of pwc_block_tree_sum_f64<36, 1> -- 36 x 256 doubles and 256 ints are 74,752 B of LDS (gfx950 has 160 KB a CU).
//   solve   a lane per image adds the parts in index order, fills the 9 x 9 matrix from the 36 sums and runs motion_jacobi<9>; f is
//           the eigenvector of the smallest eigenvalue.  Rank 2: v, the eigenvector of the smallest eigenvalue of F^^T F^
//           (motion_jacobi<3>), and F^ <- F^ - (F^ v) v^T.  Degenerate is final.  The last pass writes F = T^T F^ T entry by entry,
//           over its Frobenius norm, the entry of largest magnitude positive, and the epipole T^-1 v.
// Every value is an IEEE double + - x / sqrt or a comparison in the order written here -- no fused multiply-add is formed anywhere
// in this file (the pragma below), sqrt on doubles (correctly rounded, as pwc_flowvis.hip relies on) is the only library call -- so
// tests/fundamental_ref.py restates it in numpy bit for bit.  No atomic, no host synchronisation, no process-wide state.  Flows at
// any channel stride >= 2, loaded as pwc_motion.hip loads them.
#include "loss_common.h"
#include "motion_jacobi.h"

#pragma clang fp contract(off)

#define FUNDAMENTAL_EIGEN_FLOOR 1e-9
#define FUNDAMENTAL_SUMS 36
#define FUNDAMENTAL_MIN_COUNT 8
#define FUNDAMENTAL_SENTINEL 1e10f
#define FUNDAMENTAL_MAX_BLOCKS 4096

template <bool VEC>
__device__ __forceinline__ void fundamental_load2(const float* p, float& a, float& b) {
    if (VEC) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(p);
        a = v[0]; b = v[1];
    } else {
        a = p[0]; b = p[1];
    }
}

__device__ __forceinline__ bool fundamental_known(float a, float b) { return fabsf(a) <= 1e9f && fabsf(b) <= 1e9f; }
__device__ __forceinline__ bool fundamental_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (false for a NaN)

// r = p'^T F p and g = l0^2 + l1^2 + l'0^2 + l'1^2 with l = F p, l' = F^T p': the one order both the weights and the residual use.
__device__ __forceinline__ void fundamental_sampson(const double* f, double x, double y, double xp, double yp, double& r, double& g) {
    const double l0 = ((f[0] * x) + (f[1] * y)) + f[2];
    const double l1 = ((f[3] * x) + (f[4] * y)) + f[5];
    const double l2 = ((f[6] * x) + (f[7] * y)) + f[8];
    r = ((xp * l0) + (yp * l1)) + l2;
    const double m0 = ((f[0] * xp) + (f[3] * yp)) + f[6];
    const double m1 = ((f[1] * xp) + (f[4] * yp)) + f[7];
    g = (((l0 * l0) + (l1 * l1)) + (m0 * m0)) + (m1 * m1);
}

struct FundamentalFitArgs {
    const float* flow;        // [N][H][W] records of cs floats, 2 used
    const uint8_t* valid;     // [N][H][W], null: every pixel
    double* part;             // [N][parts][36]
    double* param;            // [N][9]: F^ of the pass before, rank 2, normalised coordinates; zeros where degenerate
    int* part_n;              // [N][parts]
    double* matrices;         // [N][9]
    uint8_t* ok;              // [N]
    int* count;               // [N]
    double* weight_sum;       // [N]
    double* eigen;            // [N][2]
    double* epipole;          // [N][3]
    double scale;
    int cs, N, H, W, parts;
    int first, last;          // pass 0: w = 1; the last pass writes the matrices
};

template <bool VEC>
__global__ __launch_bounds__(256) void fundamental_sums_kernel(const FundamentalFitArgs a) {
    const int n = blockIdx.y, hw = a.H * a.W;
    const size_t img = (size_t)n * hw;
    const double cx = (double)(a.W - 1) / 2.0, cy = (double)(a.H - 1) / 2.0, s = (double)max(a.H, a.W) / 2.0;
    const double c2 = a.scale * a.scale, s2 = s * s;
    double f[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) f[j] = a.first ? 0.0 : a.param[(size_t)n * 9 + j];
    double sum[FUNDAMENTAL_SUMS];
#pragma unroll
    for (int j = 0; j < FUNDAMENTAL_SUMS; ++j) sum[j] = 0.0;
    int cnt = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += (int)gridDim.x * 256) {
        if (a.valid && !a.valid[img + i]) continue;
        float fu, fv;
        fundamental_load2<VEC>(a.flow + (img + i) * a.cs, fu, fv);
        if (!fundamental_known(fu, fv)) continue;
        cnt += 1;                                                          // (a known pixel, in the pass or left out of it)
        const double xh = ((double)(i % a.W) - cx) / s, yh = ((double)(i / a.W) - cy) / s;
        const double xp = xh + ((double)fu / s), yp = yh + ((double)fv / s);
        double w = 1.0;
        if (!a.first) {
            double r, g;
            fundamental_sampson(f, xh, yh, xp, yp, r, g);
            if (!(g > 0.0)) continue;                                      // no gradient under the F^ of the pass before: left out
            const double d2 = ((r * r) / g) * s2;
            w = (1.0 / (1.0 + (d2 / c2))) / g;
        }
        const double wx = w * xh, wy = w * yh;
        double b[6];
        b[0] = w; b[1] = wx; b[2] = wy; b[3] = wx * xh; b[4] = wx * yh; b[5] = wy * yh;
        const double pa[5] = {xp, yp, xp * xp, xp * yp, yp * yp};
#pragma unroll
        for (int j = 0; j < 6; ++j) sum[j] = sum[j] + b[j];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
#pragma unroll
            for (int j = 0; j < 6; ++j) sum[6 * (m + 1) + j] = sum[6 * (m + 1) + j] + (b[j] * pa[m]);
        }
    }
    pwc_block_tree_sum_f64<FUNDAMENTAL_SUMS, 1>(sum, &cnt);
    if (threadIdx.x == 0) {
        const size_t o = (size_t)n * gridDim.x + blockIdx.x;
#pragma unroll
        for (int j = 0; j < FUNDAMENTAL_SUMS; ++j) a.part[o * FUNDAMENTAL_SUMS + j] = sum[j];
        a.part_n[o] = cnt;
    }
}

// a_k = P[pk] Q[qk] with P = (1, x', y'), Q = (1, xh, yh); the monomial of a pair of P's (or of Q's) among (1, x, y, x x, x y, y y)
__device__ __forceinline__ constexpr int fundamental_pk(int k) { return k < 3 ? 1 : (k < 6 ? 2 : 0); }
__device__ __forceinline__ constexpr int fundamental_qk(int k) { return k % 3 == 2 ? 0 : k % 3 + 1; }
__device__ __forceinline__ constexpr int fundamental_mono(int i, int j) {
    return i == 0 ? j : (j == 0 ? i : (i == 1 && j == 1 ? 3 : (i == 2 && j == 2 ? 5 : 4)));
}

// One lane per image.
__global__ __launch_bounds__(64) void fundamental_solve_kernel(const FundamentalFitArgs a) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= a.N) return;
    double S[FUNDAMENTAL_SUMS];
#pragma unroll
    for (int j = 0; j < FUNDAMENTAL_SUMS; ++j) S[j] = 0.0;
    int cnt = 0;
    for (int i = 0; i < a.parts; ++i) {
        const size_t o = (size_t)n * a.parts + i;
#pragma unroll
        for (int j = 0; j < FUNDAMENTAL_SUMS; ++j) S[j] = S[j] + a.part[o * FUNDAMENTAL_SUMS + j];
        cnt += a.part_n[o];
    }
    const bool before = a.first || a.ok[n] != 0;                           // not degenerate in an earlier pass
    bool good = before && cnt >= FUNDAMENTAL_MIN_COUNT;
    double F[9], v[3] = {0.0, 0.0, 0.0}, eig[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 9; ++j) F[j] = 0.0;
    if (good) {
        double A[9][9], V[9][9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
#pragma unroll
            for (int l = k; l < 9; ++l)
                A[k][l] = S[6 * fundamental_mono(fundamental_pk(k), fundamental_pk(l)) + fundamental_mono(fundamental_qk(k), fundamental_qk(l))];
        }
        double tr = A[0][0];
#pragma unroll
        for (int k = 1; k < 9; ++k) tr = tr + A[k][k];
        motion_jacobi<9>(A, V);
        int j0, j1;
        double other[9];
        const double e0 = motion_jacobi_smallest<9>(A, V, -1, F, j0);
        const double e1 = motion_jacobi_smallest<9>(A, V, j0, other, j1);
        eig[0] = e0 / tr; eig[1] = e1 / tr;
        good = e1 > (FUNDAMENTAL_EIGEN_FLOOR * tr);
        // rank 2: the eigenvector of the smallest eigenvalue of F^T F
        double B[3][3], U[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = i; j < 3; ++j) B[i][j] = ((F[i] * F[j]) + (F[3 + i] * F[3 + j])) + (F[6 + i] * F[6 + j]);
        }
        motion_jacobi<3>(B, U);
        int jv;
        motion_jacobi_smallest<3>(B, U, -1, v, jv);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double ui = ((F[3 * i] * v[0]) + (F[3 * i + 1] * v[1])) + (F[3 * i + 2] * v[2]);
#pragma unroll
            for (int j = 0; j < 3; ++j) F[3 * i + j] = F[3 * i + j] - (ui * v[j]);
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) good = good && fundamental_finite(F[j]);
        good = good && fundamental_finite(v[0]) && fundamental_finite(v[1]) && fundamental_finite(v[2]) && fundamental_finite(eig[0]) &&
               fundamental_finite(eig[1]);
    }
    const bool fit = good;                                                 // what the later passes see
    if (a.last) {
        const double cx = (double)(a.W - 1) / 2.0, cy = (double)(a.H - 1) / 2.0, s = (double)max(a.H, a.W) / 2.0;
        // F^ T, row by row: (h0 / s, h1 / s, h2 - ((h0 cx) + (h1 cy)) / s); then T^T (F^ T) the same way down the columns
        double r[3][3], m[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            r[i][0] = F[3 * i] / s; r[i][1] = F[3 * i + 1] / s;
            r[i][2] = F[3 * i + 2] - (((F[3 * i] * cx) + (F[3 * i + 1] * cy)) / s);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            m[j] = r[0][j] / s; m[3 + j] = r[1][j] / s;
            m[6 + j] = r[2][j] - (((r[0][j] * cx) + (r[1][j] * cy)) / s);
        }
        double q = m[0] * m[0];
#pragma unroll
        for (int j = 1; j < 9; ++j) q = q + (m[j] * m[j]);
        const double nrm = sqrt(q);
        double big = 0.0, sign = 0.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            m[j] = m[j] / nrm;
            if (j == 0 || fabs(m[j]) > big) { big = fabs(m[j]); sign = m[j]; }
        }
        const bool flip = sign < 0.0;
        const double e[3] = {(s * v[0]) + (cx * v[2]), (s * v[1]) + (cy * v[2]), v[2]};
#pragma unroll
        for (int j = 0; j < 9; ++j) { m[j] = flip ? -m[j] : m[j]; good = good && fundamental_finite(m[j]); }
        good = good && fundamental_finite(e[0]) && fundamental_finite(e[1]) && fundamental_finite(e[2]);
#pragma unroll
        for (int j = 0; j < 9; ++j) a.matrices[(size_t)n * 9 + j] = good ? m[j] : 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) a.epipole[(size_t)n * 3 + j] = good ? e[j] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) a.param[(size_t)n * 9 + j] = fit ? F[j] : 0.0;
    if (before) {                                                          // (else: the figures of the pass that found it degenerate)
        a.eigen[(size_t)n * 2] = eig[0];
        a.eigen[(size_t)n * 2 + 1] = eig[1];
    }
    a.ok[n] = (a.last ? good : fit) ? 1 : 0;
    a.count[n] = cnt;
    a.weight_sum[n] = S[0];
}

// ---------------------------------------------------------------- the residual
struct EpipolarResidualArgs {
    const float* flow;        // [N][H][W] records of cs floats
    const uint8_t* valid;     // [N][H][W], null: every pixel
    const double* matrices;   // [N][9]
    float* distance;          // [N][H][W]
    uint8_t* inlier;          // [N][H][W]
    double threshold;
    int cs, N, H, W;
};

// One lane per pixel of the batch.
template <bool VEC>
__global__ __launch_bounds__(256) void epipolar_residual_kernel(const EpipolarResidualArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel q = pwc_loss_pixel(p, a.H, a.W);
        double f[9];
        bool zero = true;
#pragma unroll
        for (int j = 0; j < 9; ++j) { f[j] = a.matrices[(size_t)q.n * 9 + j]; zero = zero && f[j] == 0.0; }
        float d = FUNDAMENTAL_SENTINEL;
        uint8_t in = 0;
        if (!zero && !(a.valid && !a.valid[p])) {
            float fu, fv;
            fundamental_load2<VEC>(a.flow + (size_t)p * a.cs, fu, fv);
            if (fundamental_known(fu, fv)) {
                const double x = (double)q.x, y = (double)q.y;
                double r, g;
                fundamental_sampson(f, x, y, x + (double)fu, y + (double)fv, r, g);
                if (g > 0.0) {
                    const double dd = fabs(r) / sqrt(g);
                    d = (float)dd;
                    in = dd <= a.threshold ? 1 : 0;
                }
            }
        }
        a.distance[p] = d;
        a.inlier[p] = in;
    }
}

// ---------------------------------------------------------------- host
static inline bool fundamental_off(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

extern "C" size_t pwc_fundamental_fit_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || !pwc_loss_in_range(N, H, W)) return 0;
    const size_t cells = (size_t)N * pwc_loss_parts(H, W);
    return 8 * (cells * FUNDAMENTAL_SUMS + (size_t)N * 9) + ((4 * cells + 7) & ~(size_t)7);
}

extern "C" int pwc_fundamental_fit_f64(const float* flows, int flow_cs, const uint8_t* valid, int N, int H, int W, int iters,
                                       double scale, void* workspace, size_t workspace_bytes, double* matrices, uint8_t* ok,
                                       int32_t* count, double* weight_sum, double* eigen, double* epipole, pwc_stream_t stream) {
    if (!flows || !workspace || !matrices || !ok || !count || !weight_sum || !eigen || !epipole) return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || iters < 0 || iters > PWC_MOTION_MAX_ITERS || !(scale > 0.0) || flow_cs < 2) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (fundamental_off(flows, 3u) || fundamental_off(workspace, 7u) || fundamental_off(matrices, 7u) || fundamental_off(weight_sum, 7u) ||
        fundamental_off(eigen, 7u) || fundamental_off(epipole, 7u) || fundamental_off(count, 3u))
        return PWC_EALIGN;
    if (workspace_bytes < pwc_fundamental_fit_workspace_bytes(N, H, W)) return PWC_EINVAL;
    const int parts = (int)pwc_loss_parts(H, W);
    const size_t cells = (size_t)N * parts;
    FundamentalFitArgs a = {};
    a.flow = flows; a.valid = valid;
    a.part = reinterpret_cast<double*>(workspace);
    a.param = a.part + cells * FUNDAMENTAL_SUMS;
    a.part_n = reinterpret_cast<int*>(a.param + (size_t)N * 9);
    a.matrices = matrices; a.ok = ok; a.count = count; a.weight_sum = weight_sum; a.eigen = eigen; a.epipole = epipole;
    a.scale = scale; a.cs = flow_cs; a.N = N; a.H = H; a.W = W; a.parts = parts;
    const bool vec = !(flow_cs & 1) && !fundamental_off(flows, 7u);
    const hipStream_t s = (hipStream_t)stream;
    for (int pass = 0; pass <= iters; ++pass) {
        a.first = pass == 0 ? 1 : 0;
        a.last = pass == iters ? 1 : 0;
        if (vec) hipLaunchKernelGGL(fundamental_sums_kernel<true>, dim3(parts, N), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(fundamental_sums_kernel<false>, dim3(parts, N), dim3(256), 0, s, a);
        hipLaunchKernelGGL(fundamental_solve_kernel, dim3((N + 63) / 64), dim3(64), 0, s, a);
    }
    return pwc_launch_status();
}

extern "C" int pwc_epipolar_residual_f32(const float* flows, int flow_cs, const uint8_t* valid, const double* matrices, int N, int H,
                                         int W, double threshold, float* distance, uint8_t* inlier, pwc_stream_t stream) {
    if (!flows || !matrices || !distance || !inlier) return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || flow_cs < 2 || !(threshold >= 0.0)) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (fundamental_off(flows, 3u) || fundamental_off(distance, 3u) || fundamental_off(matrices, 7u)) return PWC_EALIGN;
    EpipolarResidualArgs a = {};
    a.flow = flows; a.valid = valid; a.matrices = matrices; a.distance = distance; a.inlier = inlier;
    a.threshold = threshold; a.cs = flow_cs; a.N = N; a.H = H; a.W = W;
    const bool vec = !(flow_cs & 1) && !fundamental_off(flows, 7u);
    const long blocks = ((long)N * H * W + 255) / 256;
    const dim3 grid((unsigned)(blocks > FUNDAMENTAL_MAX_BLOCKS ? FUNDAMENTAL_MAX_BLOCKS : blocks));
    const hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(epipolar_residual_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(epipolar_residual_kernel<false>, grid, dim3(256), 0, s, a);
    return pwc_launch_status();
}
