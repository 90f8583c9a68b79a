// pwc_fundamental.hip -- epipolar camera motion: the fundamental matrix that explains most of a flow field, by the reweighted
// normalised eight-point fit, and the Sampson distance of every pixel to it, wholly on the device (gfx950; C ABI and every
// operation's order in include/pwc_hip.h, "epipolar motion"; launch plan and figures in DESIGN.md 27).
//
//   pwc_fundamental_fit_workspace_bytes   8 (N parts 36 + N 9) + 4 N parts, rounded up to 8: the parts' sums and counts, F^ per image
//   pwc_fundamental_fit_f64               matrices (N, 3, 3) doubles, ok (N) bytes, count (N) int32, weight_sum (N), eigen (N, 2) and
//                                         epipole (N, 3) doubles
//   pwc_epipolar_residual_f32             distance (N, H, W) floats and inlier (N, H, W) bytes
//
// The pass structure is robust_fit.h's: iters + 1 passes of two launches each on the caller's stream, the device reading
// what the pass before wrote.
//   sums    grid (parts, N), loss_common.h's partition.  A known pixel (flow_record.h's rule) has xh, yh, x', y' as the homography
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
// any channel stride >= 2, loaded as flow_record.h loads them.  The Sampson terms r and g are two_view.h's, the one order both the
// weights and the residual use.
#include "motion_jacobi.h"
#include "robust_fit.h"
#include "two_view.h"

#pragma clang fp contract(off)

#define FUNDAMENTAL_EIGEN_FLOOR 1e-9
#define FUNDAMENTAL_SUMS 36
#define FUNDAMENTAL_MIN_COUNT 8

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
    const PwcFitNorm t = pwc_fit_norm(a.H, a.W);
    const double s = t.s, c2 = a.scale * a.scale, s2 = s * s;
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
        pwc_flow_load2<VEC>(a.flow + (img + i) * a.cs, fu, fv);
        if (!pwc_flow_known(fu, fv)) continue;
        cnt += 1;                                                          // (a known pixel, in the pass or left out of it)
        double xh, yh;
        pwc_fit_normalise(t, i, a.W, xh, yh);
        const double xp = xh + ((double)fu / s), yp = yh + ((double)fv / s);
        double w = 1.0;
        if (!a.first) {
            double r, g;
            two_view_sampson(f, xh, yh, xp, yp, r, g);
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
    pwc_fit_write_part<FUNDAMENTAL_SUMS>(sum, cnt, n, a.part, a.part_n);
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
    int cnt;
    pwc_fit_gather<FUNDAMENTAL_SUMS>(a.part, a.part_n, n, a.parts, S, cnt);
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
        for (int j = 0; j < 9; ++j) good = good && pwc_finite(F[j]);
        good = good && pwc_finite(v[0]) && pwc_finite(v[1]) && pwc_finite(v[2]) && pwc_finite(eig[0]) &&
               pwc_finite(eig[1]);
    }
    const bool fit = good;                                                 // what the later passes see
    if (a.last) {
        const PwcFitNorm t = pwc_fit_norm(a.H, a.W);
        const double cx = t.cx, cy = t.cy, s = t.s;
        // F^ T, row by row; then T^T (F^ T) the same way down the columns
        double r[3][3], m[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) pwc_fit_row_times_t(t, F[3 * i], F[3 * i + 1], F[3 * i + 2], r[i][0], r[i][1], r[i][2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) pwc_fit_row_times_t(t, r[0][j], r[1][j], r[2][j], m[j], m[3 + j], m[6 + j]);
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
        for (int j = 0; j < 9; ++j) { m[j] = flip ? -m[j] : m[j]; good = good && pwc_finite(m[j]); }
        good = good && pwc_finite(e[0]) && pwc_finite(e[1]) && pwc_finite(e[2]);
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
        float d = PWC_FLOW_SENTINEL;
        uint8_t in = 0;
        if (!zero && !(a.valid && !a.valid[p])) {
            float fu, fv;
            pwc_flow_load2<VEC>(a.flow + (size_t)p * a.cs, fu, fv);
            if (pwc_flow_known(fu, fv)) {
                const double x = (double)q.x, y = (double)q.y;
                double r, g;
                two_view_sampson(f, x, y, x + (double)fu, y + (double)fv, r, g);
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
extern "C" size_t pwc_fundamental_fit_workspace_bytes(int N, int H, int W) {
    return pwc_fit_workspace_bytes(N, H, W, FUNDAMENTAL_SUMS, 9);
}

extern "C" int pwc_fundamental_fit_f64(const float* flows, int flow_cs, const uint8_t* valid, int N, int H, int W, int iters,
                                       double scale, void* workspace, size_t workspace_bytes, double* matrices, uint8_t* ok,
                                       int32_t* count, double* weight_sum, double* eigen, double* epipole, pwc_stream_t stream) {
    if (!matrices || !ok || !count || !weight_sum || !eigen || !epipole) return PWC_EINVAL;
    const int rc = pwc_fit_check(flows, flow_cs, N, H, W, iters, scale, workspace, workspace_bytes,
                                 pwc_fundamental_fit_workspace_bytes(N, H, W),
                                 pwc_off(matrices, 7u) || pwc_off(weight_sum, 7u) || pwc_off(eigen, 7u) || pwc_off(epipole, 7u) ||
                                     pwc_off(count, 3u));
    if (rc != PWC_OK) return rc;
    const int parts = (int)pwc_loss_parts(H, W);
    FundamentalFitArgs a = {};
    a.flow = flows; a.valid = valid;
    pwc_fit_carve(workspace, N, parts, FUNDAMENTAL_SUMS, 9, a.part, a.param, a.part_n);
    a.matrices = matrices; a.ok = ok; a.count = count; a.weight_sum = weight_sum; a.eigen = eigen; a.epipole = epipole;
    a.scale = scale; a.cs = flow_cs; a.N = N; a.H = H; a.W = W; a.parts = parts;
    pwc_fit_passes<fundamental_sums_kernel<true>, fundamental_sums_kernel<false>, fundamental_solve_kernel>(
        a, iters, pwc_flow_vec(flow_cs, {flows}), (hipStream_t)stream);
    return pwc_launch_status();
}

extern "C" int pwc_epipolar_residual_f32(const float* flows, int flow_cs, const uint8_t* valid, const double* matrices, int N, int H,
                                         int W, double threshold, float* distance, uint8_t* inlier, pwc_stream_t stream) {
    if (!flows || !matrices || !distance || !inlier) return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || flow_cs < 2 || !(threshold >= 0.0)) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (pwc_off(flows, 3u) || pwc_off(distance, 3u) || pwc_off(matrices, 7u)) return PWC_EALIGN;
    EpipolarResidualArgs a = {};
    a.flow = flows; a.valid = valid; a.matrices = matrices; a.distance = distance; a.inlier = inlier;
    a.threshold = threshold; a.cs = flow_cs; a.N = N; a.H = H; a.W = W;
    const bool vec = pwc_flow_vec(flow_cs, {flows});
    const dim3 grid = pwc_loss_grad_blocks(N, H, W);
    const hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(epipolar_residual_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(epipolar_residual_kernel<false>, grid, dim3(256), 0, s, a);
    return pwc_launch_status();
}
