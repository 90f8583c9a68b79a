// pwc_homography.hip -- projective camera motion: the homography that explains most of a flow field, by the reweighted normalised
// direct linear transform, wholly on the device (gfx950; C ABI and every operation's order in include/pwc_hip.h, "projective
// motion"; launch plan and figures in DESIGN.md 26).
//
//   pwc_homography_fit_workspace_bytes   8 (N parts 23 + N 8) + 4 N parts, rounded up to 8: the parts' sums and counts, the parameters
//   pwc_homography_fit_f64               matrices (N, 3, 3) doubles, ok (N) bytes, count (N) int32, weight_sum (N) doubles
//
// The pass structure is pwc_motion_fit_f64's: iters + 1 passes of two launches each on the caller's stream, the device reading what
// the pass before wrote.
//   sums    grid (parts, N), loss_common.h's partition.  A known pixel (pwc_motion.hip's rule) has xh, yh as there and the target
//           x' = xh + u / s, y' = yh + v / s.  Its two rows are g0 xh + g1 yh + g2 - x' (g6 xh + g7 yh) = x' and the same in
//           g3 g4 g5 and y'.  The normal equations have the blocks [[P 0 -Qx] [0 P -Qy] [. . R]] and need 23 sums, not 36 + 8 + 1:
//           b = w {1, xh, yh, xh xh, xh yh, yh yh} (6), b x' (6), b y' (6) and b[1 .. 5] (x' x' + y' y') (5).  23 x 256 doubles are
//           47 KB of LDS in pwc_block_tree_sum_f64.
//   solve   a lane per image adds the parts in index order, assembles the lower triangle in the order (g2 g0 g1 g5 g3 g4 g6 g7) --
//           the constant first, as the affine fit has it -- and runs motion_ldlt<8, 1> with the pivot rule d > 1e-9 sum(w).
//           Degenerate is final.  The last pass writes M = T^-1 G T entry by entry, divided by its [2][2] entry.
// Every value is an IEEE double + - x / or a comparison in the order written here -- no fused multiply-add is formed anywhere in
// this file (the pragma below), no library function is called -- so tests/homography_ref.py restates it in numpy bit for bit.
// No atomic, no host synchronisation, no process-wide state.  Flows at any channel stride >= 2, loaded as pwc_motion.hip loads them.
#include "loss_common.h"
#include "motion_ldlt.h"

#pragma clang fp contract(off)

#define HOMOGRAPHY_PIVOT 1e-9
#define HOMOGRAPHY_SUMS 23
#define HOMOGRAPHY_MIN_COUNT 4

template <bool VEC>
__device__ __forceinline__ void homography_load2(const float* p, float& a, float& b) {
    if (VEC) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(p);
        a = v[0]; b = v[1];
    } else {
        a = p[0]; b = p[1];
    }
}

__device__ __forceinline__ bool homography_known(float a, float b) { return fabsf(a) <= 1e9f && fabsf(b) <= 1e9f; }
__device__ __forceinline__ bool homography_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (false for a NaN)

struct HomographyFitArgs {
    const float* flow;        // [N][H][W] records of cs floats, 2 used
    const uint8_t* valid;     // [N][H][W], null: every pixel
    double* part;             // [N][parts][23]
    double* param;            // [N][8]: g0 .. g7 of [[g0 g1 g2] [g3 g4 g5] [g6 g7 1]], normalised coordinates
    int* part_n;              // [N][parts]
    double* matrices;         // [N][9]
    uint8_t* ok;              // [N]
    int* count;               // [N]
    double* weight_sum;       // [N]
    double scale;
    int cs, N, H, W, parts;
    int first, last;          // pass 0: w = 1; the last pass writes the matrices
};

template <bool VEC>
__global__ __launch_bounds__(256) void homography_sums_kernel(const HomographyFitArgs a) {
    const int n = blockIdx.y, hw = a.H * a.W;
    const size_t img = (size_t)n * hw;
    const double cx = (double)(a.W - 1) / 2.0, cy = (double)(a.H - 1) / 2.0, s = (double)max(a.H, a.W) / 2.0;
    const double c2 = a.scale * a.scale;
    double g[8] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    if (!a.first) {
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = a.param[(size_t)n * 8 + j];
    }
    double sum[HOMOGRAPHY_SUMS];
#pragma unroll
    for (int j = 0; j < HOMOGRAPHY_SUMS; ++j) sum[j] = 0.0;
    int cnt = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += (int)gridDim.x * 256) {
        if (a.valid && !a.valid[img + i]) continue;
        float fu, fv;
        homography_load2<VEC>(a.flow + (img + i) * a.cs, fu, fv);
        if (!homography_known(fu, fv)) continue;
        cnt += 1;                                                          // (a known pixel, in the pass or left out of it)
        const double xh = ((double)(i % a.W) - cx) / s, yh = ((double)(i / a.W) - cy) / s;
        const double xp = xh + ((double)fu / s), yp = yh + ((double)fv / s);
        double w = 1.0;
        if (!a.first) {
            const double D = ((g[6] * xh) + (g[7] * yh)) + 1.0;
            if (!(D > 0.0)) continue;                                      // behind the horizon of the pass before: left out
            const double rx = (((((g[0] * xh) + (g[1] * yh)) + g[2]) / D) - xp) * s;
            const double ry = (((((g[3] * xh) + (g[4] * yh)) + g[5]) / D) - yp) * s;
            w = (1.0 / (1.0 + (((rx * rx) + (ry * ry)) / c2))) / (D * D);
        }
        const double wx = w * xh, wy = w * yh;
        double b[6];
        b[0] = w; b[1] = wx; b[2] = wy; b[3] = wx * xh; b[4] = wx * yh; b[5] = wy * yh;
        const double q = (xp * xp) + (yp * yp);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            sum[j] = sum[j] + b[j];
            sum[6 + j] = sum[6 + j] + (b[j] * xp);
            sum[12 + j] = sum[12 + j] + (b[j] * yp);
        }
#pragma unroll
        for (int j = 1; j < 6; ++j) sum[17 + j] = sum[17 + j] + (b[j] * q);
    }
    pwc_block_tree_sum_f64<HOMOGRAPHY_SUMS, 1>(sum, &cnt);
    if (threadIdx.x == 0) {
        const size_t o = (size_t)n * gridDim.x + blockIdx.x;
#pragma unroll
        for (int j = 0; j < HOMOGRAPHY_SUMS; ++j) a.part[o * HOMOGRAPHY_SUMS + j] = sum[j];
        a.part_n[o] = cnt;
    }
}

// One lane per image.
__global__ __launch_bounds__(64) void homography_solve_kernel(const HomographyFitArgs a) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= a.N) return;
    double S[HOMOGRAPHY_SUMS];
#pragma unroll
    for (int j = 0; j < HOMOGRAPHY_SUMS; ++j) S[j] = 0.0;
    int cnt = 0;
    for (int i = 0; i < a.parts; ++i) {
        const size_t o = (size_t)n * a.parts + i;
#pragma unroll
        for (int j = 0; j < HOMOGRAPHY_SUMS; ++j) S[j] = S[j] + a.part[o * HOMOGRAPHY_SUMS + j];
        cnt += a.part_n[o];
    }
    const double tol = HOMOGRAPHY_PIVOT * S[0];
    double g[8] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    bool good = (a.first || a.ok[n] != 0) && cnt >= HOMOGRAPHY_MIN_COUNT;
    if (good) {
        // unknowns in the order (g2 g0 g1 g5 g3 g4 g6 g7); S: 0 w, 1 x, 2 y, 3 xx, 4 xy, 5 yy; + 6 times x'; + 12 times y'; 18 .. 22: x y xx xy yy times q
        const double A[8][8] = {{S[0], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
                                {S[1], S[3], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
                                {S[2], S[4], S[5], 0.0, 0.0, 0.0, 0.0, 0.0},
                                {0.0, 0.0, 0.0, S[0], 0.0, 0.0, 0.0, 0.0},
                                {0.0, 0.0, 0.0, S[1], S[3], 0.0, 0.0, 0.0},
                                {0.0, 0.0, 0.0, S[2], S[4], S[5], 0.0, 0.0},
                                {-S[7], -S[9], -S[10], -S[13], -S[15], -S[16], S[20], 0.0},
                                {-S[8], -S[10], -S[11], -S[14], -S[16], -S[17], S[21], S[22]}};
        double r[1][8] = {{S[6], S[7], S[8], S[12], S[13], S[14], -S[18], -S[19]}};
        good = motion_ldlt<8, 1>(A, r, tol);
        if (good) {                                                        // (else g stays the identity)
            g[2] = r[0][0]; g[0] = r[0][1]; g[1] = r[0][2]; g[5] = r[0][3]; g[3] = r[0][4]; g[4] = r[0][5]; g[6] = r[0][6]; g[7] = r[0][7];
        }
    }
    bool fit = good;                                                       // what the later passes see
    if (a.last) {
        const double cx = (double)(a.W - 1) / 2.0, cy = (double)(a.H - 1) / 2.0, s = (double)max(a.H, a.W) / 2.0;
        // G T, row by row: (h0 / s, h1 / s, h2 - ((h0 cx) + (h1 cy)) / s); the last row of G is g6 g7 1
        const double a00 = g[0] / s, a01 = g[1] / s, a02 = g[2] - (((g[0] * cx) + (g[1] * cy)) / s);
        const double a10 = g[3] / s, a11 = g[4] / s, a12 = g[5] - (((g[3] * cx) + (g[4] * cy)) / s);
        const double a20 = g[6] / s, a21 = g[7] / s, a22 = 1.0 - (((g[6] * cx) + (g[7] * cy)) / s);
        // T^-1 (G T): rows (s r0) + (cx r2), (s r1) + (cy r2), r2
        double e[9];
        e[0] = (s * a00) + (cx * a20); e[1] = (s * a01) + (cx * a21); e[2] = (s * a02) + (cx * a22);
        e[3] = (s * a10) + (cy * a20); e[4] = (s * a11) + (cy * a21); e[5] = (s * a12) + (cy * a22);
        e[6] = a20; e[7] = a21; e[8] = a22;
        good = good && e[8] > 0.0;
        double m[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) { m[j] = e[j] / e[8]; good = good && homography_finite(m[j]); }
        // the horizon stays outside the frame: D > 0 at the four corners
        const double xr = (double)(a.W - 1), yb = (double)(a.H - 1);
        good = good && (((m[6] * 0.0) + (m[7] * 0.0)) + 1.0) > 0.0 && (((m[6] * xr) + (m[7] * 0.0)) + 1.0) > 0.0 &&
               (((m[6] * 0.0) + (m[7] * yb)) + 1.0) > 0.0 && (((m[6] * xr) + (m[7] * yb)) + 1.0) > 0.0;
        double* out = a.matrices + (size_t)n * 9;
#pragma unroll
        for (int j = 0; j < 9; ++j) out[j] = good ? m[j] : ((j & 3) == 0 ? 1.0 : 0.0);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) a.param[(size_t)n * 8 + j] = g[j];
    a.ok[n] = (a.last ? good : fit) ? 1 : 0;
    a.count[n] = cnt;
    a.weight_sum[n] = S[0];
}

// ---------------------------------------------------------------- host
static inline bool homography_off(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

extern "C" size_t pwc_homography_fit_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || !pwc_loss_in_range(N, H, W)) return 0;
    const size_t cells = (size_t)N * pwc_loss_parts(H, W);
    return 8 * (cells * HOMOGRAPHY_SUMS + (size_t)N * 8) + ((4 * cells + 7) & ~(size_t)7);
}

extern "C" int pwc_homography_fit_f64(const float* flows, int flow_cs, const uint8_t* valid, int N, int H, int W, int iters, double scale,
                                      void* workspace, size_t workspace_bytes, double* matrices, uint8_t* ok, int32_t* count,
                                      double* weight_sum, pwc_stream_t stream) {
    if (!flows || !workspace || !matrices || !ok || !count || !weight_sum) return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || iters < 0 || iters > PWC_MOTION_MAX_ITERS || !(scale > 0.0) || flow_cs < 2) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (homography_off(flows, 3u) || homography_off(workspace, 7u) || homography_off(matrices, 7u) || homography_off(weight_sum, 7u) ||
        homography_off(count, 3u))
        return PWC_EALIGN;
    if (workspace_bytes < pwc_homography_fit_workspace_bytes(N, H, W)) return PWC_EINVAL;
    const int parts = (int)pwc_loss_parts(H, W);
    const size_t cells = (size_t)N * parts;
    HomographyFitArgs a = {};
    a.flow = flows; a.valid = valid;
    a.part = reinterpret_cast<double*>(workspace);
    a.param = a.part + cells * HOMOGRAPHY_SUMS;
    a.part_n = reinterpret_cast<int*>(a.param + (size_t)N * 8);
    a.matrices = matrices; a.ok = ok; a.count = count; a.weight_sum = weight_sum;
    a.scale = scale; a.cs = flow_cs; a.N = N; a.H = H; a.W = W; a.parts = parts;
    const bool vec = !(flow_cs & 1) && !homography_off(flows, 7u);
    const hipStream_t s = (hipStream_t)stream;
    for (int pass = 0; pass <= iters; ++pass) {
        a.first = pass == 0 ? 1 : 0;
        a.last = pass == iters ? 1 : 0;
        if (vec) hipLaunchKernelGGL(homography_sums_kernel<true>, dim3(parts, N), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(homography_sums_kernel<false>, dim3(parts, N), dim3(256), 0, s, a);
        hipLaunchKernelGGL(homography_solve_kernel, dim3((N + 63) / 64), dim3(64), 0, s, a);
    }
    return pwc_launch_status();
}
