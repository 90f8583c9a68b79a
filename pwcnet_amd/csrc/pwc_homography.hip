// pwc_homography.hip -- projective camera motion: the homography that explains most of a flow field, by the reweighted normalised
// direct linear transform, wholly on the device (gfx950; C ABI and every operation's order in include/pwc_hip.h, "projective
// motion"; launch plan and figures in DESIGN.md 26).
//
//   pwc_homography_fit_workspace_bytes   8 (N parts 23 + N 8) + 4 N parts, rounded up to 8: the parts' sums and counts, the parameters
//   pwc_homography_fit_f64               matrices (N, 3, 3) doubles, ok (N) bytes, count (N) int32, weight_sum (N) doubles
//
// The pass structure is robust_fit.h's: iters + 1 passes of two launches each on the caller's stream, the device reading what
// the pass before wrote.
//   sums    grid (parts, N), loss_common.h's partition.  A known pixel (flow_record.h's rule) has xh, yh as there and the target
//           x' = xh + u / s, y' = yh + v / s.  Its two rows are g0 xh + g1 yh + g2 - x' (g6 xh + g7 yh) = x' and the same in
//           g3 g4 g5 and y'.  The normal equations have the blocks [[P 0 -Qx] [0 P -Qy] [. . R]] and need 23 sums, not 36 + 8 + 1:
//           b = w {1, xh, yh, xh xh, xh yh, yh yh} (6), b x' (6), b y' (6) and b[1 .. 5] (x' x' + y' y') (5).  23 x 256 doubles are
//           47 KB of LDS in pwc_block_tree_sum_f64.
//   solve   a lane per image adds the parts in index order, assembles the lower triangle in the order (g2 g0 g1 g5 g3 g4 g6 g7) --
//           the constant first, as the affine fit has it -- and runs motion_ldlt<8, 1> with the pivot rule d > 1e-9 sum(w).
//           Degenerate is final.  The last pass writes M = T^-1 G T entry by entry, divided by its [2][2] entry.
// Every value is an IEEE double + - x / or a comparison in the order written here -- no fused multiply-add is formed anywhere in
// this file (the pragma below), no library function is called -- so tests/homography_ref.py restates it in numpy bit for bit.
// No atomic, no host synchronisation, no process-wide state.  Flows at any channel stride >= 2, loaded as flow_record.h loads them.
#include "motion_ldlt.h"
#include "robust_fit.h"

#pragma clang fp contract(off)

#define HOMOGRAPHY_PIVOT 1e-9
#define HOMOGRAPHY_SUMS 23
#define HOMOGRAPHY_MIN_COUNT 4

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
    const PwcFitNorm t = pwc_fit_norm(a.H, a.W);
    const double s = t.s, c2 = a.scale * a.scale;
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
        pwc_flow_load2<VEC>(a.flow + (img + i) * a.cs, fu, fv);
        if (!pwc_flow_known(fu, fv)) continue;
        cnt += 1;                                                          // (a known pixel, in the pass or left out of it)
        double xh, yh;
        pwc_fit_normalise(t, i, a.W, xh, yh);
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
    pwc_fit_write_part<HOMOGRAPHY_SUMS>(sum, cnt, n, a.part, a.part_n);
}

// One lane per image.
__global__ __launch_bounds__(64) void homography_solve_kernel(const HomographyFitArgs a) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= a.N) return;
    double S[HOMOGRAPHY_SUMS];
    int cnt;
    pwc_fit_gather<HOMOGRAPHY_SUMS>(a.part, a.part_n, n, a.parts, S, cnt);
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
        const PwcFitNorm t = pwc_fit_norm(a.H, a.W);
        const double cx = t.cx, cy = t.cy, s = t.s;
        // G T, row by row; the last row of G is g6 g7 1
        double a00, a01, a02, a10, a11, a12, a20, a21, a22;
        pwc_fit_row_times_t(t, g[0], g[1], g[2], a00, a01, a02);
        pwc_fit_row_times_t(t, g[3], g[4], g[5], a10, a11, a12);
        pwc_fit_row_times_t(t, g[6], g[7], 1.0, a20, a21, a22);
        // T^-1 (G T): rows (s r0) + (cx r2), (s r1) + (cy r2), r2
        double e[9];
        e[0] = (s * a00) + (cx * a20); e[1] = (s * a01) + (cx * a21); e[2] = (s * a02) + (cx * a22);
        e[3] = (s * a10) + (cy * a20); e[4] = (s * a11) + (cy * a21); e[5] = (s * a12) + (cy * a22);
        e[6] = a20; e[7] = a21; e[8] = a22;
        good = good && e[8] > 0.0;
        double m[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) { m[j] = e[j] / e[8]; good = good && pwc_finite(m[j]); }
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
extern "C" size_t pwc_homography_fit_workspace_bytes(int N, int H, int W) {
    return pwc_fit_workspace_bytes(N, H, W, HOMOGRAPHY_SUMS, 8);
}

extern "C" int pwc_homography_fit_f64(const float* flows, int flow_cs, const uint8_t* valid, int N, int H, int W, int iters, double scale,
                                      void* workspace, size_t workspace_bytes, double* matrices, uint8_t* ok, int32_t* count,
                                      double* weight_sum, pwc_stream_t stream) {
    if (!matrices || !ok || !count || !weight_sum) return PWC_EINVAL;
    const int rc = pwc_fit_check(flows, flow_cs, N, H, W, iters, scale, workspace, workspace_bytes,
                                 pwc_homography_fit_workspace_bytes(N, H, W),
                                 pwc_off(matrices, 7u) || pwc_off(weight_sum, 7u) || pwc_off(count, 3u));
    if (rc != PWC_OK) return rc;
    const int parts = (int)pwc_loss_parts(H, W);
    HomographyFitArgs a = {};
    a.flow = flows; a.valid = valid;
    pwc_fit_carve(workspace, N, parts, HOMOGRAPHY_SUMS, 8, a.part, a.param, a.part_n);
    a.matrices = matrices; a.ok = ok; a.count = count; a.weight_sum = weight_sum;
    a.scale = scale; a.cs = flow_cs; a.N = N; a.H = H; a.W = W; a.parts = parts;
    pwc_fit_passes<homography_sums_kernel<true>, homography_sums_kernel<false>, homography_solve_kernel>(
        a, iters, pwc_flow_vec(flow_cs, {flows}), (hipStream_t)stream);
    return pwc_launch_status();
}
