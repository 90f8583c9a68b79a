// pwc_pose_refine.hip -- refinement of the relative pose of camera_pose: a reweighted Gauss-Newton fit of the five pose parameters
// to the Sampson distance over a fixed set of inlier pixels, wholly on the device (gfx950; C ABI and every operation's order in
// include/pwc_hip.h, "pose refinement"; launch plan and figures in DESIGN.md 30).
//
//   pwc_pose_refine_workspace_bytes   8 (N parts 22 + N 19) + 4 N parts, rounded up to 8: the parts' sums and counts, the pose in work
//   pwc_pose_refine_f64               rotation (N, 3, 3), translation (N, 3) doubles, ok (N) bytes, samples and best_pass (N) int32,
//                                     cost (N, iters + 1) and weight_sum (N) doubles
//
// The pass structure is robust_fit.h's: iters + 1 passes of two launches each on the caller's stream, the device reading
// what the pass before wrote.
//   sums    grid (parts, N), loss_common.h's partition.  The pixel set is decided against the INPUT pose in every pass (the same
//           pixels each time); a pixel of the set adds the 15 entries of the triangle of w J J^T, the 5 of w J rho, w and w d^2 under
//           the pose of the pass.  ONE tree round over all 22 (45 KB of LDS in pwc_block_tree_sum_f64).  An OFF or frozen image's
//           workgroups return at once.  The pose, the basis and the intrinsics of the image are wave-uniform.
//   solve   a lane per image adds the parts in index order, records the cost, keeps the best pose so far in the outputs and, before
//           the last pass, runs motion_ldlt<5, 1> with the pivot rule d > 1e-9 trace and writes the next pose into the workspace.
// Every value is an IEEE double + - x / sqrt or a comparison in the order written here -- no fused multiply-add is formed anywhere
// in this file (the pragma below), sqrt on doubles (correctly rounded) is the only library call -- so tests/pose_refine_ref.py
// restates it in numpy bit for bit.  No atomic, no host synchronisation, no process-wide state.
#include "motion_ldlt.h"
#include "robust_fit.h"
#include "two_view.h"

#pragma clang fp contract(off)

#define REFINE_SUMS 22
#define REFINE_STATE 19       // doubles per image: R (9), t (3), b1 (3), b2 (3), live (1.0 or 0.0)
#define REFINE_LIVE 18
#define REFINE_MIN_SAMPLES 5
#define REFINE_PIVOT 1e-9

struct RefineArgs {
    const float* flow;        // [N][H][W] records of cs floats, 2 used
    const uint8_t* valid;     // [N][H][W], null: every pixel
    const double* intrinsics; // [N][4]: fx fy cx cy
    const double* rotation0;  // [N][9]: the input pose
    const double* translation0; // [N][3]
    double* part;             // [N][parts][22]
    double* state;            // [N][REFINE_STATE]
    int* part_n;              // [N][parts]
    double* rotation;         // [N][9]
    double* translation;      // [N][3]
    uint8_t* ok;              // [N]
    int* samples;             // [N]
    int* best_pass;           // [N]
    double* cost;             // [N][iters + 1]
    double* weight_sum;       // [N]
    double scale, threshold;
    int cs, N, H, W, parts;
    int pass, iters;
};

// OFF of the header: an all-zero rotation or intrinsics that are not FINE.
__device__ __forceinline__ bool refine_off(const double* R0, const double* k) {
    bool zero = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) zero = zero && R0[j] == 0.0;
    return zero || !two_view_intrinsics_fine(k);
}

template <bool VEC, bool FIRST>
__global__ __launch_bounds__(256) void pose_refine_sums_kernel(const RefineArgs a) {
    const int n = blockIdx.y, hw = a.H * a.W;
    double R0[9], t0[3], k[4];
#pragma unroll
    for (int j = 0; j < 9; ++j) R0[j] = a.rotation0[(size_t)n * 9 + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) t0[j] = a.translation0[(size_t)n * 3 + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = a.intrinsics[(size_t)n * 4 + j];
    if (refine_off(R0, k)) return;                                         // (the whole workgroup: the solve reads no part of it)
    const double* st = a.state + (size_t)n * REFINE_STATE;
    if (!FIRST && st[REFINE_LIVE] == 0.0) return;                                   // frozen
    double R[9], t[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) R[j] = FIRST ? R0[j] : st[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = FIRST ? t0[j] : st[9 + j];
    double b1[3], b2[3];
    if (FIRST) {
        two_view_tangent_basis(t, b1, b2);
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) { b1[j] = st[12 + j]; b2[j] = st[15 + j]; }
    }
    const double fx = k[0], fy = k[1], cx = k[2], cy = k[3];
    const double c2 = a.scale * a.scale;
    const size_t img = (size_t)n * hw;
    double sum[REFINE_SUMS];
#pragma unroll
    for (int j = 0; j < REFINE_SUMS; ++j) sum[j] = 0.0;
    int cnt = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += (int)gridDim.x * 256) {
        if (a.valid && !a.valid[img + i]) continue;
        float fu, fv;
        pwc_flow_load2<VEC>(a.flow + (img + i) * a.cs, fu, fv);
        if (!pwc_flow_known(fu, fv)) continue;
        const double x = (double)(i % a.W), y = (double)(i / a.W);
        const double xp = x + (double)fu, yp = y + (double)fv;
        const double d0x = (x - cx) / fx, d0y = (y - cy) / fy, d1x = (xp - cx) / fx, d1y = (yp - cy) / fy;
        TwoViewEpipolar q = two_view_epipolar(R0, t0, fx, fy, d0x, d0y, d1x, d1y);
        if (!(q.g > 0.0)) continue;
        if (!((fabs(q.r) / sqrt(q.g)) <= a.threshold)) continue;
        cnt += 1;                                                          // (a pixel of the set, in this pass or left out of it)
        if (!FIRST) {
            q = two_view_epipolar(R, t, fx, fy, d0x, d0y, d1x, d1y);
            if (!(q.g > 0.0)) continue;
        }
        const double sg = sqrt(q.g);
        const double rho = q.r / sg;
        const double d2 = (q.r * q.r) / q.g;
        const double w = 1.0 / (1.0 + (d2 / c2));
        double J[5];
        J[0] = ((q.a1 * q.e2) - (q.a2 * q.e1)) / sg;
        J[1] = ((q.a2 * q.e0) - (q.a0 * q.e2)) / sg;
        J[2] = ((q.a0 * q.e1) - (q.a1 * q.e0)) / sg;
        J[3] = (-(((q.c0 * b1[0]) + (q.c1 * b1[1])) + (q.c2 * b1[2]))) / sg;
        J[4] = (-(((q.c0 * b2[0]) + (q.c1 * b2[1])) + (q.c2 * b2[2]))) / sg;
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const double wj = w * J[r];
#pragma unroll
            for (int c = 0; c <= r; ++c) sum[r * (r + 1) / 2 + c] = sum[r * (r + 1) / 2 + c] + (wj * J[c]);
            sum[15 + r] = sum[15 + r] + (wj * rho);
        }
        sum[20] = sum[20] + w;
        sum[21] = sum[21] + (w * d2);
    }
    pwc_fit_write_part<REFINE_SUMS>(sum, cnt, n, a.part, a.part_n);
}

// One lane per image.
__global__ __launch_bounds__(64) void pose_refine_solve_kernel(const RefineArgs a) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= a.N) return;
    const bool first = a.pass == 0;
    const int passes = a.iters + 1;
    double* st = a.state + (size_t)n * REFINE_STATE;
    double* cost = a.cost + (size_t)n * passes;
    double R[9], t[3], k[4];
#pragma unroll
    for (int j = 0; j < 9; ++j) R[j] = a.rotation0[(size_t)n * 9 + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = a.translation0[(size_t)n * 3 + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = a.intrinsics[(size_t)n * 4 + j];
    const bool off = refine_off(R, k);
    if (!first && (off || st[REFINE_LIVE] == 0.0)) {                                // a pass that an OFF or frozen image skips
        cost[a.pass] = 0.0;
        return;
    }
    double S[REFINE_SUMS];
#pragma unroll
    for (int j = 0; j < REFINE_SUMS; ++j) S[j] = 0.0;
    int cnt = 0;
    if (!off) pwc_fit_gather<REFINE_SUMS>(a.part, a.part_n, n, a.parts, S, cnt);   // (an OFF image's workgroups wrote no part)
    if (first) {
        const bool good = !off && cnt >= REFINE_MIN_SAMPLES;
#pragma unroll
        for (int j = 0; j < 9; ++j) a.rotation[(size_t)n * 9 + j] = good ? R[j] : 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) a.translation[(size_t)n * 3 + j] = good ? t[j] : 0.0;
        a.ok[n] = good ? 1 : 0;
        a.samples[n] = cnt;
        a.best_pass[n] = 0;
        a.weight_sum[n] = good ? S[20] : 0.0;
        cost[0] = good ? S[21] : 0.0;
        if (!good) {
            st[REFINE_LIVE] = 0.0;
            return;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = st[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = st[9 + j];
    }
    bool fin = true;
#pragma unroll
    for (int j = 0; j < REFINE_SUMS; ++j) fin = fin && pwc_finite(S[j]);
    if (!first) {
        if (!fin) {
            cost[a.pass] = 0.0;
            st[REFINE_LIVE] = 0.0;
            return;
        }
        cost[a.pass] = S[21];
        if (S[21] < cost[a.best_pass[n]]) {                                // (only a strictly lower cost: ties to the earlier pass)
#pragma unroll
            for (int j = 0; j < 9; ++j) a.rotation[(size_t)n * 9 + j] = R[j];
#pragma unroll
            for (int j = 0; j < 3; ++j) a.translation[(size_t)n * 3 + j] = t[j];
            a.best_pass[n] = a.pass;
            a.weight_sum[n] = S[20];
        }
    }
    if (a.pass == a.iters) return;
    bool live = fin;
    double Rn[9], tn[3];
    if (live) {
        const double A[5][5] = {{S[0], 0.0, 0.0, 0.0, 0.0},
                                {S[1], S[2], 0.0, 0.0, 0.0},
                                {S[3], S[4], S[5], 0.0, 0.0},
                                {S[6], S[7], S[8], S[9], 0.0},
                                {S[10], S[11], S[12], S[13], S[14]}};
        double r[1][5] = {{-S[15], -S[16], -S[17], -S[18], -S[19]}};
        const double tr = (((S[0] + S[2]) + S[5]) + S[9]) + S[14];
        live = motion_ldlt<5, 1>(A, r, REFINE_PIVOT * tr);
        if (live) {
            // the Cayley map of omega = r[0][0 .. 2], a = omega / 2
            const double a0 = r[0][0] / 2.0, a1 = r[0][1] / 2.0, a2 = r[0][2] / 2.0;
            const double q = ((a0 * a0) + (a1 * a1)) + (a2 * a2);
            const double p = 1.0 - q, den = 1.0 + q;
            double C[9];
            C[0] = (p + (2.0 * (a0 * a0))) / den; C[1] = ((2.0 * (a0 * a1)) - (2.0 * a2)) / den; C[2] = ((2.0 * (a0 * a2)) + (2.0 * a1)) / den;
            C[3] = ((2.0 * (a1 * a0)) + (2.0 * a2)) / den; C[4] = (p + (2.0 * (a1 * a1))) / den; C[5] = ((2.0 * (a1 * a2)) - (2.0 * a0)) / den;
            C[6] = ((2.0 * (a2 * a0)) - (2.0 * a1)) / den; C[7] = ((2.0 * (a2 * a1)) + (2.0 * a0)) / den; C[8] = (p + (2.0 * (a2 * a2))) / den;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int c = 0; c < 3; ++c) Rn[3 * i + c] = ((C[3 * i] * R[c]) + (C[3 * i + 1] * R[3 + c])) + (C[3 * i + 2] * R[6 + c]);
            }
            double b1[3], b2[3], u[3];
            two_view_tangent_basis(t, b1, b2);
#pragma unroll
            for (int i = 0; i < 3; ++i) u[i] = (t[i] + (r[0][3] * b1[i])) + (r[0][4] * b2[i]);
            const double nrm = sqrt(((u[0] * u[0]) + (u[1] * u[1])) + (u[2] * u[2]));
#pragma unroll
            for (int i = 0; i < 3; ++i) { tn[i] = u[i] / nrm; live = live && pwc_finite(tn[i]); }
#pragma unroll
            for (int j = 0; j < 9; ++j) live = live && pwc_finite(Rn[j]);
        }
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < 9; ++j) st[j] = Rn[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) st[9 + j] = tn[j];
        double b1[3], b2[3];
        two_view_tangent_basis(tn, b1, b2);                                // (the next pass's sums read it; the next solve forms it again)
#pragma unroll
        for (int j = 0; j < 3; ++j) { st[12 + j] = b1[j]; st[15 + j] = b2[j]; }
    }
    st[REFINE_LIVE] = live ? 1.0 : 0.0;
}

// ---------------------------------------------------------------- host
extern "C" size_t pwc_pose_refine_workspace_bytes(int N, int H, int W) {
    return pwc_fit_workspace_bytes(N, H, W, REFINE_SUMS, REFINE_STATE);
}

extern "C" int pwc_pose_refine_f64(const float* flows, int flow_cs, const uint8_t* valid, const double* intrinsics,
                                   const double* rotation0, const double* translation0, int N, int H, int W, int iters, double scale,
                                   double threshold, void* workspace, size_t workspace_bytes, double* rotation, double* translation,
                                   uint8_t* ok, int32_t* samples, int32_t* best_pass, double* cost, double* weight_sum,
                                   pwc_stream_t stream) {
    if (!intrinsics || !rotation0 || !translation0 || !rotation || !translation || !ok || !samples || !best_pass || !cost || !weight_sum)
        return PWC_EINVAL;
    if (!(threshold >= 0.0)) return PWC_EINVAL;
    const int rc = pwc_fit_check(flows, flow_cs, N, H, W, iters, scale, workspace, workspace_bytes, pwc_pose_refine_workspace_bytes(N, H, W),
                                 pwc_off(intrinsics, 7u) || pwc_off(rotation0, 7u) || pwc_off(translation0, 7u) ||
                                     pwc_off(rotation, 7u) || pwc_off(translation, 7u) || pwc_off(samples, 3u) ||
                                     pwc_off(best_pass, 3u) || pwc_off(cost, 7u) || pwc_off(weight_sum, 7u));
    if (rc != PWC_OK) return rc;
    const int parts = (int)pwc_loss_parts(H, W);
    RefineArgs a = {};
    a.flow = flows; a.valid = valid; a.intrinsics = intrinsics; a.rotation0 = rotation0; a.translation0 = translation0;
    pwc_fit_carve(workspace, N, parts, REFINE_SUMS, REFINE_STATE, a.part, a.state, a.part_n);
    a.rotation = rotation; a.translation = translation; a.ok = ok; a.samples = samples; a.best_pass = best_pass;
    a.cost = cost; a.weight_sum = weight_sum;
    a.scale = scale; a.threshold = threshold; a.cs = flow_cs; a.N = N; a.H = H; a.W = W; a.parts = parts; a.iters = iters;
    const bool vec = pwc_flow_vec(flow_cs, {flows});
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(parts, N);
    for (int pass = 0; pass <= iters; ++pass) {
        a.pass = pass;
        if (pass == 0) {
            if (vec) hipLaunchKernelGGL((pose_refine_sums_kernel<true, true>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((pose_refine_sums_kernel<false, true>), grid, dim3(256), 0, s, a);
        } else {
            if (vec) hipLaunchKernelGGL((pose_refine_sums_kernel<true, false>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((pose_refine_sums_kernel<false, false>), grid, dim3(256), 0, s, a);
        }
        hipLaunchKernelGGL(pose_refine_solve_kernel, dim3((N + 63) / 64), dim3(64), 0, s, a);
    }
    return pwc_launch_status();
}
