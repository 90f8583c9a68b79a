// pwc_pose.hip -- relative pose and depth from a flow field, a fundamental matrix and a calibration: how the camera moved between the
// two frames and how far away every rigid pixel is, wholly on the device (gfx950; C ABI and every operation's order in
// include/pwc_hip.h, "relative pose and depth"; launch plan and figures in DESIGN.md 28).
//
//   pwc_camera_pose_workspace_bytes   8 x 22 N: per image the two candidate rotations, the translation and a flag
//   pwc_camera_pose_f64               rotation (N, 3, 3), translation (N, 3) doubles, ok (N) bytes, votes (N, 4) and voters (N) int32,
//                                     singular (N, 2) and essential (N, 3, 3) doubles
//   pwc_triangulate_depth_f32         depth (N, H, W) floats, known (N, H, W) bytes, optionally parallax (N, H, W) floats
//
// pwc_camera_pose_f64 is three launches on the caller's stream, each reading what the one before wrote:
//   decompose  a lane per image: E = K^T F K entry by entry, motion_jacobi<3> of E^T E, the singular vectors, the four textbook
//              candidates (R_a, +t), (R_a, -t), (R_b, +t), (R_b, -t) into the workspace; it also zeroes the image's counts.
//   vote       grid (parts, N), loss_common.h's partition.  A known pixel that is a Sampson inlier of F (pwc_fundamental.hip's
//              rule, in pixels) triangulates under R_a and R_b with +t (two_view.h); under -t both depths are the exact negations,
//              so two triangulations decide four candidates.  A lane keeps four counts and the voters in registers; a wave adds
//              them with a butterfly, the four waves meet in the LDS and ONE integer atomic per count and workgroup reaches
//              global memory (pwc_region_links.hip's rule): integers, the same in any order.
//   select     a lane per image: the candidate with the most votes, ties to the lowest index, if it holds more than half the voters.
// pwc_triangulate_depth_f32 is one launch, a lane per pixel of the batch, epipolar_residual_kernel's loads and grid.
// Every value is an IEEE double + - x / sqrt or a comparison in the order written here -- no fused multiply-add is formed anywhere
// in this file (the pragma below), sqrt on doubles (correctly rounded) is the only library call -- so tests/pose_ref.py restates it
// in numpy bit for bit.  No floating-point atomic, no host synchronisation, no process-wide state.
#include "loss_common.h"
#include "motion_jacobi.h"
#include "two_view.h"

#pragma clang fp contract(off)

#define POSE_WS 22            // doubles per image: R_a (9), R_b (9), t (3), good (1.0 or 0.0)

struct PoseArgs {
    const float* flow;        // [N][H][W] records of cs floats, 2 used
    const uint8_t* valid;     // [N][H][W], null: every pixel
    const double* matrices;   // [N][9]: F
    const double* intrinsics; // [N][4]: fx fy cx cy
    double* ws;               // [N][POSE_WS]
    double* rotation;         // [N][9]
    double* translation;      // [N][3]
    uint8_t* ok;              // [N]
    int* votes;               // [N][4]
    int* voters;              // [N]
    double* singular;         // [N][2]
    double* essential;        // [N][9]
    double threshold;
    int cs, N, H, W;
};

// ---------------------------------------------------------------- decompose: one lane per image
__global__ __launch_bounds__(64) void pose_decompose_kernel(const PoseArgs a) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= a.N) return;
    double f[9], k[4];
    bool zero = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) { f[j] = a.matrices[(size_t)n * 9 + j]; zero = zero && f[j] == 0.0; }
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = a.intrinsics[(size_t)n * 4 + j];
    bool good = !zero && two_view_intrinsics_fine(k);
    double E[9], Ra[9], Rb[9], t[3], sing[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 9; ++j) { E[j] = 0.0; Ra[j] = 0.0; Rb[j] = 0.0; }
    t[0] = 0.0; t[1] = 0.0; t[2] = 0.0;
    if (good) {
        const double fx = k[0], fy = k[1], cx = k[2], cy = k[3];
        // G = F K row by row, then E = K^T G down the columns
        double G[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            G[3 * i] = f[3 * i] * fx;
            G[3 * i + 1] = f[3 * i + 1] * fy;
            G[3 * i + 2] = ((f[3 * i] * cx) + (f[3 * i + 1] * cy)) + f[3 * i + 2];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            E[j] = fx * G[j];
            E[3 + j] = fy * G[3 + j];
            E[6 + j] = ((cx * G[j]) + (cy * G[3 + j])) + G[6 + j];
        }
        double B[3][3], V[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = i; j < 3; ++j) B[i][j] = ((E[i] * E[j]) + (E[3 + i] * E[3 + j])) + (E[6 + i] * E[6 + j]);
        }
        motion_jacobi<3>(B, V);
        int j0;
        double v3[3];
        const double l3 = motion_jacobi_smallest<3>(B, V, -1, v3, j0);
        // the other two columns in column order (no array is indexed with j0)
        double v1[3], v2[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            v1[i] = j0 == 0 ? V[i][1] : V[i][0];
            v2[i] = j0 == 2 ? V[i][1] : V[i][2];
        }
        const double l1 = j0 == 0 ? B[1][1] : B[0][0], l2 = j0 == 2 ? B[1][1] : B[2][2];
        const double s1 = sqrt(l1), s2 = sqrt(l2), s3 = l3 > 0.0 ? sqrt(l3) : 0.0;
        good = s1 > 0.0 && s2 > 0.0;
        sing[0] = s2 / s1; sing[1] = s3 / s1;
        double u1[3], u2[3], u3[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            u1[i] = (((E[3 * i] * v1[0]) + (E[3 * i + 1] * v1[1])) + (E[3 * i + 2] * v1[2])) / s1;
            u2[i] = (((E[3 * i] * v2[0]) + (E[3 * i + 1] * v2[1])) + (E[3 * i + 2] * v2[2])) / s2;
        }
        u3[0] = (u1[1] * u2[2]) - (u1[2] * u2[1]);
        u3[1] = (u1[2] * u2[0]) - (u1[0] * u2[2]);
        u3[2] = (u1[0] * u2[1]) - (u1[1] * u2[0]);
        const double nrm = sqrt(((u3[0] * u3[0]) + (u3[1] * u3[1])) + (u3[2] * u3[2]));
#pragma unroll
        for (int i = 0; i < 3; ++i) u3[i] = u3[i] / nrm;
        // det V = (v1 x v2) . v3 < 0: the null column is negated
        const double c0 = (v1[1] * v2[2]) - (v1[2] * v2[1]), c1 = (v1[2] * v2[0]) - (v1[0] * v2[2]), c2 = (v1[0] * v2[1]) - (v1[1] * v2[0]);
        const double det = ((c0 * v3[0]) + (c1 * v3[1])) + (c2 * v3[2]);
        if (det < 0.0) { v3[0] = -v3[0]; v3[1] = -v3[1]; v3[2] = -v3[2]; }
        // R_a = U W V^T = u2 v1^T - u1 v2^T + u3 v3^T;  R_b = U W^T V^T = u1 v2^T - u2 v1^T + u3 v3^T
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Ra[3 * r + c] = ((u2[r] * v1[c]) - (u1[r] * v2[c])) + (u3[r] * v3[c]);
                Rb[3 * r + c] = ((u1[r] * v2[c]) - (u2[r] * v1[c])) + (u3[r] * v3[c]);
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) { t[i] = u3[i]; good = good && pwc_finite(t[i]); }
#pragma unroll
        for (int j = 0; j < 9; ++j) good = good && pwc_finite(Ra[j]) && pwc_finite(Rb[j]) && pwc_finite(E[j]);
        good = good && pwc_finite(sing[0]) && pwc_finite(sing[1]);
    }
    double* w = a.ws + (size_t)n * POSE_WS;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        w[j] = good ? Ra[j] : 0.0;
        w[9 + j] = good ? Rb[j] : 0.0;
        a.essential[(size_t)n * 9 + j] = good ? E[j] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) w[18 + j] = good ? t[j] : 0.0;
    w[21] = good ? 1.0 : 0.0;
    a.singular[(size_t)n * 2] = good ? sing[0] : 0.0;
    a.singular[(size_t)n * 2 + 1] = good ? sing[1] : 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) a.votes[(size_t)n * 4 + j] = 0;
    a.voters[n] = 0;
}

// ---------------------------------------------------------------- vote: grid (parts, N)
template <bool VEC>
__global__ __launch_bounds__(256) void pose_vote_kernel(const PoseArgs a) {
    __shared__ int wave_count[4][5];
    const int n = blockIdx.y, hw = a.H * a.W;
    const double* w = a.ws + (size_t)n * POSE_WS;
    if (w[21] == 0.0) return;                                              // (the whole workgroup: the image has no candidates)
    const size_t img = (size_t)n * hw;
    double f[9], Ra[9], Rb[9], t[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) { f[j] = a.matrices[(size_t)n * 9 + j]; Ra[j] = w[j]; Rb[j] = w[9 + j]; }
    t[0] = w[18]; t[1] = w[19]; t[2] = w[20];
    const double fx = a.intrinsics[(size_t)n * 4], fy = a.intrinsics[(size_t)n * 4 + 1];
    const double cx = a.intrinsics[(size_t)n * 4 + 2], cy = a.intrinsics[(size_t)n * 4 + 3];
    int cnt[5] = {0, 0, 0, 0, 0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += (int)gridDim.x * 256) {
        if (a.valid && !a.valid[img + i]) continue;
        float fu, fv;
        pwc_flow_load2<VEC>(a.flow + (img + i) * a.cs, fu, fv);
        if (!pwc_flow_known(fu, fv)) continue;
        const double x = (double)(i % a.W), y = (double)(i / a.W);
        const double xp = x + (double)fu, yp = y + (double)fv;
        double r, g;
        two_view_sampson(f, x, y, xp, yp, r, g);
        if (!(g > 0.0)) continue;
        if (!((fabs(r) / sqrt(g)) <= a.threshold)) continue;
        cnt[4] += 1;
        const double d0x = (x - cx) / fx, d0y = (y - cy) / fy, d1x = (xp - cx) / fx, d1y = (yp - cy) / fy;
        const TwoViewPoint pa = two_view_triangulate(Ra, t, d0x, d0y, d1x, d1y);
        const TwoViewPoint pb = two_view_triangulate(Rb, t, d0x, d0y, d1x, d1y);
        // (R, -t): z0 and z1 are the exact negations of (R, +t)'s
        cnt[0] += pa.den > 0.0 && pa.z0 > 0.0 && pa.z1 > 0.0 ? 1 : 0;
        cnt[1] += pa.den > 0.0 && pa.z0 < 0.0 && pa.z1 < 0.0 ? 1 : 0;
        cnt[2] += pb.den > 0.0 && pb.z0 > 0.0 && pb.z1 > 0.0 ? 1 : 0;
        cnt[3] += pb.den > 0.0 && pb.z0 < 0.0 && pb.z1 < 0.0 ? 1 : 0;
    }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) {
#pragma unroll
        for (int j = 0; j < 5; ++j) cnt[j] += __shfl_xor(cnt[j], k);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 5; ++j) wave_count[threadIdx.x >> 6][j] = cnt[j];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int j = threadIdx.x;
        const int total = (wave_count[0][j] + wave_count[1][j]) + (wave_count[2][j] + wave_count[3][j]);
        if (total != 0) atomicAdd(j < 4 ? a.votes + (size_t)n * 4 + j : a.voters + n, total);
    }
}

// ---------------------------------------------------------------- select: one lane per image
__global__ __launch_bounds__(64) void pose_select_kernel(const PoseArgs a) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= a.N) return;
    const double* w = a.ws + (size_t)n * POSE_WS;
    const int voters = a.voters[n];
    int best = a.votes[(size_t)n * 4], at = 0;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const int v = a.votes[(size_t)n * 4 + j];
        if (v > best) { best = v; at = j; }                                // (only a strictly larger count: ties to the lowest index)
    }
    const bool good = w[21] != 0.0 && voters > 0 && 2L * best > (long)voters;
    const double sign = (at & 1) ? -1.0 : 1.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) a.rotation[(size_t)n * 9 + j] = good ? (at < 2 ? w[j] : w[9 + j]) : 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) a.translation[(size_t)n * 3 + j] = good ? sign * w[18 + j] : 0.0;
    a.ok[n] = good ? 1 : 0;
}

// ---------------------------------------------------------------- depth
struct DepthArgs {
    const float* flow;        // [N][H][W] records of cs floats
    const uint8_t* valid;     // [N][H][W], null: every pixel
    const double* rotation;   // [N][9]
    const double* translation;// [N][3]
    const double* intrinsics; // [N][4]
    float* depth;             // [N][H][W]
    uint8_t* known;           // [N][H][W]
    float* parallax;          // [N][H][W] or null
    double min_parallax;
    int cs, N, H, W;
};

// One lane per pixel of the batch.
template <bool VEC>
__global__ __launch_bounds__(256) void pose_depth_kernel(const DepthArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel q = pwc_loss_pixel(p, a.H, a.W);
        double R[9], t[3], k[4];
        bool zero = true;
#pragma unroll
        for (int j = 0; j < 9; ++j) { R[j] = a.rotation[(size_t)q.n * 9 + j]; zero = zero && R[j] == 0.0; }
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = a.translation[(size_t)q.n * 3 + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = a.intrinsics[(size_t)q.n * 4 + j];
        float d = PWC_FLOW_SENTINEL, par = 0.f;
        uint8_t kn = 0;
        if (!zero && two_view_intrinsics_fine(k) && !(a.valid && !a.valid[p])) {
            float fu, fv;
            pwc_flow_load2<VEC>(a.flow + (size_t)p * a.cs, fu, fv);
            if (pwc_flow_known(fu, fv)) {
                const double x = (double)q.x, y = (double)q.y;
                const double xp = x + (double)fu, yp = y + (double)fv;
                const double d0x = (x - k[2]) / k[0], d0y = (y - k[3]) / k[1], d1x = (xp - k[2]) / k[0], d1y = (yp - k[3]) / k[1];
                const TwoViewPoint pt = two_view_triangulate(R, t, d0x, d0y, d1x, d1y);
                if (pt.a2 > 0.0) {
                    // where a point at infinity along the first ray would be seen in the second frame
                    const double ex = xp - ((k[0] * (pt.a0 / pt.a2)) + k[2]), ey = yp - ((k[1] * (pt.a1 / pt.a2)) + k[3]);
                    const double pp = sqrt((ex * ex) + (ey * ey));
                    par = (float)pp;
                    if (pt.den > 0.0 && pt.z0 > 0.0 && pt.z1 > 0.0 && pp >= a.min_parallax) {
                        d = (float)pt.z0;
                        kn = 1;
                    }
                }
            }
        }
        a.depth[p] = d;
        a.known[p] = kn;
        if (a.parallax) a.parallax[p] = par;
    }
}

// ---------------------------------------------------------------- host
extern "C" size_t pwc_camera_pose_workspace_bytes(int N) {
    if (N <= 0 || N > 65535) return 0;
    return 8 * (size_t)N * POSE_WS;
}

extern "C" int pwc_camera_pose_f64(const float* flows, int flow_cs, const uint8_t* valid, const double* matrices,
                                   const double* intrinsics, int N, int H, int W, double threshold, void* workspace,
                                   size_t workspace_bytes, double* rotation, double* translation, uint8_t* ok, int32_t* votes,
                                   int32_t* voters, double* singular, double* essential, pwc_stream_t stream) {
    if (!flows || !matrices || !intrinsics || !workspace || !rotation || !translation || !ok || !votes || !voters || !singular || !essential)
        return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || flow_cs < 2 || !(threshold >= 0.0)) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (pwc_off(flows, 3u) || pwc_off(matrices, 7u) || pwc_off(intrinsics, 7u) || pwc_off(workspace, 7u) || pwc_off(rotation, 7u) ||
        pwc_off(translation, 7u) || pwc_off(votes, 3u) || pwc_off(voters, 3u) || pwc_off(singular, 7u) || pwc_off(essential, 7u))
        return PWC_EALIGN;
    if (workspace_bytes < pwc_camera_pose_workspace_bytes(N)) return PWC_EINVAL;
    PoseArgs a = {};
    a.flow = flows; a.valid = valid; a.matrices = matrices; a.intrinsics = intrinsics;
    a.ws = reinterpret_cast<double*>(workspace);
    a.rotation = rotation; a.translation = translation; a.ok = ok; a.votes = votes; a.voters = voters;
    a.singular = singular; a.essential = essential;
    a.threshold = threshold; a.cs = flow_cs; a.N = N; a.H = H; a.W = W;
    const int parts = (int)pwc_loss_parts(H, W);
    const bool vec = pwc_flow_vec(flow_cs, {flows});
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pose_decompose_kernel, dim3((N + 63) / 64), dim3(64), 0, s, a);
    if (vec) hipLaunchKernelGGL(pose_vote_kernel<true>, dim3(parts, N), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(pose_vote_kernel<false>, dim3(parts, N), dim3(256), 0, s, a);
    hipLaunchKernelGGL(pose_select_kernel, dim3((N + 63) / 64), dim3(64), 0, s, a);
    return pwc_launch_status();
}

extern "C" int pwc_triangulate_depth_f32(const float* flows, int flow_cs, const uint8_t* valid, const double* rotation,
                                         const double* translation, const double* intrinsics, int N, int H, int W,
                                         double min_parallax, float* depth, uint8_t* known, float* parallax, pwc_stream_t stream) {
    if (!flows || !rotation || !translation || !intrinsics || !depth || !known) return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || flow_cs < 2 || !(min_parallax >= 0.0)) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (pwc_off(flows, 3u) || pwc_off(depth, 3u) || pwc_off(parallax, 3u) || pwc_off(rotation, 7u) || pwc_off(translation, 7u) ||
        pwc_off(intrinsics, 7u))
        return PWC_EALIGN;
    DepthArgs a = {};
    a.flow = flows; a.valid = valid; a.rotation = rotation; a.translation = translation; a.intrinsics = intrinsics;
    a.depth = depth; a.known = known; a.parallax = parallax;
    a.min_parallax = min_parallax; a.cs = flow_cs; a.N = N; a.H = H; a.W = W;
    const bool vec = pwc_flow_vec(flow_cs, {flows});
    const dim3 grid = pwc_loss_grad_blocks(N, H, W);
    const hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(pose_depth_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(pose_depth_kernel<false>, grid, dim3(256), 0, s, a);
    return pwc_launch_status();
}
