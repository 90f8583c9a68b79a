// robust_fit.h -- the skeleton of the reweighted fits (pwc_motion_fit_f64, pwc_homography_fit_f64, pwc_fundamental_fit_f64,
// pwc_pose_refine_f64), written once.  A fit is iters + 1 passes of two launches each on the caller's stream, the
// device reading what the pass before wrote:
//   sums    grid (parts, N), loss_common.h's partition: part b takes the pixels b 256 + t, + parts 256, ... of its image, adds the M
//           terms of its known pixels and a count to its lanes' sums, the 256 lanes add in the fixed tree and lane 0 writes the part
//           (pwc_fit_write_part).  Known: mask non-zero, then the flow loaded and known (flow_record.h); each kernel writes that
//           loop head out itself;
//   solve   a lane per image adds the parts in index order (pwc_fit_gather) and solves.
// The workspace is 8 (N parts M + N state) + 4 N parts bytes, rounded up to 8: the parts' sums, the state a pass leaves the next one,
// the parts' counts (pwc_fit_workspace_bytes, pwc_fit_carve).  What a model adds per pixel and how it solves stay in its file.
#pragma once
#include "flow_record.h"
#include "loss_common.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------- device
// The normalisation T of an H x W image: xh = (x - cx) / s, yh = (y - cy) / s.
struct PwcFitNorm {
    double cx, cy, s;
};
__device__ __forceinline__ PwcFitNorm pwc_fit_norm(int H, int W) {
    return PwcFitNorm{(double)(W - 1) / 2.0, (double)(H - 1) / 2.0, (double)max(H, W) / 2.0};
}
// Pixel i of an image W wide.
__device__ __forceinline__ void pwc_fit_normalise(const PwcFitNorm& t, int i, int W, double& xh, double& yh) {
    xh = ((double)(i % W) - t.cx) / t.s;
    yh = ((double)(i / W) - t.cy) / t.s;
}
// A row h of a matrix in normalised coordinates times T: (h0 / s, h1 / s, h2 - ((h0 cx) + (h1 cy)) / s).
__device__ __forceinline__ void pwc_fit_row_times_t(const PwcFitNorm& t, double h0, double h1, double h2, double& r0, double& r1,
                                                    double& r2) {
    r0 = h0 / t.s;
    r1 = h1 / t.s;
    r2 = h2 - (((h0 * t.cx) + (h1 * t.cy)) / t.s);
}

// The part of workgroup blockIdx.x of image n: M sums and a count, tree-summed, into part ([N][gridDim.x][M]) and part_n.
template <int M>
__device__ __forceinline__ void pwc_fit_write_part(double* sum, int cnt, int n, double* part, int* part_n) {
    pwc_block_tree_sum_f64<M, 1>(sum, &cnt);
    if (threadIdx.x == 0) {
        const size_t o = (size_t)n * gridDim.x + blockIdx.x;
#pragma unroll
        for (int j = 0; j < M; ++j) part[o * M + j] = sum[j];
        part_n[o] = cnt;
    }
}

// Image n's parts added in index order.
template <int M>
__device__ __forceinline__ void pwc_fit_gather(const double* part, const int* part_n, int n, int parts, double* S, int& cnt) {
#pragma unroll
    for (int j = 0; j < M; ++j) S[j] = 0.0;
    cnt = 0;
    for (int i = 0; i < parts; ++i) {
        const size_t o = (size_t)n * parts + i;
#pragma unroll
        for (int j = 0; j < M; ++j) S[j] = S[j] + part[o * M + j];
        cnt += part_n[o];
    }
}

// ---------------------------------------------------------------- host
// M sums per part, `state` doubles per image.
static inline size_t pwc_fit_workspace_bytes(int N, int H, int W, int M, int state) {
    if (N <= 0 || H <= 0 || W <= 0 || !pwc_loss_in_range(N, H, W)) return 0;
    const size_t cells = (size_t)N * pwc_loss_parts(H, W);
    return 8 * (cells * M + (size_t)N * state) + ((4 * cells + 7) & ~(size_t)7);
}
static inline void pwc_fit_carve(void* workspace, int N, int parts, int M, int state, double*& part, double*& st, int*& part_n) {
    part = reinterpret_cast<double*>(workspace);
    st = part + (size_t)N * parts * M;
    part_n = reinterpret_cast<int*>(st + (size_t)N * state);
}

// The checks the four entry points share, in the order they report: null pointers and values out of their domain (PWC_EINVAL),
// the range (PWC_ERANGE), the alignment (PWC_EALIGN; own_off: one of the entry point's own pointers is off its boundary), the
// workspace's size (PWC_EINVAL; needed: the entry point's *_workspace_bytes).  An entry point's own null and domain checks are
// PWC_EINVAL too and stand in front of this call.
static inline int pwc_fit_check(const float* flows, int flow_cs, int N, int H, int W, int iters, double scale, const void* workspace,
                                size_t workspace_bytes, size_t needed, bool own_off) {
    if (!flows || !workspace) return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || iters < 0 || iters > PWC_MOTION_MAX_ITERS || !(scale > 0.0) || flow_cs < 2) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (pwc_off(flows, 3u) || pwc_off(workspace, 7u) || own_off) return PWC_EALIGN;
    if (workspace_bytes < needed) return PWC_EINVAL;
    return PWC_OK;
}

// The passes of a fit whose arguments carry `first` and `last`: pass 0 has w = 1, the last pass writes the result.
template <auto SumsVec, auto Sums, auto Solve, typename Args>
static inline void pwc_fit_passes(Args& a, int iters, bool vec, hipStream_t s) {
    for (int pass = 0; pass <= iters; ++pass) {
        a.first = pass == 0 ? 1 : 0;
        a.last = pass == iters ? 1 : 0;
        if (vec) hipLaunchKernelGGL(SumsVec, dim3(a.parts, a.N), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(Sums, dim3(a.parts, a.N), dim3(256), 0, s, a);
        hipLaunchKernelGGL(Solve, dim3((a.N + 63) / 64), dim3(64), 0, s, a);
    }
}
