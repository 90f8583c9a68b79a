// pwc_featnorm.hip -- cost-volume feature normalisation: ONE layer norm over the two feature maps of a pair at a pyramid level
// (gfx950; C ABI in include/pwc_hip.h, "feature normalisation"; semantics and bounds in DESIGN.md).
//
//   pwc_feature_norm_f32        y = float32(((double)x - mean) * rstd) for every x of f0[n] and f1[n]; mean and rstd of the pair
//                               (over M = 2 H W C values, biased variance) go to stats[n] = {mean, rstd}
//   pwc_feature_norm_grad_f32   dx (+)= float32(rstd * (g - a - xh * b)), xh recomputed from x, a = sum g / M, b = sum g xh / M
//
// Sums.  loss_common.h's two-stage scheme in doubles: the H W C values of a frame, in flat (pixel, channel) order, are cut into
// groups of four; a pair has `parts` parts (featnorm_parts: a function of H, W and C only, never of N); part b takes the groups
// b * 256 + t, + parts * 256, ... of BOTH frames, a lane adds its groups in that order (f0's four values, then f1's), a workgroup
// adds its lanes in a fixed tree, and the parts are added in index order.  Two calls give the same bits, an image gives the same
// bits alone and in a batch, and the 16-byte path and the scalar path -- which differ only in how a group is fetched -- agree too.
// The second stage is not a launch of its own (pwc_loss_final_kernel would be a third): every workgroup of the consuming kernel
// adds the parts itself, all in the same order, so all of them hold the same bits.
// Variance.  One pass, from sums SHIFTED by the pair's first value K = f0[n][0]: d = x - K, S1 = sum d, S2 = sum d^2,
// mean = K + S1 / M, var = max(S2 / M - (S1 / M)^2, 0).  Two passes would cost a third launch or a second read before the first
// result exists.  The plain form (K = 0) loses (|mean| rstd)^2 ulps of the double to cancellation -- 2^20 of them at
// |mean| rstd = 2^10, and a constant pair comes out with var != 0; the shifted form loses (|mean - K| rstd)^2, and K is a sample:
// a few standard deviations from the mean unless the very first value is an outlier (at worst sqrt(M) of them).
// A pair of at most FEATNORM_ONE_WG_GROUPS groups per frame is one part: ONE workgroup per pair sums and applies in one launch
// (the coarse levels, where a second launch is pure latency).  Otherwise two launches: the parts, then the apply.
// NaN / Inf: plain arithmetic; a pair that holds one comes out non-finite, the other pairs do not see it.  No atomics, no status
// word, no host synchronisation, no process-wide state.
#include "loss_common.h"

#define FEATNORM_ONE_WG_GROUPS 1024
#define FEATNORM_APPLY_BLOCKS 512

struct FeatNormArgs {
    const float* f0;          // [N][H][W] records of f0_cs floats, C used
    const float* f1;
    const float* g0;          // (grad) upstream of y0 / y1
    const float* g1;
    float* o0;                // y0 / y1, or (grad) d f0 / d f1
    float* o1;
    double* part;             // [N][parts][2] partial sums
    double* stats;            // [N][2] mean, rstd: written by the forward, read by the gradient
    int f0_cs, f1_cs, g0_cs, g1_cs, o0_cs, o1_cs;
    int C, parts;
    unsigned E;               // H * W * C, below 2^31
    unsigned G;               // groups of four per frame: ceil(E / 4)
    size_t HW;
    double eps, inv_m;
    int accumulate;
};

// ---------------------------------------------------------------- host: partition
static inline long featnorm_groups(int H, int W, int C) { return ((long)H * W * C + 3) / 4; }
static inline int featnorm_parts(int H, int W, int C) {
    const long G = featnorm_groups(H, W, C);
    if (G <= FEATNORM_ONE_WG_GROUPS) return 1;
    const long p = (G + 255) / 256;
    return (int)(p > 256 ? 256 : p);
}

// ---------------------------------------------------------------- device: a group of four values
// Group q of a frame: the flat values 4 q .. 4 q + 3 (cnt of them exist).  VEC: C % 4 == 0, so the four are one pixel's
// consecutive channels -- one 16-byte access (the host has checked strides and pointers).  Else value by value.
template <bool VEC>
__device__ __forceinline__ int featnorm_load(const float* base, int cs, int C, unsigned q, unsigned E, float v[4]) {
    if (VEC) {
        const unsigned c4 = (unsigned)C >> 2;
        const unsigned pix = q / c4, c = (q - pix * c4) << 2;
        const f32x4 r = *reinterpret_cast<const f32x4*>(base + (size_t)pix * cs + c);
        v[0] = r[0]; v[1] = r[1]; v[2] = r[2]; v[3] = r[3];
        return 4;
    }
    const unsigned e0 = q << 2;
    const int cnt = (int)min(4u, E - e0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = 0.f;
        if (k < cnt) {
            const unsigned e = e0 + k, pix = e / (unsigned)C;
            v[k] = base[(size_t)pix * cs + (e - pix * (unsigned)C)];
        }
    }
    return cnt;
}

// The store of a group: written, or (accumulate) added as fma(1, v, d) = d + v, pwc_grad_store2's rule for one value.
template <bool VEC>
__device__ __forceinline__ void featnorm_store(float* base, int cs, int C, unsigned q, unsigned E, const float v[4], int accumulate) {
    if (VEC) {
        const unsigned c4 = (unsigned)C >> 2;
        const unsigned pix = q / c4, c = (q - pix * c4) << 2;
        f32x4* d = reinterpret_cast<f32x4*>(base + (size_t)pix * cs + c);
        f32x4 r = {v[0], v[1], v[2], v[3]};
        if (accumulate) {
            const f32x4 o = *d;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = __builtin_fmaf(1.f, v[k], o[k]);
        }
        *d = r;
        return;
    }
    const unsigned e0 = q << 2;
    const int cnt = (int)min(4u, E - e0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < cnt) {
            const unsigned e = e0 + k, pix = e / (unsigned)C;
            float* d = base + (size_t)pix * cs + (e - pix * (unsigned)C);
            d[0] = accumulate ? __builtin_fmaf(1.f, v[k], d[0]) : v[k];
        }
    }
}

// pwc_block_tree_sum for two doubles: t += t + k for k = 128, 64 .. 1.  On return EVERY thread holds the totals.
__device__ __forceinline__ void featnorm_tree_sum(double& s, double& u) {
    __shared__ double red[2][256];
    const int t = threadIdx.x;
    __syncthreads();                                                       // (the array is used more than once per kernel)
    red[0][t] = s; red[1][t] = u;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) {
            red[0][t] += red[0][t + k];
            red[1][t] += red[1][t + k];
        }
        __syncthreads();
    }
    s = red[0][0]; u = red[1][0];
}

// The totals of a pair from its parts, added in index order by every thread alike (the parts sit in the LDS first).
__device__ __forceinline__ void featnorm_total(const double* part, int parts, double& s, double& u) {
    __shared__ double sp[2][256];
    const int t = threadIdx.x;
    __syncthreads();
    if (t < parts) { sp[0][t] = part[2 * t]; sp[1][t] = part[2 * t + 1]; }
    __syncthreads();
    s = 0.0; u = 0.0;
    for (int i = 0; i < parts; ++i) { s += sp[0][i]; u += sp[1][i]; }
}

// ---------------------------------------------------------------- device: forward
// Part b of pair n: S1 = sum (x - K), S2 = sum (x - K)^2 over the part's groups of both frames.
template <bool VEC>
__device__ __forceinline__ void featnorm_sums(const FeatNormArgs& a, const float* p0, const float* p1, unsigned b, double K,
                                              double& s1, double& s2) {
    s1 = 0.0; s2 = 0.0;
    for (unsigned q = b * 256u + threadIdx.x; q < a.G; q += (unsigned)a.parts * 256u) {
        float v0[4], v1[4];
        const int cnt = featnorm_load<VEC>(p0, a.f0_cs, a.C, q, a.E, v0);
        featnorm_load<VEC>(p1, a.f1_cs, a.C, q, a.E, v1);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) { const double d = (double)v0[k] - K; s1 += d; s2 = __builtin_fma(d, d, s2); }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) { const double d = (double)v1[k] - K; s1 += d; s2 = __builtin_fma(d, d, s2); }
    }
}

__device__ __forceinline__ void featnorm_moments(const FeatNormArgs& a, double K, double s1, double s2, double& mean, double& rstd) {
    const double m1 = s1 * a.inv_m;
    double var = __builtin_fma(-m1, m1, s2 * a.inv_m);
    var = var < 0.0 ? 0.0 : var;                                           // (a NaN stays a NaN)
    mean = K + m1;
    rstd = 1.0 / sqrt(var + a.eps);
}

template <bool VEC>
__device__ __forceinline__ void featnorm_apply(const FeatNormArgs& a, const float* p0, const float* p1, float* y0, float* y1,
                                               unsigned b, unsigned nb, double mean, double rstd) {
    for (unsigned q = b * 256u + threadIdx.x; q < a.G; q += nb * 256u) {
        float v0[4], v1[4];
        featnorm_load<VEC>(p0, a.f0_cs, a.C, q, a.E, v0);
        featnorm_load<VEC>(p1, a.f1_cs, a.C, q, a.E, v1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v0[k] = (float)(((double)v0[k] - mean) * rstd);
            v1[k] = (float)(((double)v1[k] - mean) * rstd);
        }
        featnorm_store<VEC>(y0, a.o0_cs, a.C, q, a.E, v0, 0);
        featnorm_store<VEC>(y1, a.o1_cs, a.C, q, a.E, v1, 0);
    }
}

// grid (parts, N)
template <bool VEC>
__global__ __launch_bounds__(256) void featnorm_parts_kernel(const FeatNormArgs a) {
    const unsigned n = blockIdx.y;
    const float* p0 = a.f0 + n * a.HW * a.f0_cs;
    const float* p1 = a.f1 + n * a.HW * a.f1_cs;
    double s1, s2;
    featnorm_sums<VEC>(a, p0, p1, blockIdx.x, (double)p0[0], s1, s2);
    featnorm_tree_sum(s1, s2);
    if (threadIdx.x == 0) {
        double* o = a.part + ((size_t)n * a.parts + blockIdx.x) * 2;
        o[0] = s1; o[1] = s2;
    }
}

// grid (blocks, N).  ONE_WG (blocks == 1, parts == 1): the workgroup sums the pair itself; else the parts are in a.part.
template <bool VEC, bool ONE_WG>
__global__ __launch_bounds__(256) void featnorm_apply_kernel(const FeatNormArgs a) {
    const unsigned n = blockIdx.y;
    const float* p0 = a.f0 + n * a.HW * a.f0_cs;
    const float* p1 = a.f1 + n * a.HW * a.f1_cs;
    const double K = (double)p0[0];
    double s1, s2;
    if (ONE_WG) {
        featnorm_sums<VEC>(a, p0, p1, 0, K, s1, s2);
        featnorm_tree_sum(s1, s2);
    } else {
        featnorm_total(a.part + (size_t)n * a.parts * 2, a.parts, s1, s2);
    }
    double mean, rstd;
    featnorm_moments(a, K, s1, s2, mean, rstd);
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.stats[2 * n] = mean; a.stats[2 * n + 1] = rstd; }
    featnorm_apply<VEC>(a, p0, p1, a.o0 + n * a.HW * a.o0_cs, a.o1 + n * a.HW * a.o1_cs, blockIdx.x, gridDim.x, mean, rstd);
}

// ---------------------------------------------------------------- device: gradient
// Part b of pair n: SA = sum g, SB = sum g xh, xh = (x - mean) rstd recomputed from x.
template <bool VEC>
__device__ __forceinline__ void featnorm_grad_sums(const FeatNormArgs& a, unsigned n, unsigned b, double mean, double rstd,
                                                   double& sa, double& sb) {
    const float* p0 = a.f0 + n * a.HW * a.f0_cs;
    const float* p1 = a.f1 + n * a.HW * a.f1_cs;
    const float* q0 = a.g0 + n * a.HW * a.g0_cs;
    const float* q1 = a.g1 + n * a.HW * a.g1_cs;
    sa = 0.0; sb = 0.0;
    for (unsigned q = b * 256u + threadIdx.x; q < a.G; q += (unsigned)a.parts * 256u) {
        float v0[4], v1[4], h0[4], h1[4];
        const int cnt = featnorm_load<VEC>(p0, a.f0_cs, a.C, q, a.E, v0);
        featnorm_load<VEC>(p1, a.f1_cs, a.C, q, a.E, v1);
        featnorm_load<VEC>(q0, a.g0_cs, a.C, q, a.E, h0);
        featnorm_load<VEC>(q1, a.g1_cs, a.C, q, a.E, h1);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) { const double g = (double)h0[k]; sa += g; sb = __builtin_fma(g, ((double)v0[k] - mean) * rstd, sb); }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) { const double g = (double)h1[k]; sa += g; sb = __builtin_fma(g, ((double)v1[k] - mean) * rstd, sb); }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void featnorm_grad_parts_kernel(const FeatNormArgs a) {
    const unsigned n = blockIdx.y;
    double sa, sb;
    featnorm_grad_sums<VEC>(a, n, blockIdx.x, a.stats[2 * n], a.stats[2 * n + 1], sa, sb);
    featnorm_tree_sum(sa, sb);
    if (threadIdx.x == 0) {
        double* o = a.part + ((size_t)n * a.parts + blockIdx.x) * 2;
        o[0] = sa; o[1] = sb;
    }
}

template <bool VEC, bool ONE_WG>
__global__ __launch_bounds__(256) void featnorm_grad_kernel(const FeatNormArgs a) {
    const unsigned n = blockIdx.y;
    const double mean = a.stats[2 * n], rstd = a.stats[2 * n + 1];
    double sa, sb;
    if (ONE_WG) {
        featnorm_grad_sums<VEC>(a, n, 0, mean, rstd, sa, sb);
        featnorm_tree_sum(sa, sb);
    } else {
        featnorm_total(a.part + (size_t)n * a.parts * 2, a.parts, sa, sb);
    }
    const double ga = sa * a.inv_m, gb = sb * a.inv_m;
    const float* p0 = a.f0 + n * a.HW * a.f0_cs;
    const float* p1 = a.f1 + n * a.HW * a.f1_cs;
    const float* q0 = a.g0 + n * a.HW * a.g0_cs;
    const float* q1 = a.g1 + n * a.HW * a.g1_cs;
    float* d0 = a.o0 + n * a.HW * a.o0_cs;
    float* d1 = a.o1 + n * a.HW * a.o1_cs;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < a.G; q += gridDim.x * 256u) {
        float v0[4], v1[4], h0[4], h1[4];
        featnorm_load<VEC>(p0, a.f0_cs, a.C, q, a.E, v0);
        featnorm_load<VEC>(p1, a.f1_cs, a.C, q, a.E, v1);
        featnorm_load<VEC>(q0, a.g0_cs, a.C, q, a.E, h0);
        featnorm_load<VEC>(q1, a.g1_cs, a.C, q, a.E, h1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // rstd * (g - a - xh * b), the last two terms as one fused multiply-add whatever the compiler contracts
            v0[k] = (float)(rstd * __builtin_fma(-(((double)v0[k] - mean) * rstd), gb, (double)h0[k] - ga));
            v1[k] = (float)(rstd * __builtin_fma(-(((double)v1[k] - mean) * rstd), gb, (double)h1[k] - ga));
        }
        featnorm_store<VEC>(d0, a.o0_cs, a.C, q, a.E, v0, a.accumulate);
        featnorm_store<VEC>(d1, a.o1_cs, a.C, q, a.E, v1, a.accumulate);
    }
}

// ---------------------------------------------------------------- host
extern "C" size_t pwc_feature_norm_workspace_bytes(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || (long)H * W * C >= (1L << 31)) return 0;
    const int parts = featnorm_parts(H, W, C);
    return parts == 1 ? 0 : (size_t)N * parts * 2 * sizeof(double);
}

extern "C" int pwc_feature_norm_parts(int H, int W, int C) {
    if (H <= 0 || W <= 0 || C <= 0 || (long)H * W * C >= (1L << 31)) return 0;
    return featnorm_parts(H, W, C);
}

// The checks both entry points share behind their own null / stride checks, in the order they report.
static int featnorm_check(int N, int H, int W, int C, const void* stats, const void* workspace, size_t workspace_bytes) {
    if ((long)H * W * C >= (1L << 31) || N > 65535) return PWC_ERANGE;
    if (pwc_off(stats, 7u)) return PWC_EALIGN;
    const size_t need = pwc_feature_norm_workspace_bytes(N, H, W, C);
    if (need) {
        if (!workspace) return PWC_EINVAL;
        if (pwc_off(workspace, 7u)) return PWC_EALIGN;
        if (workspace_bytes < need) return PWC_EINVAL;
    }
    return PWC_OK;
}

static void featnorm_geometry(FeatNormArgs& a, int H, int W, int C, void* workspace, double* stats) {
    a.C = C; a.parts = featnorm_parts(H, W, C);
    a.E = (unsigned)((long)H * W * C); a.G = (unsigned)featnorm_groups(H, W, C);
    a.HW = (size_t)H * W;
    a.inv_m = 1.0 / (2.0 * (double)a.E);
    a.part = reinterpret_cast<double*>(workspace);
    a.stats = stats;
}

static inline dim3 featnorm_apply_grid(const FeatNormArgs& a, int N) {
    const unsigned blocks = (a.G + 255u) / 256u;
    return dim3(blocks > FEATNORM_APPLY_BLOCKS ? FEATNORM_APPLY_BLOCKS : blocks, (unsigned)N);
}

extern "C" int pwc_feature_norm_f32(const float* f0, int f0_cs, const float* f1, int f1_cs, int N, int H, int W, int C, double eps,
                                    void* workspace, size_t workspace_bytes, float* y0, int y0_cs, float* y1, int y1_cs,
                                    double* stats, pwc_stream_t stream) {
    if (!f0 || !f1 || !y0 || !y1 || !stats || N <= 0 || H <= 0 || W <= 0 || C <= 0) return PWC_EINVAL;
    if (f0_cs < C || f1_cs < C || y0_cs < C || y1_cs < C || !(eps >= 0.0)) return PWC_EINVAL;
    if (pwc_off(f0, 3u) || pwc_off(f1, 3u) || pwc_off(y0, 3u) || pwc_off(y1, 3u)) return PWC_EALIGN;
    const int rc = featnorm_check(N, H, W, C, stats, workspace, workspace_bytes);
    if (rc != PWC_OK) return rc;
    FeatNormArgs a = {};
    a.f0 = f0; a.f1 = f1; a.o0 = y0; a.o1 = y1;
    a.f0_cs = f0_cs; a.f1_cs = f1_cs; a.o0_cs = y0_cs; a.o1_cs = y1_cs; a.eps = eps;
    featnorm_geometry(a, H, W, C, workspace, stats);
    const bool vec = !(C & 3) && !((f0_cs | f1_cs | y0_cs | y1_cs) & 3) && pwc_aligned16(f0) && pwc_aligned16(f1) &&
                     pwc_aligned16(y0) && pwc_aligned16(y1);
    const hipStream_t s = (hipStream_t)stream;
    if (a.parts == 1) {
        if (vec) hipLaunchKernelGGL((featnorm_apply_kernel<true, true>), dim3(1, N), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((featnorm_apply_kernel<false, true>), dim3(1, N), dim3(256), 0, s, a);
        return pwc_launch_status();
    }
    const dim3 pg((unsigned)a.parts, (unsigned)N), ag = featnorm_apply_grid(a, N);
    if (vec) {
        hipLaunchKernelGGL(featnorm_parts_kernel<true>, pg, dim3(256), 0, s, a);
        hipLaunchKernelGGL((featnorm_apply_kernel<true, false>), ag, dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(featnorm_parts_kernel<false>, pg, dim3(256), 0, s, a);
        hipLaunchKernelGGL((featnorm_apply_kernel<false, false>), ag, dim3(256), 0, s, a);
    }
    return pwc_launch_status();
}

extern "C" int pwc_feature_norm_grad_f32(const float* f0, int f0_cs, const float* f1, int f1_cs, const float* g0, int g0_cs,
                                         const float* g1, int g1_cs, const double* stats, int N, int H, int W, int C,
                                         void* workspace, size_t workspace_bytes, float* d0, int d0_cs, float* d1, int d1_cs,
                                         int accumulate, pwc_stream_t stream) {
    if (!f0 || !f1 || !g0 || !g1 || !d0 || !d1 || !stats || N <= 0 || H <= 0 || W <= 0 || C <= 0) return PWC_EINVAL;
    if (f0_cs < C || f1_cs < C || g0_cs < C || g1_cs < C || d0_cs < C || d1_cs < C) return PWC_EINVAL;
    if (pwc_off(f0, 3u) || pwc_off(f1, 3u) || pwc_off(g0, 3u) || pwc_off(g1, 3u) || pwc_off(d0, 3u) ||
        pwc_off(d1, 3u))
        return PWC_EALIGN;
    const int rc = featnorm_check(N, H, W, C, stats, workspace, workspace_bytes);
    if (rc != PWC_OK) return rc;
    FeatNormArgs a = {};
    a.f0 = f0; a.f1 = f1; a.g0 = g0; a.g1 = g1; a.o0 = d0; a.o1 = d1;
    a.f0_cs = f0_cs; a.f1_cs = f1_cs; a.g0_cs = g0_cs; a.g1_cs = g1_cs; a.o0_cs = d0_cs; a.o1_cs = d1_cs;
    a.accumulate = accumulate ? 1 : 0;
    featnorm_geometry(a, H, W, C, workspace, const_cast<double*>(stats));
    const bool vec = !(C & 3) && !((f0_cs | f1_cs | g0_cs | g1_cs | d0_cs | d1_cs) & 3) && pwc_aligned16(f0) && pwc_aligned16(f1) &&
                     pwc_aligned16(g0) && pwc_aligned16(g1) && pwc_aligned16(d0) && pwc_aligned16(d1);
    const hipStream_t s = (hipStream_t)stream;
    if (a.parts == 1) {
        if (vec) hipLaunchKernelGGL((featnorm_grad_kernel<true, true>), dim3(1, N), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((featnorm_grad_kernel<false, true>), dim3(1, N), dim3(256), 0, s, a);
        return pwc_launch_status();
    }
    const dim3 pg((unsigned)a.parts, (unsigned)N), ag = featnorm_apply_grid(a, N);
    if (vec) {
        hipLaunchKernelGGL(featnorm_grad_parts_kernel<true>, pg, dim3(256), 0, s, a);
        hipLaunchKernelGGL((featnorm_grad_kernel<true, false>), ag, dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(featnorm_grad_parts_kernel<false>, pg, dim3(256), 0, s, a);
        hipLaunchKernelGGL((featnorm_grad_kernel<false, false>), ag, dim3(256), 0, s, a);
    }
    return pwc_launch_status();
}
