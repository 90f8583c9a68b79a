// loss_common.h -- what the loss, loss-gradient and metric kernels (pwc_flow_loss.hip, pwc_unsup.hip, pwc_census.hip) share.  Their numerics are
// bit-level contracts (tests/test_gpu_loss_bits.py), and every rule of them is written here once:
//   sums       an image is cut into at most 256 parts of 256-pixel strides (pwc_loss_parts), a workgroup adds its part in a fixed
//              tree (pwc_block_tree_sum), one thread per image adds the parts in index order (pwc_loss_final_kernel) -- two calls
//              give the same bits; pwc_block_tree_sum_f64 is the same tree in doubles (pwc_motion.hip);
//   norm       the ground truth's nearest-neighbour index (pwc_nearest_index), the difference with the ground truth DIVIDED
//              (pwc_flow_diff), the norm of a pixel and its direction (pwc_norm_term, pwc_norm_direction);
//   rho        the generalised Charbonnier function of the label-free terms and its derivative (unsup_rho, unsup_rho_grad);
//   gradients  gathers, one lane per pixel of the batch: the flat pixel's (n, y, x) (pwc_loss_pixel), the launch width
//              (pwc_loss_grad_blocks), the plain / accumulate store of the two channels (pwc_grad_store2, pwc_grad_skip2).
#pragma once
#include "pwc_common.h"

// ---------------------------------------------------------------- host: partition, workspace, checks
// The parts of an H x W image: part b of `parts` takes the pixels b * 256 + t, + parts * 256, ...; at most 256 of them.
static inline long pwc_loss_parts(int H, int W) {
    long parts = ((long)H * W + 255) / 256;
    return parts > 256 ? 256 : parts;
}
// `words` 32-bit words (float sums, int32 counts) per part of every image.
static inline size_t pwc_loss_workspace_floats(int N, int H, int W, int words) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)words * N * pwc_loss_parts(H, W);
}
// The pixels of an image are indexed with an int that the sums loops advance by up to 256 parts * 256 lanes = 65536 past the last
// pixel before they compare it: H * W + 65536 has to fit.  The images are indexed with a grid dimension.
#define PWC_LOSS_MAX_PIXELS (2147483647L - 65536L)
static inline bool pwc_loss_in_range(int N, int H, int W) { return (long)H * W <= PWC_LOSS_MAX_PIXELS && N <= 65535; }
// The checks the *_sums entry points share, behind their own, in the order they report: the range (PWC_ERANGE), then the
// workspace (PWC_EINVAL).
static inline int pwc_loss_sums_check(int N, int H, int W, int words, size_t workspace_floats) {
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (workspace_floats < pwc_loss_workspace_floats(N, H, W, words)) return PWC_EINVAL;
    return PWC_OK;
}
// Workgroups of a gradient kernel over npix = N * H * W pixels: pwc_common.h's flat grid.
static inline dim3 pwc_loss_grad_blocks(int N, int H, int W) { return pwc_flat_grid((long)N * H * W); }

// ---------------------------------------------------------------- device: sums
// Sum of M floats and K ints over the 256 threads of a workgroup: t += t + k for k = 128, 64 .. 1, every quantity on its own,
// one barrier per step.  On return thread 0's sf / ci hold the totals (the other threads' are unchanged).  K = 0: ci unused.
template <int M, int K>
__device__ __forceinline__ void pwc_block_tree_sum(float* sf, int* ci) {
    __shared__ float redf[M][256];
    __shared__ int redi[K > 0 ? K : 1][256];
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < M; ++j) redf[j][t] = sf[j];
#pragma unroll
    for (int j = 0; j < K; ++j) redi[j][t] = ci[j];
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) {
#pragma unroll
            for (int j = 0; j < M; ++j) redf[j][t] += redf[j][t + k];
#pragma unroll
            for (int j = 0; j < K; ++j) redi[j][t] += redi[j][t + k];
        }
        __syncthreads();
    }
    if (t == 0) {
#pragma unroll
        for (int j = 0; j < M; ++j) sf[j] = redf[j][0];
#pragma unroll
        for (int j = 0; j < K; ++j) ci[j] = redi[j][0];
    }
}

// The same rule in doubles (pwc_motion.hip): M doubles and K ints, the same tree, the same barriers.  24 KB of LDS at M = 12.
template <int M, int K>
__device__ __forceinline__ void pwc_block_tree_sum_f64(double* sd, int* ci) {
    __shared__ double redd[M][256];
    __shared__ int redi[K > 0 ? K : 1][256];
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < M; ++j) redd[j][t] = sd[j];
#pragma unroll
    for (int j = 0; j < K; ++j) redi[j][t] = ci[j];
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) {
#pragma unroll
            for (int j = 0; j < M; ++j) redd[j][t] += redd[j][t + k];
#pragma unroll
            for (int j = 0; j < K; ++j) redi[j][t] += redi[j][t + k];
        }
        __syncthreads();
    }
    if (t == 0) {
#pragma unroll
        for (int j = 0; j < M; ++j) sd[j] = redd[j][0];
#pragma unroll
        for (int j = 0; j < K; ++j) ci[j] = redi[j][0];
    }
}

// The part of workgroup (blockIdx.x, image blockIdx.y): a float sum and, COUNTS, an int count, into partial / partial_n
// ([N][gridDim.x] each).
template <bool COUNTS>
__device__ __forceinline__ void pwc_loss_write_part(float s, int cnt, float* partial, int* partial_n) {
    pwc_block_tree_sum<1, COUNTS ? 1 : 0>(&s, &cnt);
    if (threadIdx.x == 0) {
        const size_t o = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[o] = s;
        if (COUNTS) partial_n[o] = cnt;
    }
}

// One thread per image: the parts are added in index order (deterministic), the counts as integers (exact).
template <bool COUNTS>
__global__ void pwc_loss_final_kernel(const float* __restrict__ partial, const int* __restrict__ partial_n, int nparts, int nimg,
                                      float* __restrict__ out, int* __restrict__ out_n) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nimg) return;
    float s = 0.f;
    int c = 0;
    for (int i = 0; i < nparts; ++i) {
        s += partial[(size_t)n * nparts + i];
        if (COUNTS) c += partial_n[(size_t)n * nparts + i];
    }
    out[n] = s;
    if (COUNTS) out_n[n] = c;
}
// workspace = [N][parts] float sums, then (out_counts given) [N][parts] int32 counts
static inline void pwc_loss_final_launch(const float* workspace, int parts, int N, float* out_sums, int32_t* out_counts,
                                         pwc_stream_t stream) {
    const dim3 grid((unsigned)((N + 63) / 64));
    const int* partial_n = reinterpret_cast<const int*>(workspace + (size_t)N * parts);
    if (out_counts)
        hipLaunchKernelGGL(pwc_loss_final_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, workspace, partial_n, parts, N,
                           out_sums, (int*)out_counts);
    else
        hipLaunchKernelGGL(pwc_loss_final_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, workspace, (const int*)nullptr,
                           parts, N, out_sums, (int*)nullptr);
}

// ---------------------------------------------------------------- device: the norm of a pixel
// tf.image.resize_nearest_neighbor (TF 1.8, align_corners=False): source index floor(dst * in / out) of the ROUNDED product,
// clipped; scale = (float)in / (float)out.
__device__ __forceinline__ int pwc_nearest_index(int dst, float scale, int in) {
    return min((int)floorf(pwc_mul_rounded((float)dst, scale)), in - 1);
}
// pred - gt / gt_div.  The ground truth is DIVIDED (losses.py:20 `flows_gt/20.`), not multiplied by a reciprocal: x / 20 and
// x * (1 / 20) differ by 1 ulp.  The loss is the norm of gt / gt_div - pred, which is this value negated -- exactly, so the
// norm is the same bits -- and its gradient w.r.t. pred has this value's direction.
__device__ __forceinline__ float pwc_flow_diff(float pred, float gt, float gt_div) { return pred - gt / gt_div; }
__device__ __forceinline__ float pwc_norm_term(float dx, float dy, int ord) {
    return ord == 1 ? fabsf(dx) + fabsf(dy) : sqrtf(dx * dx + dy * dy);
}
// d/d(dx, dy) of pwc_norm_term: ord 1 the signs; ord 2 (dx, dy) / norm, 0 where the norm is 0.
__device__ __forceinline__ void pwc_norm_direction(float dx, float dy, int ord, float& ox, float& oy) {
    if (ord == 1) {
        ox = dx > 0.f ? 1.f : (dx < 0.f ? -1.f : 0.f);
        oy = dy > 0.f ? 1.f : (dy < 0.f ? -1.f : 0.f);
    } else {
        const float nrm = sqrtf(dx * dx + dy * dy);
        ox = nrm > 0.f ? dx / nrm : 0.f;
        oy = nrm > 0.f ? dy / nrm : 0.f;
    }
}

// ---------------------------------------------------------------- device: the robust function of the label-free terms
// rho(d) = (d^2 + eps^2)^q (generalised Charbonnier) and rho'(d); eps2 = eps * eps (pwc_unsup.hip, pwc_census.hip).
__device__ __forceinline__ float unsup_rho(float d, float eps2, float q) { return powf(d * d + eps2, q); }
__device__ __forceinline__ float unsup_rho_grad(float d, float eps2, float q) { return 2.f * q * d * powf(d * d + eps2, q - 1.f); }

// ---------------------------------------------------------------- device: gradient scaffolding
// Flat pixel p of an [N][H][W] batch.
struct PwcLossPixel {
    int n, y, x;
};
__device__ __forceinline__ PwcLossPixel pwc_loss_pixel(long p, int H, int W) {
    const int x = (int)(p % W);
    const long r = p / W;
    return PwcLossPixel{(int)(r / H), (int)(r % H), x};
}
// The two channels of a pixel's gradient record: scale * (ox, oy) written, or (accumulate) added to what is there -- then as ONE
// fused multiply-add, which is what the norm gradient has always compiled to, spelled out so that it does not hang on the
// compiler's contraction.  A caller whose accumulate has to add exactly what a plain call writes rounds the product itself
// (pwc_mul_rounded) and passes it with scale 1: fma(1, v, d) is d + v.
__device__ __forceinline__ void pwc_grad_store2(float* d, int accumulate, float scale, float ox, float oy) {
    d[0] = accumulate ? __builtin_fmaf(scale, ox, d[0]) : scale * ox;
    d[1] = accumulate ? __builtin_fmaf(scale, oy, d[1]) : scale * oy;
}
// A pixel that does not contribute: set to 0, or (accumulate: it adds nothing) left alone.
__device__ __forceinline__ void pwc_grad_skip2(float* d, int accumulate) {
    if (!accumulate) { d[0] = 0.f; d[1] = 0.f; }
}
