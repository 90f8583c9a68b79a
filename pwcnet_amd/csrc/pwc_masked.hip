// pwc_masked.hip -- sparse ground truth: the loss sums, the loss gradient and the flow metrics under a validity mask
// (gfx950; C ABI in include/pwc_hip.h, "sparse ground truth").
//
//   pwc_flow_norm_masked_sums_f32   per-image sums of ||pred - gt / gt_div||_ord over the VALID pixels, and their number
//   pwc_flow_norm_masked_grad_f32   the gradient of those sums w.r.t. pred; invalid pixels get 0 (or stay as they are)
//   pwc_flow_metrics_f32            EPE sums, KITTI outliers, 1/3/5-px error counts, EPE by motion magnitude
//
// The mask is one byte per pixel of the GROUND TRUTH, non-zero = valid, read at the nearest-neighbour index the ground truth is
// read at (tf.image.resize_nearest_neighbor of the mask).  Invalid pixels are selected out, not multiplied out: neither pred nor
// gt is read there, so NaN, Inf or the .flo sentinel 1e10 at an invalid pixel cannot reach a sum or a gradient.
// The masked sums / gradient restate the per-pixel arithmetic of flow_norm_partial_kernel (pwc_ops.hip) and
// flow_norm_grad_kernel (pwc_backward.hip) expression by expression, with the same partition of the pixels and the same order
// of additions: under an all-ones mask they return the unmasked kernels' bits (tests/test_gpu_masked_loss.py).
#include "pwc_common.h"

struct MaskedNormArgs {
    const float* pred;
    const float* gt;
    const uint8_t* valid;    // [N][GH][GW]
    float* partial;          // [N][gridDim.x] sums
    int* partial_n;          // [N][gridDim.x] valid-pixel counts
    int pred_cs, gt_cs;
    int H, W, GH, GW;
    float sy, sx, gt_div;
    int ord;
};

__global__ __launch_bounds__(256) void flow_norm_masked_partial_kernel(const MaskedNormArgs a) {
    __shared__ float red[256];
    __shared__ int redn[256];
    const int n = blockIdx.y;
    const int npix = a.H * a.W;
    float s = 0.f;
    int cnt = 0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
        const int y = p / a.W, x = p - y * a.W;
        const int gy = min((int)floorf(pwc_mul_rounded((float)y, a.sy)), a.GH - 1), gx = min((int)floorf(pwc_mul_rounded((float)x, a.sx)), a.GW - 1);
        const size_t g = ((size_t)n * a.GH + gy) * a.GW + gx;
        if (a.valid[g]) {
            const float* pp = a.pred + ((size_t)n * npix + p) * a.pred_cs;
            const float* gp = a.gt + g * a.gt_cs;
            const float dx = gp[0] / a.gt_div - pp[0], dy = gp[1] / a.gt_div - pp[1];
            s += a.ord == 1 ? fabsf(dx) + fabsf(dy) : sqrtf(dx * dx + dy * dy);
            ++cnt;
        }
    }
    red[threadIdx.x] = s;
    redn[threadIdx.x] = cnt;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            red[threadIdx.x] += red[threadIdx.x + k];
            redn[threadIdx.x] += redn[threadIdx.x + k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.partial[(size_t)n * gridDim.x + blockIdx.x] = red[0];
        a.partial_n[(size_t)n * gridDim.x + blockIdx.x] = redn[0];
    }
}

__global__ void flow_norm_masked_final_kernel(const float* __restrict__ partial, const int* __restrict__ partial_n, int nparts,
                                              int nimg, float* __restrict__ out, int* __restrict__ out_n) {
    // one thread per image: the partials are added in index order (deterministic), the counts as integers (exact)
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nimg) return;
    float s = 0.f;
    int c = 0;
    for (int i = 0; i < nparts; ++i) {
        s += partial[(size_t)n * nparts + i];
        c += partial_n[(size_t)n * nparts + i];
    }
    out[n] = s;
    out_n[n] = c;
}

// the partition of pwc_flow_norm_workspace_floats (pwc_ops.hip): at most 256 parts of an image
static inline long masked_parts(int H, int W) {
    long parts = ((long)H * W + 255) / 256;
    return parts > 256 ? 256 : parts;
}

extern "C" size_t pwc_flow_norm_masked_workspace_floats(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * (size_t)N * masked_parts(H, W);       // a float sum and an int32 count per part
}

extern "C" int pwc_flow_norm_masked_sums_f32(const float* pred, int pred_cs, const float* gt, int gt_cs, const uint8_t* valid,
                                             int N, int H, int W, int GH, int GW, float gt_div, int ord, float* workspace,
                                             size_t workspace_floats, float* out_sums, int32_t* out_counts, pwc_stream_t stream) {
    if (!pred || !gt || !valid || !workspace || !out_sums || !out_counts) return PWC_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || GH <= 0 || GW <= 0 || pred_cs < 2 || gt_cs < 2) return PWC_EINVAL;
    if (ord != 1 && ord != 2) return PWC_EUNSUPPORTED;
    if (!(gt_div != 0.f)) return PWC_EINVAL;
    if ((long)H * W >= (1L << 31) || N > 65535) return PWC_ERANGE;
    if (workspace_floats < pwc_flow_norm_masked_workspace_floats(N, H, W)) return PWC_EINVAL;
    const int parts = (int)masked_parts(H, W);
    MaskedNormArgs a;
    a.pred = pred; a.gt = gt; a.valid = valid; a.partial = workspace;
    a.partial_n = reinterpret_cast<int*>(workspace + (size_t)N * parts);
    a.pred_cs = pred_cs; a.gt_cs = gt_cs;
    a.H = H; a.W = W; a.GH = GH; a.GW = GW;
    a.sy = (float)GH / (float)H; a.sx = (float)GW / (float)W; a.gt_div = gt_div; a.ord = ord;
    hipLaunchKernelGGL(flow_norm_masked_partial_kernel, dim3((unsigned)parts, (unsigned)N), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(flow_norm_masked_final_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       (const float*)a.partial, (const int*)a.partial_n, parts, N, out_sums, (int*)out_counts);
    return pwc_launch_status();
}

// ------------------------------------------------------------------ masked loss gradient
struct MaskedNormGradArgs {
    const float* pred;
    const float* gt;
    const uint8_t* valid;
    float* dpred;
    int pred_cs, gt_cs, dpred_cs;
    int N, H, W, GH, GW;
    float sy, sx, gt_div, scale;
    int ord, accumulate;
};

__global__ __launch_bounds__(256) void flow_norm_masked_grad_kernel(const MaskedNormGradArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const int x = (int)(p % a.W);
        const long r = p / a.W;
        const int y = (int)(r % a.H), n = (int)(r / a.H);
        const int gy = min((int)floorf(pwc_mul_rounded((float)y, a.sy)), a.GH - 1);
        const int gx = min((int)floorf(pwc_mul_rounded((float)x, a.sx)), a.GW - 1);
        const long g = ((long)n * a.GH + gy) * a.GW + gx;
        float* d = a.dpred + p * a.dpred_cs;
        if (!a.valid[g]) {
            if (!a.accumulate) { d[0] = 0.f; d[1] = 0.f; }       // accumulate: an invalid pixel adds nothing
            continue;
        }
        const float* pp = a.pred + p * a.pred_cs;
        const float* gp = a.gt + g * a.gt_cs;
        const float dx = pp[0] - gp[0] / a.gt_div, dy = pp[1] - gp[1] / a.gt_div;
        float ox, oy;
        if (a.ord == 1) {
            ox = dx > 0.f ? 1.f : (dx < 0.f ? -1.f : 0.f);
            oy = dy > 0.f ? 1.f : (dy < 0.f ? -1.f : 0.f);
        } else {
            const float nrm = sqrtf(dx * dx + dy * dy);
            ox = nrm > 0.f ? dx / nrm : 0.f;
            oy = nrm > 0.f ? dy / nrm : 0.f;
        }
        d[0] = a.accumulate ? d[0] + a.scale * ox : a.scale * ox;
        d[1] = a.accumulate ? d[1] + a.scale * oy : a.scale * oy;
    }
}

extern "C" int pwc_flow_norm_masked_grad_f32(const float* pred, int pred_cs, const float* gt, int gt_cs, const uint8_t* valid,
                                             int N, int H, int W, int GH, int GW, float gt_div, int ord, float scale,
                                             float* dpred, int dpred_cs, int accumulate, pwc_stream_t stream) {
    if (!pred || !gt || !valid || !dpred || N <= 0 || H <= 0 || W <= 0 || GH <= 0 || GW <= 0) return PWC_EINVAL;
    if (pred_cs < 2 || gt_cs < 2 || dpred_cs < 2 || !(gt_div != 0.f)) return PWC_EINVAL;
    if (ord != 1 && ord != 2) return PWC_EUNSUPPORTED;
    MaskedNormGradArgs a;
    a.pred = pred; a.gt = gt; a.valid = valid; a.dpred = dpred; a.pred_cs = pred_cs; a.gt_cs = gt_cs; a.dpred_cs = dpred_cs;
    a.N = N; a.H = H; a.W = W; a.GH = GH; a.GW = GW;
    a.sy = (float)GH / (float)H; a.sx = (float)GW / (float)W; a.gt_div = gt_div; a.scale = scale; a.ord = ord;
    a.accumulate = accumulate;
    long blocks = ((long)N * H * W + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(flow_norm_masked_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return pwc_launch_status();
}

// ------------------------------------------------------------------ flow metrics
// Per image, over the valid pixels, with e = ||pred - gt||_2 and g = ||gt||_2 (both flows in pixels, one resolution):
//   0 n_valid   1 sum e   2 n(e > 3 && e > 0.05 g) [KITTI Fl]   3 n(e > 1)   4 n(e > 3)   5 n(e > 5)
//   6 n(g < 10)   7 sum e (g < 10)   8 n(10 <= g < 40)   9 sum e (10 <= g < 40)   10 n(g >= 40)   11 sum e (g >= 40)
// One pass: every thread keeps the eight integer counts and the four float sums, a block adds them in a fixed tree and writes
// twelve words per part ([N][parts][12], counts as int32 bits); one thread per image then adds the parts in index order, the
// counts as integers, the sums in double.
#define PWC_METRICS 12
struct FlowMetricsArgs {
    const float* pred;
    const float* gt;
    const uint8_t* valid;    // null: every pixel
    float* partial;          // [N][gridDim.x][12]
    int pred_cs, gt_cs;
    int npix;
};

__global__ __launch_bounds__(256) void flow_metrics_partial_kernel(const FlowMetricsArgs a) {
    __shared__ float redf[4][256];     // sum e: all, g < 10, 10 <= g < 40, g >= 40
    __shared__ int redi[8][256];       // n_valid, n_fl, n(e > 1), n(e > 3), n(e > 5), n(g < 10), n(10 <= g < 40), n(g >= 40)
    const int n = blockIdx.y;
    float sf[4] = {0.f, 0.f, 0.f, 0.f};
    int ci[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int p = blockIdx.x * 256 + threadIdx.x; p < a.npix; p += gridDim.x * 256) {
        const size_t q = (size_t)n * a.npix + p;
        if (a.valid && !a.valid[q]) continue;
        const float* pp = a.pred + q * a.pred_cs;
        const float* gp = a.gt + q * a.gt_cs;
        const float gx = gp[0], gy = gp[1];
        const float dx = pp[0] - gx, dy = pp[1] - gy;
        const float e = sqrtf(dx * dx + dy * dy), g = sqrtf(gx * gx + gy * gy);
        ci[0] += 1;
        sf[0] += e;
        ci[1] += (e > 3.f && e > 0.05f * g) ? 1 : 0;
        ci[2] += e > 1.f ? 1 : 0;
        ci[3] += e > 3.f ? 1 : 0;
        ci[4] += e > 5.f ? 1 : 0;
        if (g < 10.f) { ci[5] += 1; sf[1] += e; }
        else if (g < 40.f) { ci[6] += 1; sf[2] += e; }
        else if (g >= 40.f) { ci[7] += 1; sf[3] += e; }       // (a NaN magnitude belongs to no bucket)
    }
    const int t = threadIdx.x;
    for (int j = 0; j < 4; ++j) redf[j][t] = sf[j];
    for (int j = 0; j < 8; ++j) redi[j][t] = ci[j];
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) {
            for (int j = 0; j < 4; ++j) redf[j][t] += redf[j][t + k];
            for (int j = 0; j < 8; ++j) redi[j][t] += redi[j][t + k];
        }
        __syncthreads();
    }
    if (t == 0) {
        float* o = a.partial + ((size_t)n * gridDim.x + blockIdx.x) * PWC_METRICS;
        int* oi = reinterpret_cast<int*>(o);
        oi[0] = redi[0][0]; o[1] = redf[0][0]; oi[2] = redi[1][0]; oi[3] = redi[2][0]; oi[4] = redi[3][0]; oi[5] = redi[4][0];
        oi[6] = redi[5][0]; o[7] = redf[1][0]; oi[8] = redi[6][0]; o[9] = redf[2][0]; oi[10] = redi[7][0]; o[11] = redf[3][0];
    }
}

__global__ void flow_metrics_final_kernel(const float* __restrict__ partial, int nparts, int nimg, double* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nimg) return;
    double s[PWC_METRICS];
    long c[PWC_METRICS];
    for (int j = 0; j < PWC_METRICS; ++j) { s[j] = 0.0; c[j] = 0; }
    for (int i = 0; i < nparts; ++i) {
        const float* o = partial + ((size_t)n * nparts + i) * PWC_METRICS;
        const int* oi = reinterpret_cast<const int*>(o);
        for (int j = 0; j < PWC_METRICS; ++j) {
            const bool is_sum = j == 1 || j == 7 || j == 9 || j == 11;
            if (is_sum) s[j] += (double)o[j];
            else c[j] += oi[j];
        }
    }
    for (int j = 0; j < PWC_METRICS; ++j) {
        const bool is_sum = j == 1 || j == 7 || j == 9 || j == 11;
        out[(size_t)n * PWC_METRICS + j] = is_sum ? s[j] : (double)c[j];
    }
}

extern "C" size_t pwc_flow_metrics_workspace_floats(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)PWC_METRICS * N * masked_parts(H, W);
}

extern "C" int pwc_flow_metrics_f32(const float* pred, int pred_cs, const float* gt, int gt_cs, const uint8_t* valid, int N, int H,
                                    int W, float* workspace, size_t workspace_floats, double* out, pwc_stream_t stream) {
    if (!pred || !gt || !workspace || !out) return PWC_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || pred_cs < 2 || gt_cs < 2) return PWC_EINVAL;
    if ((long)H * W >= (1L << 31) || N > 65535) return PWC_ERANGE;
    if (workspace_floats < pwc_flow_metrics_workspace_floats(N, H, W)) return PWC_EINVAL;
    const int parts = (int)masked_parts(H, W);
    FlowMetricsArgs a;
    a.pred = pred; a.gt = gt; a.valid = valid; a.partial = workspace; a.pred_cs = pred_cs; a.gt_cs = gt_cs; a.npix = H * W;
    hipLaunchKernelGGL(flow_metrics_partial_kernel, dim3((unsigned)parts, (unsigned)N), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(flow_metrics_final_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       (const float*)workspace, parts, N, out);
    return pwc_launch_status();
}
