// pwc_flow_loss.hip -- the supervised losses on the flow and the flow metrics, dense or under a validity mask (sparse ground
// truth) (gfx950; C ABI in include/pwc_hip.h, "losses" and "sparse ground truth").
//
//   pwc_flow_norm_sums_f32          per-image sums of ||pred - gt / gt_div||_ord          losses.py:4-13,15-48
//   pwc_flow_norm_grad_f32          the gradient of those sums w.r.t. pred               losses.py:4-8 inside :20-29,38-45
//   pwc_flow_norm_masked_sums_f32   the sums over the VALID pixels, and their number
//   pwc_flow_norm_masked_grad_f32   their gradient; invalid pixels get 0 (or stay as they are)
//   pwc_flow_metrics_f32            EPE sums, KITTI outliers, 1/3/5-px error counts, EPE by motion magnitude
//
// reference losses.py:4-13 (L1loss / L2loss / EPE) and the per-level term of multiscale_loss / multirobust_loss
// (losses.py:15-48): sum over the pixels of image n of
//     || pred[n,y,x,0:2] - gt[n, floor(y*GH/H), floor(x*GW/W), 0:2] / gt_div ||_ord ,  ord in {1, 2}
// -- tf.image.resize_nearest_neighbor is folded into the read; GH = H, GW = W, gt_div = 1: plain norm of the difference.
// The mask is one byte per pixel of the GROUND TRUTH, non-zero = valid, read at the nearest-neighbour index the ground truth is
// read at (tf.image.resize_nearest_neighbor of the mask).  Invalid pixels are selected out, not multiplied out: neither pred nor
// gt is read there, so NaN, Inf or the .flo sentinel 1e10 at an invalid pixel cannot reach a sum or a gradient.
// The dense and the masked form are the two instantiations of one kernel each (MASKED), on the per-pixel arithmetic, the
// partition of the pixels and the order of additions of loss_common.h: under an all-ones mask the masked form returns the dense
// form's bits (tests/test_gpu_masked_loss.py).
#include "loss_common.h"

// ------------------------------------------------------------------ loss sums
struct FlowNormArgs {
    const float* pred;
    const float* gt;
    const uint8_t* valid;    // [N][GH][GW] (MASKED)
    float* partial;          // [N][gridDim.x] sums
    int* partial_n;          // [N][gridDim.x] valid-pixel counts (MASKED)
    int pred_cs, gt_cs;
    int H, W, GH, GW;
    float sy, sx, gt_div;
    int ord;
};

template <bool MASKED>
__global__ __launch_bounds__(256) void flow_norm_partial_kernel(const FlowNormArgs a) {
    const int n = blockIdx.y;
    const int npix = a.H * a.W;
    float s = 0.f;
    int cnt = 0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
        const int y = p / a.W, x = p - y * a.W;
        const size_t g = ((size_t)n * a.GH + pwc_nearest_index(y, a.sy, a.GH)) * a.GW + pwc_nearest_index(x, a.sx, a.GW);
        if (MASKED && !a.valid[g]) continue;
        const float* pp = a.pred + ((size_t)n * npix + p) * a.pred_cs;
        const float* gp = a.gt + g * a.gt_cs;
        s += pwc_norm_term(pwc_flow_diff(pp[0], gp[0], a.gt_div), pwc_flow_diff(pp[1], gp[1], a.gt_div), a.ord);
        ++cnt;
    }
    pwc_loss_write_part<MASKED>(s, cnt, a.partial, a.partial_n);
}

template <bool MASKED>
static int flow_norm_sums(const float* pred, int pred_cs, const float* gt, int gt_cs, const uint8_t* valid, int N, int H, int W,
                          int GH, int GW, float gt_div, int ord, float* workspace, size_t workspace_floats, float* out_sums,
                          int32_t* out_counts, pwc_stream_t stream) {
    if (!pred || !gt || !workspace || !out_sums || (MASKED && (!valid || !out_counts))) return PWC_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || GH <= 0 || GW <= 0 || pred_cs < 2 || gt_cs < 2) return PWC_EINVAL;
    if (ord != 1 && ord != 2) return PWC_EUNSUPPORTED;
    if (!(gt_div != 0.f)) return PWC_EINVAL;
    const int rc = pwc_loss_sums_check(N, H, W, MASKED ? 2 : 1, workspace_floats);
    if (rc != PWC_OK) return rc;
    const int parts = (int)pwc_loss_parts(H, W);
    FlowNormArgs a;
    a.pred = pred; a.gt = gt; a.valid = valid; a.partial = workspace;
    a.partial_n = reinterpret_cast<int*>(workspace + (size_t)N * parts);
    a.pred_cs = pred_cs; a.gt_cs = gt_cs;
    a.H = H; a.W = W; a.GH = GH; a.GW = GW;
    a.sy = (float)GH / (float)H; a.sx = (float)GW / (float)W; a.gt_div = gt_div; a.ord = ord;
    hipLaunchKernelGGL(flow_norm_partial_kernel<MASKED>, dim3((unsigned)parts, (unsigned)N), dim3(256), 0, (hipStream_t)stream, a);
    pwc_loss_final_launch(workspace, parts, N, out_sums, out_counts, stream);
    return pwc_launch_status();
}

extern "C" size_t pwc_flow_norm_workspace_floats(int N, int H, int W) { return pwc_loss_workspace_floats(N, H, W, 1); }
// a float sum and an int32 count per part
extern "C" size_t pwc_flow_norm_masked_workspace_floats(int N, int H, int W) { return pwc_loss_workspace_floats(N, H, W, 2); }

extern "C" int pwc_flow_norm_sums_f32(const float* pred, int pred_cs, const float* gt, int gt_cs, int N, int H, int W,
                                      int GH, int GW, float gt_div, int ord, float* workspace,
                                      size_t workspace_floats, float* out_sums, pwc_stream_t stream) {
    return flow_norm_sums<false>(pred, pred_cs, gt, gt_cs, nullptr, N, H, W, GH, GW, gt_div, ord, workspace, workspace_floats,
                                 out_sums, nullptr, stream);
}

extern "C" int pwc_flow_norm_masked_sums_f32(const float* pred, int pred_cs, const float* gt, int gt_cs, const uint8_t* valid,
                                             int N, int H, int W, int GH, int GW, float gt_div, int ord, float* workspace,
                                             size_t workspace_floats, float* out_sums, int32_t* out_counts, pwc_stream_t stream) {
    return flow_norm_sums<true>(pred, pred_cs, gt, gt_cs, valid, N, H, W, GH, GW, gt_div, ord, workspace, workspace_floats,
                                out_sums, out_counts, stream);
}

// ------------------------------------------------------------------ loss gradient
// d/dpred of  scale * sum_p || pred[p] - gt[nearest(p)] / gt_div ||_ord   (losses.py:4-8 inside :20-29,38-45):
//   ord 2: (pred - g) / ||pred - g||_2   (0 where the norm is 0);   ord 1: sign(pred - g)
struct FlowNormGradArgs {
    const float* pred;
    const float* gt;
    const uint8_t* valid;    // (MASKED)
    float* dpred;
    int pred_cs, gt_cs, dpred_cs;
    int N, H, W, GH, GW;
    float sy, sx, gt_div, scale;
    int ord, accumulate;
};

template <bool MASKED>
__global__ __launch_bounds__(256) void flow_norm_grad_kernel(const FlowNormGradArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel q = pwc_loss_pixel(p, a.H, a.W);
        const long g = ((long)q.n * a.GH + pwc_nearest_index(q.y, a.sy, a.GH)) * a.GW + pwc_nearest_index(q.x, a.sx, a.GW);
        float* d = a.dpred + p * a.dpred_cs;
        if (MASKED && !a.valid[g]) {
            pwc_grad_skip2(d, a.accumulate);
            continue;
        }
        const float* pp = a.pred + p * a.pred_cs;
        const float* gp = a.gt + g * a.gt_cs;
        float ox, oy;
        pwc_norm_direction(pwc_flow_diff(pp[0], gp[0], a.gt_div), pwc_flow_diff(pp[1], gp[1], a.gt_div), a.ord, ox, oy);
        pwc_grad_store2(d, a.accumulate, a.scale, ox, oy);
    }
}

template <bool MASKED>
static int flow_norm_grad(const float* pred, int pred_cs, const float* gt, int gt_cs, const uint8_t* valid, int N, int H, int W,
                          int GH, int GW, float gt_div, int ord, float scale, float* dpred, int dpred_cs, int accumulate,
                          pwc_stream_t stream) {
    if (!pred || !gt || (MASKED && !valid) || !dpred || N <= 0 || H <= 0 || W <= 0 || GH <= 0 || GW <= 0) return PWC_EINVAL;
    if (pred_cs < 2 || gt_cs < 2 || dpred_cs < 2 || !(gt_div != 0.f)) return PWC_EINVAL;
    if (ord != 1 && ord != 2) return PWC_EUNSUPPORTED;
    FlowNormGradArgs a;
    a.pred = pred; a.gt = gt; a.valid = valid; a.dpred = dpred; a.pred_cs = pred_cs; a.gt_cs = gt_cs; a.dpred_cs = dpred_cs;
    a.N = N; a.H = H; a.W = W; a.GH = GH; a.GW = GW;
    a.sy = (float)GH / (float)H; a.sx = (float)GW / (float)W; a.gt_div = gt_div; a.scale = scale; a.ord = ord;
    a.accumulate = accumulate;
    hipLaunchKernelGGL(flow_norm_grad_kernel<MASKED>, pwc_loss_grad_blocks(N, H, W), dim3(256), 0, (hipStream_t)stream, a);
    return pwc_launch_status();
}

extern "C" int pwc_flow_norm_grad_f32(const float* pred, int pred_cs, const float* gt, int gt_cs, int N, int H, int W, int GH,
                                      int GW, float gt_div, int ord, float scale, float* dpred, int dpred_cs,
                                      int accumulate, pwc_stream_t stream) {
    return flow_norm_grad<false>(pred, pred_cs, gt, gt_cs, nullptr, N, H, W, GH, GW, gt_div, ord, scale, dpred, dpred_cs,
                                 accumulate, stream);
}

extern "C" int pwc_flow_norm_masked_grad_f32(const float* pred, int pred_cs, const float* gt, int gt_cs, const uint8_t* valid,
                                             int N, int H, int W, int GH, int GW, float gt_div, int ord, float scale,
                                             float* dpred, int dpred_cs, int accumulate, pwc_stream_t stream) {
    return flow_norm_grad<true>(pred, pred_cs, gt, gt_cs, valid, N, H, W, GH, GW, gt_div, ord, scale, dpred, dpred_cs,
                                accumulate, stream);
}

// ------------------------------------------------------------------ flow metrics
// Per image, over the valid pixels, with e = ||pred - gt||_2 and g = ||gt||_2 (both flows in pixels, one resolution):
//   0 n_valid   1 sum e   2 n(e > 3 && e > 0.05 g) [KITTI Fl]   3 n(e > 1)   4 n(e > 3)   5 n(e > 5)
//   6 n(g < 10)   7 sum e (g < 10)   8 n(10 <= g < 40)   9 sum e (10 <= g < 40)   10 n(g >= 40)   11 sum e (g >= 40)
// One pass: every thread keeps the eight integer counts and the four float sums, a block adds them in the fixed tree and writes
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
    const int n = blockIdx.y;
    float sf[4] = {0.f, 0.f, 0.f, 0.f};            // sum e: all, g < 10, 10 <= g < 40, g >= 40
    int ci[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // n_valid, n_fl, n(e > 1), n(e > 3), n(e > 5), n(g < 10), n(10 <= g < 40), n(g >= 40)
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
    pwc_block_tree_sum<4, 8>(sf, ci);
    if (threadIdx.x == 0) {
        float* o = a.partial + ((size_t)n * gridDim.x + blockIdx.x) * PWC_METRICS;
        int* oi = reinterpret_cast<int*>(o);
        oi[0] = ci[0]; o[1] = sf[0]; oi[2] = ci[1]; oi[3] = ci[2]; oi[4] = ci[3]; oi[5] = ci[4];
        oi[6] = ci[5]; o[7] = sf[1]; oi[8] = ci[6]; o[9] = sf[2]; oi[10] = ci[7]; o[11] = sf[3];
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
    return pwc_loss_workspace_floats(N, H, W, PWC_METRICS);
}

extern "C" int pwc_flow_metrics_f32(const float* pred, int pred_cs, const float* gt, int gt_cs, const uint8_t* valid, int N, int H,
                                    int W, float* workspace, size_t workspace_floats, double* out, pwc_stream_t stream) {
    if (!pred || !gt || !workspace || !out) return PWC_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || pred_cs < 2 || gt_cs < 2) return PWC_EINVAL;
    const int rc = pwc_loss_sums_check(N, H, W, PWC_METRICS, workspace_floats);
    if (rc != PWC_OK) return rc;
    const int parts = (int)pwc_loss_parts(H, W);
    FlowMetricsArgs a;
    a.pred = pred; a.gt = gt; a.valid = valid; a.partial = workspace; a.pred_cs = pred_cs; a.gt_cs = gt_cs; a.npix = H * W;
    hipLaunchKernelGGL(flow_metrics_partial_kernel, dim3((unsigned)parts, (unsigned)N), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(flow_metrics_final_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       (const float*)workspace, parts, N, out);
    return pwc_launch_status();
}
