// pwc_unsup.hip -- label-free losses on the flow: the photometric warp term and the edge-aware smoothness term, forward sums
// and the gradient with respect to the flow (gfx950; C ABI in include/pwc_hip.h, "self-supervised losses").
//
//   pwc_photometric_sums_f32       per-image sums over the contributing pixels of sum_c rho(images_0 - warp(images_1, flow)), and
//                                  the number of contributing pixels
//   pwc_photometric_grad_f32       the gradient of those sums w.r.t. the flow, times an upstream gradient per image
//   pwc_flow_smoothness_sums_f32   per-image sums of w * rho(forward difference of the flow), w = exp(-alpha * mean_c |d image|)
//   pwc_flow_smoothness_grad_f32   their gradient w.r.t. the flow
//   pwc_flow_smoothness2_sums_f32  the same with the SECOND difference of the flow, weighted by the image difference across the
//   pwc_flow_smoothness2_grad_f32  centre (end of the file)
//
// rho(d) = (d^2 + eps^2)^q (generalised Charbonnier), rho'(d) = 2 q d (d^2 + eps^2)^(q - 1).  The images are constants.
// A pixel of the photometric term contributes iff it is valid and its sample point lies inside the frame; the others are
// selected out as in pwc_flow_loss.hip: a masked pixel reads neither its flow nor an image, an out-of-frame one no image.
// rho' turns a rounding error of d into one of up to 1 / eps times its size in the gradient, so the sample point, the bilinear
// weights and the difference d are computed in double (a few dozen operations per pixel of kernels that wait for memory) and d is
// rounded to fp32 once: the gradient then carries fp32's RELATIVE error.  Images have 1..4 channels at any channel stride:
// scalar loads, no alignment asked.  Sums: every workgroup adds its pixels in a fixed tree and writes one partial, one thread
// per image adds the partials in index order -- two calls give the same bits.  The gradients are gathers, one lane per pixel.
// Partition, tree, final sum, rho and the gradients' pixel walk and store are those of loss_common.h.
#include "loss_common.h"

// ------------------------------------------------------------------ photometric term
struct PhotoArgs {
    const float* im0;
    const float* im1;
    const float* flow;
    const uint8_t* valid;    // [N][H][W], null: every pixel
    const float* dsums;      // [N] upstream gradient (grad)
    float* dflow;            // 2 channels, written or accumulated (grad)
    float* partial;          // [N][gridDim.x] sums
    int* partial_n;          // [N][gridDim.x] counts of contributing pixels
    int im0_cs, im1_cs, flow_cs, dflow_cs;
    int N, H, W;
    float flow_scale, eps2, q;
    int accumulate;
};

// Pixel (n, y, x), pix = its flat index: does it contribute, and if so d[c] = images_0 - bilinear sample of images_1 and
// (GRAD) gx[c], gy[c] = the sample's derivative along x and y (floor and clip carry none).  The in-frame test is what keeps
// the four corner reads inside image n: 0 <= x0 <= x1 <= W - 1 and the same in y follow from it.
template <int C, bool GRAD>
__device__ __forceinline__ bool photo_pixel(const PhotoArgs& a, int n, int y, int x, size_t pix, float* d, float* gx, float* gy) {
    if (a.valid && !a.valid[pix]) return false;
    const float* fp = a.flow + pix * a.flow_cs;
    const double px = (double)x + (double)fp[0] * (double)a.flow_scale, py = (double)y + (double)fp[1] * (double)a.flow_scale;
    // (every comparison is false for a NaN; an Inf fails one of them)
    if (!(px >= 0.0 && px <= (double)(a.W - 1) && py >= 0.0 && py <= (double)(a.H - 1))) return false;
    // (pwc_bilinear_f64's table, written out: with the struct photometric_grad_kernel<3> needs 68 VGPRs and loses a wave per SIMD)
    const double fx0 = floor(px), fy0 = floor(py);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int x1 = min(x0 + 1, a.W - 1), y1 = min(y0 + 1, a.H - 1);
    const double wx1 = px - fx0, wy1 = py - fy0, wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
    const size_t img = (size_t)n * a.H * a.W;
    const float* p00 = a.im1 + (img + (size_t)y0 * a.W + x0) * a.im1_cs;
    const float* p01 = a.im1 + (img + (size_t)y0 * a.W + x1) * a.im1_cs;
    const float* p10 = a.im1 + (img + (size_t)y1 * a.W + x0) * a.im1_cs;
    const float* p11 = a.im1 + (img + (size_t)y1 * a.W + x1) * a.im1_cs;
    const float* p0 = a.im0 + pix * a.im0_cs;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float v00 = p00[c], v01 = p01[c], v10 = p10[c], v11 = p11[c];
        const double top = wx0 * (double)v00 + wx1 * (double)v01, bot = wx0 * (double)v10 + wx1 * (double)v11;
        d[c] = (float)((double)p0[c] - (wy0 * top + wy1 * bot));
        if (GRAD) {
            gx[c] = (float)wy0 * (v01 - v00) + (float)wy1 * (v11 - v10);
            gy[c] = (float)wx0 * (v10 - v00) + (float)wx1 * (v11 - v01);
        }
    }
    return true;
}

template <int C>
__global__ __launch_bounds__(256) void photometric_partial_kernel(const PhotoArgs a) {
    const int n = blockIdx.y;
    const int npix = a.H * a.W;
    float s = 0.f;
    int cnt = 0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
        const int y = p / a.W, x = p - y * a.W;
        float d[C];
        if (photo_pixel<C, false>(a, n, y, x, (size_t)n * npix + p, d, nullptr, nullptr)) {
            float t = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) t += unsup_rho(d[c], a.eps2, a.q);
            s += t;
            ++cnt;
        }
    }
    pwc_loss_write_part<true>(s, cnt, a.partial, a.partial_n);
}

template <int C>
__global__ __launch_bounds__(256) void photometric_grad_kernel(const PhotoArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel px = pwc_loss_pixel(p, a.H, a.W);
        float* o = a.dflow + p * a.dflow_cs;
        float d[C], gx[C], gy[C];
        if (!photo_pixel<C, true>(a, px.n, px.y, px.x, (size_t)p, d, gx, gy)) {
            pwc_grad_skip2(o, a.accumulate);
            continue;
        }
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float rg = unsup_rho_grad(d[c], a.eps2, a.q);   // d = images_0 - sample: d(d)/d(px) = -gx
            sx -= rg * gx[c];
            sy -= rg * gy[c];
        }
        // (the products are rounded on their own: accumulate adds exactly what a plain call writes)
        const float up = a.dsums[px.n] * a.flow_scale;
        pwc_grad_store2(o, a.accumulate, 1.f, pwc_mul_rounded(up, sx), pwc_mul_rounded(up, sy));
    }
}

static int photo_check(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs, int N, int H,
                       int W, int C, float eps, float q) {
    if (!im0 || !im1 || !flow || N <= 0 || H <= 0 || W <= 0) return PWC_EINVAL;
    if (C < 1 || C > 4) return PWC_EUNSUPPORTED;
    if (im0_cs < C || im1_cs < C || flow_cs < 2) return PWC_EINVAL;
    if (!(eps > 0.f) || !(q > 0.f && q <= 1.f)) return PWC_EINVAL;
    return PWC_OK;
}

// a float sum and an int32 count per part
extern "C" size_t pwc_photometric_workspace_floats(int N, int H, int W) { return pwc_loss_workspace_floats(N, H, W, 2); }

extern "C" int pwc_photometric_sums_f32(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                                        float flow_scale, const uint8_t* valid, int N, int H, int W, int C, float eps, float q,
                                        float* workspace, size_t workspace_floats, float* out_sums, int32_t* out_counts,
                                        pwc_stream_t stream) {
    int rc = photo_check(im0, im0_cs, im1, im1_cs, flow, flow_cs, N, H, W, C, eps, q);
    if (rc == PWC_OK) rc = pwc_loss_sums_check(N, H, W, 2, workspace_floats);
    if (rc != PWC_OK) return rc;
    if (!workspace || !out_sums || !out_counts) return PWC_EINVAL;
    const int parts = (int)pwc_loss_parts(H, W);
    PhotoArgs a;
    a.im0 = im0; a.im1 = im1; a.flow = flow; a.valid = valid; a.dsums = nullptr; a.dflow = nullptr;
    a.partial = workspace; a.partial_n = reinterpret_cast<int*>(workspace + (size_t)N * parts);
    a.im0_cs = im0_cs; a.im1_cs = im1_cs; a.flow_cs = flow_cs; a.dflow_cs = 0;
    a.N = N; a.H = H; a.W = W; a.flow_scale = flow_scale; a.eps2 = eps * eps; a.q = q; a.accumulate = 0;
    const dim3 grid((unsigned)parts, (unsigned)N);
    switch (C) {
    case 1: hipLaunchKernelGGL(photometric_partial_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL(photometric_partial_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 3: hipLaunchKernelGGL(photometric_partial_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL(photometric_partial_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    }
    pwc_loss_final_launch(workspace, parts, N, out_sums, out_counts, stream);
    return pwc_launch_status();
}

extern "C" int pwc_photometric_grad_f32(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                                        float flow_scale, const uint8_t* valid, int N, int H, int W, int C, float eps, float q,
                                        const float* dsums, float* dflow, int dflow_cs, int accumulate, pwc_stream_t stream) {
    const int rc = photo_check(im0, im0_cs, im1, im1_cs, flow, flow_cs, N, H, W, C, eps, q);
    if (rc != PWC_OK) return rc;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (!dsums || !dflow || dflow_cs < 2) return PWC_EINVAL;
    PhotoArgs a;
    a.im0 = im0; a.im1 = im1; a.flow = flow; a.valid = valid; a.dsums = dsums; a.dflow = dflow;
    a.partial = nullptr; a.partial_n = nullptr;
    a.im0_cs = im0_cs; a.im1_cs = im1_cs; a.flow_cs = flow_cs; a.dflow_cs = dflow_cs;
    a.N = N; a.H = H; a.W = W; a.flow_scale = flow_scale; a.eps2 = eps * eps; a.q = q; a.accumulate = accumulate;
    const dim3 grid = pwc_loss_grad_blocks(N, H, W);
    switch (C) {
    case 1: hipLaunchKernelGGL(photometric_grad_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL(photometric_grad_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 3: hipLaunchKernelGGL(photometric_grad_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL(photometric_grad_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    }
    return pwc_launch_status();
}

// ------------------------------------------------------------------ smoothness term
struct SmoothArgs {
    const float* flow;
    const float* image;      // null: every weight is 1
    const float* dsums;      // [N] upstream gradient (grad)
    float* dflow;            // (grad)
    float* partial;          // [N][gridDim.x]
    int flow_cs, image_cs, dflow_cs;
    int N, H, W, C;
    float alpha, eps2, q;
    int accumulate;
};

// weight of the difference between the pixels with flat indices pa and pb: exp(-alpha * mean_c |image[pb] - image[pa]|)
__device__ __forceinline__ float smooth_weight(const SmoothArgs& a, size_t pa, size_t pb) {
    if (!a.image) return 1.f;
    const float* ia = a.image + pa * a.image_cs;
    const float* ib = a.image + pb * a.image_cs;
    float s = 0.f;
    for (int c = 0; c < a.C; ++c) s += fabsf(ib[c] - ia[c]);
    return expf(-a.alpha * (s / (float)a.C));
}

__global__ __launch_bounds__(256) void flow_smoothness_partial_kernel(const SmoothArgs a) {
    const int n = blockIdx.y;
    const int npix = a.H * a.W;
    float s = 0.f;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
        const int y = p / a.W, x = p - y * a.W;
        const size_t pix = (size_t)n * npix + p;
        const float* f = a.flow + pix * a.flow_cs;
        const float u = f[0], v = f[1];
        if (x < a.W - 1) {
            const float* g = f + a.flow_cs;
            s += smooth_weight(a, pix, pix + 1) * (unsup_rho(g[0] - u, a.eps2, a.q) + unsup_rho(g[1] - v, a.eps2, a.q));
        }
        if (y < a.H - 1) {
            const float* g = f + (size_t)a.W * a.flow_cs;
            s += smooth_weight(a, pix, pix + a.W) * (unsup_rho(g[0] - u, a.eps2, a.q) + unsup_rho(g[1] - v, a.eps2, a.q));
        }
    }
    pwc_loss_write_part<false>(s, 0, a.partial, nullptr);
}

__global__ __launch_bounds__(256) void flow_smoothness_grad_kernel(const SmoothArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel px = pwc_loss_pixel(p, a.H, a.W);
        const int x = px.x, y = px.y;
        const float* f = a.flow + p * a.flow_cs;
        const float u = f[0], v = f[1];
        float gu = 0.f, gv = 0.f;
        // the up to four differences that touch this pixel: its own (it is the subtrahend) and its left / upper neighbour's
        if (x < a.W - 1) {
            const float* g = f + a.flow_cs;
            const float w = smooth_weight(a, (size_t)p, (size_t)p + 1);
            gu -= w * unsup_rho_grad(g[0] - u, a.eps2, a.q);
            gv -= w * unsup_rho_grad(g[1] - v, a.eps2, a.q);
        }
        if (x > 0) {
            const float* g = f - a.flow_cs;
            const float w = smooth_weight(a, (size_t)p - 1, (size_t)p);
            gu += w * unsup_rho_grad(u - g[0], a.eps2, a.q);
            gv += w * unsup_rho_grad(v - g[1], a.eps2, a.q);
        }
        if (y < a.H - 1) {
            const float* g = f + (size_t)a.W * a.flow_cs;
            const float w = smooth_weight(a, (size_t)p, (size_t)p + a.W);
            gu -= w * unsup_rho_grad(g[0] - u, a.eps2, a.q);
            gv -= w * unsup_rho_grad(g[1] - v, a.eps2, a.q);
        }
        if (y > 0) {
            const float* g = f - (size_t)a.W * a.flow_cs;
            const float w = smooth_weight(a, (size_t)p - a.W, (size_t)p);
            gu += w * unsup_rho_grad(u - g[0], a.eps2, a.q);
            gv += w * unsup_rho_grad(v - g[1], a.eps2, a.q);
        }
        const float up = a.dsums[px.n];
        pwc_grad_store2(a.dflow + p * a.dflow_cs, a.accumulate, 1.f, pwc_mul_rounded(up, gu), pwc_mul_rounded(up, gv));
    }
}

static int smooth_check(const float* flow, int flow_cs, const float* image, int image_cs, int C, float alpha, float eps, float q,
                        int N, int H, int W) {
    if (!flow || N <= 0 || H <= 0 || W <= 0 || flow_cs < 2) return PWC_EINVAL;
    if (image && (C < 1 || C > 4)) return PWC_EUNSUPPORTED;
    if (image && image_cs < C) return PWC_EINVAL;
    if (!(eps > 0.f) || !(q > 0.f && q <= 1.f) || !(alpha >= 0.f)) return PWC_EINVAL;
    return PWC_OK;
}

extern "C" size_t pwc_flow_smoothness_workspace_floats(int N, int H, int W) { return pwc_loss_workspace_floats(N, H, W, 1); }

extern "C" int pwc_flow_smoothness_sums_f32(const float* flow, int flow_cs, const float* image, int image_cs, int C, float alpha,
                                            float eps, float q, int N, int H, int W, float* workspace, size_t workspace_floats,
                                            float* out_sums, pwc_stream_t stream) {
    int rc = smooth_check(flow, flow_cs, image, image_cs, C, alpha, eps, q, N, H, W);
    if (rc == PWC_OK) rc = pwc_loss_sums_check(N, H, W, 1, workspace_floats);
    if (rc != PWC_OK) return rc;
    if (!workspace || !out_sums) return PWC_EINVAL;
    const int parts = (int)pwc_loss_parts(H, W);
    SmoothArgs a;
    a.flow = flow; a.image = image; a.dsums = nullptr; a.dflow = nullptr; a.partial = workspace;
    a.flow_cs = flow_cs; a.image_cs = image_cs; a.dflow_cs = 0;
    a.N = N; a.H = H; a.W = W; a.C = C; a.alpha = alpha; a.eps2 = eps * eps; a.q = q; a.accumulate = 0;
    hipLaunchKernelGGL(flow_smoothness_partial_kernel, dim3((unsigned)parts, (unsigned)N), dim3(256), 0, (hipStream_t)stream, a);
    pwc_loss_final_launch(workspace, parts, N, out_sums, nullptr, stream);
    return pwc_launch_status();
}

extern "C" int pwc_flow_smoothness_grad_f32(const float* flow, int flow_cs, const float* image, int image_cs, int C, float alpha,
                                            float eps, float q, int N, int H, int W, const float* dsums, float* dflow,
                                            int dflow_cs, int accumulate, pwc_stream_t stream) {
    const int rc = smooth_check(flow, flow_cs, image, image_cs, C, alpha, eps, q, N, H, W);
    if (rc != PWC_OK) return rc;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (!dsums || !dflow || dflow_cs < 2) return PWC_EINVAL;
    SmoothArgs a;
    a.flow = flow; a.image = image; a.dsums = dsums; a.dflow = dflow; a.partial = nullptr;
    a.flow_cs = flow_cs; a.image_cs = image_cs; a.dflow_cs = dflow_cs;
    a.N = N; a.H = H; a.W = W; a.C = C; a.alpha = alpha; a.eps2 = eps * eps; a.q = q; a.accumulate = accumulate;
    hipLaunchKernelGGL(flow_smoothness_grad_kernel, pwc_loss_grad_blocks(N, H, W), dim3(256), 0, (hipStream_t)stream, a);
    return pwc_launch_status();
}

// ------------------------------------------------------------------ smoothness term, second order
// Centre c of a second difference along an axis (step = 1 along x, W along y; the neighbours are c - step and c + step, the
// caller keeps them inside the row / column): the weight and the two differences l - 2 c + r.  The three fp32 values add
// exactly in double and the difference is rounded to fp32 once -- the flow's magnitude (hundreds of px where it leaves the
// frame) does not reach rho' through a rounding of the difference.
__device__ __forceinline__ float smooth2_diffs(const SmoothArgs& a, size_t c, size_t step, float& du, float& dv) {
    const float* fc = a.flow + c * a.flow_cs;
    const float* fl = fc - step * a.flow_cs;
    const float* fr = fc + step * a.flow_cs;
    du = (float)(((double)fl[0] - 2.0 * (double)fc[0]) + (double)fr[0]);
    dv = (float)(((double)fl[1] - 2.0 * (double)fc[1]) + (double)fr[1]);
    return smooth_weight(a, c - step, c + step);
}

__global__ __launch_bounds__(256) void flow_smoothness2_partial_kernel(const SmoothArgs a) {
    const int n = blockIdx.y;
    const int npix = a.H * a.W;
    float s = 0.f;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
        const int y = p / a.W, x = p - y * a.W;
        const size_t pix = (size_t)n * npix + p;
        float du, dv;
        if (x > 0 && x < a.W - 1) {
            const float w = smooth2_diffs(a, pix, 1, du, dv);
            s += w * (unsup_rho(du, a.eps2, a.q) + unsup_rho(dv, a.eps2, a.q));
        }
        if (y > 0 && y < a.H - 1) {
            const float w = smooth2_diffs(a, pix, (size_t)a.W, du, dv);
            s += w * (unsup_rho(du, a.eps2, a.q) + unsup_rho(dv, a.eps2, a.q));
        }
    }
    pwc_loss_write_part<false>(s, 0, a.partial, nullptr);
}

// gu, gv += factor * w * rho'(the second difference centred on c)
__device__ __forceinline__ void smooth2_gather(const SmoothArgs& a, size_t c, size_t step, float factor, float& gu, float& gv) {
    float du, dv;
    const float w = factor * smooth2_diffs(a, c, step, du, dv);
    gu += w * unsup_rho_grad(du, a.eps2, a.q);
    gv += w * unsup_rho_grad(dv, a.eps2, a.q);
}

__global__ __launch_bounds__(256) void flow_smoothness2_grad_kernel(const SmoothArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel px = pwc_loss_pixel(p, a.H, a.W);
        const int x = px.x, y = px.y;
        const size_t c = (size_t)p, row = (size_t)a.W;
        float gu = 0.f, gv = 0.f;
        // the up to six second differences that touch this pixel: per axis it is the right neighbour of the centre before it,
        // the centre itself (factor -2) and the left neighbour of the centre behind it; a centre keeps 1 from both borders
        if (x >= 2) smooth2_gather(a, c - 1, 1, 1.f, gu, gv);
        if (x >= 1 && x <= a.W - 2) smooth2_gather(a, c, 1, -2.f, gu, gv);
        if (x <= a.W - 3) smooth2_gather(a, c + 1, 1, 1.f, gu, gv);
        if (y >= 2) smooth2_gather(a, c - row, row, 1.f, gu, gv);
        if (y >= 1 && y <= a.H - 2) smooth2_gather(a, c, row, -2.f, gu, gv);
        if (y <= a.H - 3) smooth2_gather(a, c + row, row, 1.f, gu, gv);
        const float up = a.dsums[px.n];
        pwc_grad_store2(a.dflow + p * a.dflow_cs, a.accumulate, 1.f, pwc_mul_rounded(up, gu), pwc_mul_rounded(up, gv));
    }
}

extern "C" int pwc_flow_smoothness2_sums_f32(const float* flow, int flow_cs, const float* image, int image_cs, int C, float alpha,
                                             float eps, float q, int N, int H, int W, float* workspace, size_t workspace_floats,
                                             float* out_sums, pwc_stream_t stream) {
    int rc = smooth_check(flow, flow_cs, image, image_cs, C, alpha, eps, q, N, H, W);
    if (rc == PWC_OK) rc = pwc_loss_sums_check(N, H, W, 1, workspace_floats);
    if (rc != PWC_OK) return rc;
    if (!workspace || !out_sums) return PWC_EINVAL;
    const int parts = (int)pwc_loss_parts(H, W);
    SmoothArgs a;
    a.flow = flow; a.image = image; a.dsums = nullptr; a.dflow = nullptr; a.partial = workspace;
    a.flow_cs = flow_cs; a.image_cs = image_cs; a.dflow_cs = 0;
    a.N = N; a.H = H; a.W = W; a.C = C; a.alpha = alpha; a.eps2 = eps * eps; a.q = q; a.accumulate = 0;
    hipLaunchKernelGGL(flow_smoothness2_partial_kernel, dim3((unsigned)parts, (unsigned)N), dim3(256), 0, (hipStream_t)stream, a);
    pwc_loss_final_launch(workspace, parts, N, out_sums, nullptr, stream);
    return pwc_launch_status();
}

extern "C" int pwc_flow_smoothness2_grad_f32(const float* flow, int flow_cs, const float* image, int image_cs, int C, float alpha,
                                             float eps, float q, int N, int H, int W, const float* dsums, float* dflow,
                                             int dflow_cs, int accumulate, pwc_stream_t stream) {
    const int rc = smooth_check(flow, flow_cs, image, image_cs, C, alpha, eps, q, N, H, W);
    if (rc != PWC_OK) return rc;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (!dsums || !dflow || dflow_cs < 2) return PWC_EINVAL;
    SmoothArgs a;
    a.flow = flow; a.image = image; a.dsums = dsums; a.dflow = dflow; a.partial = nullptr;
    a.flow_cs = flow_cs; a.image_cs = image_cs; a.dflow_cs = dflow_cs;
    a.N = N; a.H = H; a.W = W; a.C = C; a.alpha = alpha; a.eps2 = eps * eps; a.q = q; a.accumulate = accumulate;
    hipLaunchKernelGGL(flow_smoothness2_grad_kernel, pwc_loss_grad_blocks(N, H, W), dim3(256), 0, (hipStream_t)stream, a);
    return pwc_launch_status();
}
