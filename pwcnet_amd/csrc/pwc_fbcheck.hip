// pwc_fbcheck.hip -- forward-backward consistency of two flows: the occlusion masks of label-free training (gfx950; C ABI in
// include/pwc_hip.h, "occlusion").
//
//   pwc_fb_valid_u8   per pixel of both directions 0 / 1: the pixel passes its input mask, its sample point lies inside the
//                     frame, and the flow it carries is undone by the other direction's flow sampled where it points to --
//                     |f + g|^2 <= alpha1 (|f|^2 + |g|^2) + alpha2 (UnFlow); per image and direction the number of such pixels
//
// Direction a reads flow_a at the pixel (f) and flow_b at the pixel moved by f (g); direction b the same with the roles swapped.
// The in-frame test and the bilinear sample are photo_pixel's of pwc_unsup.hip.  A pixel the input mask rules out reads neither
// flow, an out-of-frame one no sample.  Sample point, weights, the difference and both sides of the comparison are computed in
// double (a few dozen operations per pixel of a kernel that waits for memory), so the decision is that of a float64 restatement
// except at true near-ties.  The comparison is written `rhs - lhs >= 0`: the same decision as `lhs <= rhs` for finite values,
// false for a NaN on either side, and false for Inf on both (an Inf in the sampled flow).
// One launch for both directions (blockIdx.z), one lane per pixel, grid-stride over the parts of loss_common.h; flows at any
// channel stride >= 2: scalar loads, no alignment asked.  The masks are a gather; the counts are added in the fixed tree and in
// index order (pwc_loss_write_part, pwc_loss_final_kernel): no atomics, two calls give the same bits.
#include "loss_common.h"

struct FbArgs {
    const float* flow_a;      // the flow 0 -> 1
    const float* flow_b;      // the flow 1 -> 0
    const uint8_t* in_a;      // [N][H][W] input masks, null: every pixel
    const uint8_t* in_b;
    uint8_t* out_a;           // [N][H][W] 0 / 1
    uint8_t* out_b;
    float* block_a;           // per direction [N][parts] float (unused sums: 0), [N][parts] int32 counts -- pwc_loss_final_launch's
    float* block_b;
    int a_cs, b_cs;
    int N, H, W;
    float flow_scale, alpha1, alpha2;
};

// Pixel (n, y, x), pix = its flat index, of the direction whose own flow is `own` and whose opposite flow is `other`.  The
// in-frame test is what keeps the four corner reads inside image n: 0 <= x0 <= x1 <= W - 1 and the same in y follow from it.
__device__ __forceinline__ bool fb_pixel(const float* own, int own_cs, const float* other, int other_cs, const uint8_t* in, int n,
                                         int y, int x, size_t pix, int H, int W, double scale, double alpha1, double alpha2) {
    if (in && !in[pix]) return false;
    const float* fp = own + pix * own_cs;
    const double f0 = (double)fp[0] * scale, f1 = (double)fp[1] * scale;
    const double px = (double)x + f0, py = (double)y + f1;
    // (every comparison is false for a NaN; an Inf fails one of them)
    if (!(px >= 0.0 && px <= (double)(W - 1) && py >= 0.0 && py <= (double)(H - 1))) return false;
    const double fx0 = floor(px), fy0 = floor(py);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const double wx1 = px - fx0, wy1 = py - fy0, wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
    const size_t img = (size_t)n * H * W;
    const float* p00 = other + (img + (size_t)y0 * W + x0) * other_cs;
    const float* p01 = other + (img + (size_t)y0 * W + x1) * other_cs;
    const float* p10 = other + (img + (size_t)y1 * W + x0) * other_cs;
    const float* p11 = other + (img + (size_t)y1 * W + x1) * other_cs;
    double g[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const double top = wx0 * (double)p00[c] + wx1 * (double)p01[c], bot = wx0 * (double)p10[c] + wx1 * (double)p11[c];
        g[c] = scale * (wy0 * top + wy1 * bot);
    }
    const double d0 = f0 + g[0], d1 = f1 + g[1];
    const double lhs = d0 * d0 + d1 * d1;
    const double rhs = alpha1 * (f0 * f0 + f1 * f1 + g[0] * g[0] + g[1] * g[1]) + alpha2;
    return rhs - lhs >= 0.0;
}

template <bool COUNTS>
__global__ __launch_bounds__(256) void fb_valid_kernel(const FbArgs a) {
    const int n = blockIdx.y;
    const bool fwd = blockIdx.z == 0;
    const float* own = fwd ? a.flow_a : a.flow_b;
    const float* other = fwd ? a.flow_b : a.flow_a;
    const int own_cs = fwd ? a.a_cs : a.b_cs, other_cs = fwd ? a.b_cs : a.a_cs;
    const uint8_t* in = fwd ? a.in_a : a.in_b;
    uint8_t* out = fwd ? a.out_a : a.out_b;
    const int npix = a.H * a.W;
    const double scale = (double)a.flow_scale, alpha1 = (double)a.alpha1, alpha2 = (double)a.alpha2;
    int cnt = 0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
        const int y = p / a.W, x = p - y * a.W;
        const size_t pix = (size_t)n * npix + p;
        const bool ok = fb_pixel(own, own_cs, other, other_cs, in, n, y, x, pix, a.H, a.W, scale, alpha1, alpha2);
        out[pix] = ok ? 1 : 0;
        cnt += ok ? 1 : 0;
    }
    if (COUNTS) {
        float* block = fwd ? a.block_a : a.block_b;
        pwc_loss_write_part<true>(0.f, cnt, block, reinterpret_cast<int*>(block + (size_t)a.N * gridDim.x));
    }
}

// per direction: a float sum (unused, 0) and an int32 count per part, and the N floats the final sum writes its sums to
static inline size_t fb_block_floats(int N, int H, int W) { return pwc_loss_workspace_floats(N, H, W, 2) + (size_t)N; }

extern "C" size_t pwc_fb_workspace_floats(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * fb_block_floats(N, H, W);
}

extern "C" int pwc_fb_valid_u8(const float* flow_a, int a_cs, const float* flow_b, int b_cs, float flow_scale,
                               const uint8_t* valid_a_in, const uint8_t* valid_b_in, int N, int H, int W, float alpha1,
                               float alpha2, uint8_t* valid_a, uint8_t* valid_b, int32_t* counts_a, int32_t* counts_b,
                               float* workspace, size_t workspace_floats, pwc_stream_t stream) {
    if (!flow_a || !flow_b || !valid_a || N <= 0 || H <= 0 || W <= 0 || a_cs < 2 || b_cs < 2) return PWC_EINVAL;
    if (!(alpha1 >= 0.f) || !(alpha2 >= 0.f)) return PWC_EINVAL;           // (a NaN fails both)
    if (counts_b && !valid_b) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    const bool counts = counts_a || counts_b;
    if (counts && (!workspace || workspace_floats < pwc_fb_workspace_floats(N, H, W))) return PWC_EINVAL;
    const int parts = (int)pwc_loss_parts(H, W);
    FbArgs a;
    a.flow_a = flow_a; a.flow_b = flow_b; a.in_a = valid_a_in; a.in_b = valid_b_in; a.out_a = valid_a; a.out_b = valid_b;
    a.block_a = counts ? workspace : nullptr;
    a.block_b = counts ? workspace + fb_block_floats(N, H, W) : nullptr;
    a.a_cs = a_cs; a.b_cs = b_cs; a.N = N; a.H = H; a.W = W;
    a.flow_scale = flow_scale; a.alpha1 = alpha1; a.alpha2 = alpha2;
    const dim3 grid((unsigned)parts, (unsigned)N, valid_b ? 2u : 1u);
    if (counts)
        hipLaunchKernelGGL(fb_valid_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(fb_valid_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    const size_t sums_at = pwc_loss_workspace_floats(N, H, W, 2);
    if (counts_a) pwc_loss_final_launch(a.block_a, parts, N, a.block_a + sums_at, counts_a, stream);
    if (counts_b) pwc_loss_final_launch(a.block_b, parts, N, a.block_b + sums_at, counts_b, stream);
    return pwc_launch_status();
}
