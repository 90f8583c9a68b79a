// pwc_fbcheck.hip -- forward-backward consistency of two flows: the occlusion masks of label-free training, and (second half of
// the file) the consistency term with its gradient into both flows (gfx950; C ABI in include/pwc_hip.h, "occlusion").
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
    const PwcBilinearF64 bl = pwc_bilinear_f64(px, py, H, W);
    const double wx0 = bl.wx0, wx1 = bl.wx1, wy0 = bl.wy0, wy1 = bl.wy1;
    const size_t img = (size_t)n * H * W;
    const float* p00 = other + (img + bl.o00) * other_cs;
    const float* p01 = other + (img + bl.o01) * other_cs;
    const float* p10 = other + (img + bl.o10) * other_cs;
    const float* p11 = other + (img + bl.o11) * other_cs;
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

// ------------------------------------------------------------------ the consistency term
//   pwc_fb_consistency_sums_f32   per image and direction the sum of rho(e0) + rho(e1), e = f + g as above, over the pixels that
//                                 pass their mask and whose sample point is in frame, and their number
//   pwc_fb_consistency_grad_f32   the gradient of those sums, times an upstream gradient per image and direction, with respect
//                                 to BOTH flows
// e is fb_pixel's d0, d1 (double) rounded to fp32 once; rho and rho' are loss_common.h's.  A direction's pixel reaches its own
// flow where it stands (f and the sample position: a gather) and the other flow at the four corners it samples (a scatter:
// several pixels may share a corner).  The scatter adds corner weight * rho'(e_k) -- without the per-image upstream gradient
// and without flow_scale, which are factored out exactly -- as 64-bit fixed-point integers of 2^-36 steps: integer addition is
// associative, so the sums do not depend on the order in which the atomics land (the precedent is pwc_backward.hip's
// deterministic warp gradient).  Three steps on the stream: the accumulators are zeroed; one launch over the pixels of both
// directions scatters; one launch over the pixels of both FLOWS recomputes the pixel's own gather part, converts its two
// accumulators once, multiplies them by flow_scale * (the other direction's upstream gradient), adds and stores through
// pwc_grad_store2 -- so accumulate adds exactly what a plain call writes.
struct FbcArgs {
    const float* flow_a;
    const float* flow_b;
    const uint8_t* in_a;      // [N][H][W] masks, null: every pixel
    const uint8_t* in_b;
    const float* dsums_a;     // [N] upstream gradients (grad)
    const float* dsums_b;
    float* dflow_a;           // (grad)
    float* dflow_b;
    long long* fix_a;         // (grad) [N][H][W][2] accumulators of what direction b scatters onto flow_a, then flow_a's poison word
    long long* fix_b;
    float* block_a;           // (sums) per direction [N][parts] float sums, [N][parts] int32 counts
    float* block_b;
    int a_cs, b_cs, da_cs, db_cs;
    int N, H, W;
    float flow_scale, eps2, q;
    int accumulate;
};

// What a pixel of one direction holds once it contributes: e (fp32), the flat indices of its four corners in the other flow,
// their weights, and the derivative of the sample (before flow_scale) along x and y, per channel.
struct FbcSample {
    float e[2];
    size_t o00, o01, o10, o11;
    double w00, w01, w10, w11;
    float sx[2], sy[2];
};

// fb_pixel's mask test, in-frame test and sample, word for word; returns whether the pixel contributes.
__device__ __forceinline__ bool fbc_pixel(const float* own, int own_cs, const float* other, int other_cs, const uint8_t* in, int n,
                                          int y, int x, size_t pix, int H, int W, double scale, FbcSample& s) {
    if (in && !in[pix]) return false;
    const float* fp = own + pix * own_cs;
    const double f0 = (double)fp[0] * scale, f1 = (double)fp[1] * scale;
    const double px = (double)x + f0, py = (double)y + f1;
    // (every comparison is false for a NaN; an Inf fails one of them)
    if (!(px >= 0.0 && px <= (double)(W - 1) && py >= 0.0 && py <= (double)(H - 1))) return false;
    const PwcBilinearF64 bl = pwc_bilinear_f64(px, py, H, W);
    const double wx0 = bl.wx0, wx1 = bl.wx1, wy0 = bl.wy0, wy1 = bl.wy1;
    const size_t img = (size_t)n * H * W;
    s.o00 = img + bl.o00; s.o01 = img + bl.o01;
    s.o10 = img + bl.o10; s.o11 = img + bl.o11;
    s.w00 = wy0 * wx0; s.w01 = wy0 * wx1; s.w10 = wy1 * wx0; s.w11 = wy1 * wx1;
    const float* p00 = other + s.o00 * other_cs;
    const float* p01 = other + s.o01 * other_cs;
    const float* p10 = other + s.o10 * other_cs;
    const float* p11 = other + s.o11 * other_cs;
    const double f[2] = {f0, f1};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const double v00 = (double)p00[c], v01 = (double)p01[c], v10 = (double)p10[c], v11 = (double)p11[c];
        const double top = wx0 * v00 + wx1 * v01, bot = wx0 * v10 + wx1 * v11;
        s.e[c] = (float)(f[c] + scale * (wy0 * top + wy1 * bot));
        s.sx[c] = (float)(wy0 * (v01 - v00) + wy1 * (v11 - v10));
        s.sy[c] = (float)(wx0 * (v10 - v00) + wx1 * (v11 - v01));
    }
    return true;
}

__global__ __launch_bounds__(256) void fb_consistency_partial_kernel(const FbcArgs a) {
    const int n = blockIdx.y;
    const bool fwd = blockIdx.z == 0;
    const float* own = fwd ? a.flow_a : a.flow_b;
    const float* other = fwd ? a.flow_b : a.flow_a;
    const int own_cs = fwd ? a.a_cs : a.b_cs, other_cs = fwd ? a.b_cs : a.a_cs;
    const uint8_t* in = fwd ? a.in_a : a.in_b;
    const int npix = a.H * a.W;
    const double scale = (double)a.flow_scale;
    float sum = 0.f;
    int cnt = 0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
        const int y = p / a.W, x = p - y * a.W;
        FbcSample s;
        if (fbc_pixel(own, own_cs, other, other_cs, in, n, y, x, (size_t)n * npix + p, a.H, a.W, scale, s)) {
            sum += unsup_rho(s.e[0], a.eps2, a.q) + unsup_rho(s.e[1], a.eps2, a.q);
            ++cnt;
        }
    }
    float* block = fwd ? a.block_a : a.block_b;
    pwc_loss_write_part<true>(sum, cnt, block, reinterpret_cast<int*>(block + (size_t)a.N * gridDim.x));
}

// 2^36 steps per unit, as in pwc_backward.hip: contributions below 1.5e-11 vanish, a cell holds |sum| < 2^25 before the finish
// refuses it, and a contribution that is not finite or reaches 2^26 raises the poison word (__double2ll_rn would turn a NaN
// into 0 and saturate an Inf: a diverging step must not come out finite).
#define FBC_FIX 68719476736.0

// One lane per pixel of a direction (blockIdx.y): the corner weight * rho'(e_k) of a contributing pixel into the OTHER flow's
// accumulators.  The first workgroup of a direction also looks at that direction's upstream gradients: they multiply what it
// scatters, and a non-finite one poisons the flow it scatters onto.
__global__ __launch_bounds__(256) void fb_consistency_scatter_kernel(const FbcArgs a) {
    const bool fwd = blockIdx.y == 0;
    const float* own = fwd ? a.flow_a : a.flow_b;
    const float* other = fwd ? a.flow_b : a.flow_a;
    const int own_cs = fwd ? a.a_cs : a.b_cs, other_cs = fwd ? a.b_cs : a.a_cs;
    const uint8_t* in = fwd ? a.in_a : a.in_b;
    const float* dsums = fwd ? a.dsums_a : a.dsums_b;
    unsigned long long* fix = reinterpret_cast<unsigned long long*>(fwd ? a.fix_b : a.fix_a);
    const long npix = (long)a.N * a.H * a.W;
    unsigned long long* poison = fix + 2 * npix;
    const double scale = (double)a.flow_scale;
    if (blockIdx.x == 0) {
        bool bad = false;
        for (int n = threadIdx.x; n < a.N; n += 256) bad |= !(fabsf(dsums[n]) < __builtin_inff());      // (false for a NaN)
        if (bad) atomicOr(poison, 1ull);
    }
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel px = pwc_loss_pixel(p, a.H, a.W);
        FbcSample s;
        if (!fbc_pixel(own, own_cs, other, other_cs, in, px.n, px.y, px.x, (size_t)p, a.H, a.W, scale, s)) continue;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float rg = unsup_rho_grad(s.e[k], a.eps2, a.q);
            if (!(fabsf(rg) < 67108864.f)) {                               // (false for a NaN); the weights are in [0, 1]
                atomicOr(poison, 1ull);
                continue;
            }
            const double g = (double)rg * FBC_FIX;
            atomicAdd(fix + 2 * s.o00 + k, (unsigned long long)__double2ll_rn(s.w00 * g));
            atomicAdd(fix + 2 * s.o01 + k, (unsigned long long)__double2ll_rn(s.w01 * g));
            atomicAdd(fix + 2 * s.o10 + k, (unsigned long long)__double2ll_rn(s.w10 * g));
            atomicAdd(fix + 2 * s.o11 + k, (unsigned long long)__double2ll_rn(s.w11 * g));
        }
    }
}

// One lane per pixel of a FLOW (blockIdx.y): the gather part from the pixel's own direction plus what the other direction
// scattered onto it.
__global__ __launch_bounds__(256) void fb_consistency_finish_kernel(const FbcArgs a) {
    const bool fwd = blockIdx.y == 0;
    const float* own = fwd ? a.flow_a : a.flow_b;
    const float* other = fwd ? a.flow_b : a.flow_a;
    const int own_cs = fwd ? a.a_cs : a.b_cs, other_cs = fwd ? a.b_cs : a.a_cs;
    const uint8_t* in = fwd ? a.in_a : a.in_b;
    const float* dsums_own = fwd ? a.dsums_a : a.dsums_b;
    const float* dsums_other = fwd ? a.dsums_b : a.dsums_a;
    const long long* fix = fwd ? a.fix_a : a.fix_b;
    float* dflow = fwd ? a.dflow_a : a.dflow_b;
    const int d_cs = fwd ? a.da_cs : a.db_cs;
    const long npix = (long)a.N * a.H * a.W;
    const bool poisoned = fix[2 * npix] != 0;
    const double scale = (double)a.flow_scale;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel px = pwc_loss_pixel(p, a.H, a.W);
        float* o = dflow + p * d_cs;
        if (poisoned) {                                                    // every element, whatever accumulate holds
            o[0] = __builtin_nanf("");
            o[1] = __builtin_nanf("");
            continue;
        }
        float gx = 0.f, gy = 0.f;
        FbcSample s;
        if (fbc_pixel(own, own_cs, other, other_cs, in, px.n, px.y, px.x, (size_t)p, a.H, a.W, scale, s)) {
            // d e_k / d flow[p, j] = flow_scale * (delta_kj + flow_scale * d sample_k / d pos_j)
            const float r0 = unsup_rho_grad(s.e[0], a.eps2, a.q), r1 = unsup_rho_grad(s.e[1], a.eps2, a.q);
            const float up = dsums_own[px.n] * a.flow_scale;
            gx = pwc_mul_rounded(up, r0 * (1.f + a.flow_scale * s.sx[0]) + r1 * (a.flow_scale * s.sx[1]));
            gy = pwc_mul_rounded(up, r0 * (a.flow_scale * s.sy[0]) + r1 * (1.f + a.flow_scale * s.sy[1]));
        }
        // a sum at or beyond 2^61 is where in-range contributions start to wrap the 64-bit sum: NaN instead of a finite wrong value
        const long long v0 = fix[2 * p], v1 = fix[2 * p + 1];
        const bool wild = v0 >= (1LL << 61) || v0 <= -(1LL << 61) || v1 >= (1LL << 61) || v1 <= -(1LL << 61);
        const float ups = dsums_other[px.n] * a.flow_scale;
        const float t0 = wild ? __builtin_nanf("") : pwc_mul_rounded(ups, (float)((double)v0 * (1.0 / FBC_FIX)));
        const float t1 = wild ? __builtin_nanf("") : pwc_mul_rounded(ups, (float)((double)v1 * (1.0 / FBC_FIX)));
        pwc_grad_store2(o, a.accumulate, 1.f, gx + t0, gy + t1);
    }
}

static int fbc_check(const float* flow_a, int a_cs, const float* flow_b, int b_cs, int N, int H, int W, float eps, float q) {
    if (!flow_a || !flow_b || N <= 0 || H <= 0 || W <= 0 || a_cs < 2 || b_cs < 2) return PWC_EINVAL;
    if (!(eps > 0.f) || !(q > 0.f && q <= 1.f)) return PWC_EINVAL;
    return PWC_OK;
}

// per direction a float sum and an int32 count per part
extern "C" size_t pwc_fb_consistency_workspace_floats(int N, int H, int W) { return 2 * pwc_loss_workspace_floats(N, H, W, 2); }

extern "C" int pwc_fb_consistency_sums_f32(const float* flow_a, int a_cs, const float* flow_b, int b_cs, float flow_scale,
                                           const uint8_t* valid_a, const uint8_t* valid_b, int N, int H, int W, float eps, float q,
                                           float* workspace, size_t workspace_floats, float* sums_a, int32_t* counts_a,
                                           float* sums_b, int32_t* counts_b, pwc_stream_t stream) {
    const int rc = fbc_check(flow_a, a_cs, flow_b, b_cs, N, H, W, eps, q);
    if (rc != PWC_OK) return rc;
    if (!sums_a || !counts_a || !sums_b || !counts_b) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (!workspace || workspace_floats < pwc_fb_consistency_workspace_floats(N, H, W)) return PWC_EINVAL;
    const int parts = (int)pwc_loss_parts(H, W);
    FbcArgs a = {};
    a.flow_a = flow_a; a.flow_b = flow_b; a.in_a = valid_a; a.in_b = valid_b;
    a.block_a = workspace; a.block_b = workspace + pwc_loss_workspace_floats(N, H, W, 2);
    a.a_cs = a_cs; a.b_cs = b_cs; a.N = N; a.H = H; a.W = W;
    a.flow_scale = flow_scale; a.eps2 = eps * eps; a.q = q;
    hipLaunchKernelGGL(fb_consistency_partial_kernel, dim3((unsigned)parts, (unsigned)N, 2u), dim3(256), 0, (hipStream_t)stream, a);
    pwc_loss_final_launch(a.block_a, parts, N, sums_a, counts_a, stream);
    pwc_loss_final_launch(a.block_b, parts, N, sums_b, counts_b, stream);
    return pwc_launch_status();
}

// per flow: an accumulator per pixel and channel, and the flow's poison word
static inline size_t fbc_fix_words(int N, int H, int W) { return (size_t)N * H * W * 2 + 1; }

extern "C" size_t pwc_fb_consistency_grad_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * fbc_fix_words(N, H, W) * sizeof(long long);
}

extern "C" int pwc_fb_consistency_grad_f32(const float* flow_a, int a_cs, const float* flow_b, int b_cs, float flow_scale,
                                           const uint8_t* valid_a, const uint8_t* valid_b, int N, int H, int W, float eps, float q,
                                           const float* dsums_a, const float* dsums_b, void* workspace, size_t workspace_bytes,
                                           float* dflow_a, int dflow_a_cs, float* dflow_b, int dflow_b_cs, int accumulate,
                                           pwc_stream_t stream) {
    const int rc = fbc_check(flow_a, a_cs, flow_b, b_cs, N, H, W, eps, q);
    if (rc != PWC_OK) return rc;
    if (!dsums_a || !dsums_b || !dflow_a || !dflow_b || dflow_a_cs < 2 || dflow_b_cs < 2) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u) ||
        workspace_bytes < pwc_fb_consistency_grad_workspace_bytes(N, H, W))
        return PWC_EINVAL;
    FbcArgs a = {};
    a.flow_a = flow_a; a.flow_b = flow_b; a.in_a = valid_a; a.in_b = valid_b; a.dsums_a = dsums_a; a.dsums_b = dsums_b;
    a.dflow_a = dflow_a; a.dflow_b = dflow_b;
    a.fix_a = reinterpret_cast<long long*>(workspace); a.fix_b = a.fix_a + fbc_fix_words(N, H, W);
    a.a_cs = a_cs; a.b_cs = b_cs; a.da_cs = dflow_a_cs; a.db_cs = dflow_b_cs; a.N = N; a.H = H; a.W = W;
    a.flow_scale = flow_scale; a.eps2 = eps * eps; a.q = q; a.accumulate = accumulate;
    const hipError_t me = hipMemsetAsync(workspace, 0, 2 * fbc_fix_words(N, H, W) * sizeof(long long), (hipStream_t)stream);
    if (me != hipSuccess) { (void)hipGetLastError(); return (int)me; }          // the memset's OWN error, never PWC_OK
    const dim3 grid(pwc_loss_grad_blocks(N, H, W).x, 2u);
    hipLaunchKernelGGL(fb_consistency_scatter_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(fb_consistency_finish_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    return pwc_launch_status();
}
