// pwc_fit.hip -- frames of any size around the network: pwc_fit_frames_f32 brings N x H x W x 3 frames (uint8 or float32) to
// the network's geometry (the next multiples of 64), pwc_refit_flow_f32 brings the flow back to the frames' grid.  Two modes
// (include/pwc_hip.h): half-pixel bilinear resize, or replicate padding / cropping.
//
// Both kernels are elementwise gathers on dense tensors: no LDS, no atomics, no status word.  Every value is formed in double
// from exact integer coordinates and rounded to float32 once (the pad / crop launches run at 0.5 - 0.7 of
// their bytes at 8 TB/s, the resize launches at 0.27 - 0.34 -- their double arithmetic shows).  A lane owns consecutive pixels of the FLAT output (four of the fit: 48 bytes, three 16-byte stores; two of the
// refit: one 16-byte store), which keeps the stores aligned whatever the row length; a group may run over the end of a row, so
// every pixel carries its own (row, column).  The uint8 source is read by byte loads: its rows (3 W bytes) and its base have no
// alignment, and an aligned word around a pixel may lie outside the tensor.
#include "pwc_common.h"

namespace {

// One axis of the half-pixel resize: output index d of `out` samples takes
//   src = ((2 d + 1) in - out) / (2 out), clamped to [0, in - 1]
// (one double division of exact integers), i0 = floor(src), f = src - i0, i1 = min(i0 + 1, in - 1).  in == out: src = d, f = 0.
struct FitTap {
    int i0, i1;
    double f;
};
__device__ __forceinline__ FitTap fit_tap(int d, int in, int out) {
    const long long num = (2ll * d + 1) * in - out;
    double src = (double)num / (double)(2ll * out);
    src = fmin(fmax(src, 0.0), (double)(in - 1));
    const double fl = floor(src);
    FitTap t;
    t.i0 = (int)fl;
    t.f = src - fl;
    t.i1 = min(t.i0 + 1, in - 1);
    return t;
}
__device__ __forceinline__ FitTap fit_tap_pad(int d, int in) {
    const int i = min(d, in - 1);
    return FitTap{i, i, 0.0};
}

// Every operation rounded on its own (no contraction into fused multiply-adds): the float64 reference of the tests performs
// exactly these operations, and a weight of exactly 0 or 1 leaves a copy.
__device__ __forceinline__ double fit_blend(double a, double b, double c, double d, double fx, double fy) {
#pragma clang fp contract(off)
    return (1.0 - fy) * ((1.0 - fx) * a + fx * b) + fy * ((1.0 - fx) * c + fx * d);
}

template <typename T>
__device__ __forceinline__ double fit_value(const T* p);
template <>
__device__ __forceinline__ double fit_value<float>(const float* p) { return (double)*p; }
// The float32 the CLIs form on the host today, float(double(v) / 255.0).  v * (1.0 / 255.0) rounds to the same float32 for all
// 256 values (tests/test_host_fit.py walks them) and spares twelve double divisions per resized pixel.
template <>
__device__ __forceinline__ double fit_value<uint8_t>(const uint8_t* p) { return (double)(float)((double)*p * (1.0 / 255.0)); }

// the three channels of output pixel (oy, ox) of image n
template <typename T, bool PAD>
__device__ __forceinline__ void fit_pixel(const T* __restrict__ x, int n, const FitTap& ty, int ox, int H, int W, int OW, float* out) {
    const FitTap tx = PAD ? fit_tap_pad(ox, W) : fit_tap(ox, W, OW);
    const T* r0 = x + ((size_t)n * H + ty.i0) * W * 3;
    if (PAD) {
        const T* p = r0 + (size_t)tx.i0 * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = (float)fit_value<T>(p + c);
        return;
    }
    const T* r1 = x + ((size_t)n * H + ty.i1) * W * 3;
    const size_t o0 = (size_t)tx.i0 * 3, o1 = (size_t)tx.i1 * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out[c] = (float)fit_blend(fit_value<T>(r0 + o0 + c), fit_value<T>(r0 + o1 + c), fit_value<T>(r1 + o0 + c),
                                  fit_value<T>(r1 + o1 + c), tx.f, ty.f);
}

// y: N x OH x OW x 3 dense, 16-byte aligned.  total = N * OH * OW output pixels (< 2^31); a lane takes pixels 4 q .. 4 q + 3.
template <typename T, bool PAD>
__global__ __launch_bounds__(256) void fit_frames_kernel(const T* __restrict__ x, float* __restrict__ y, int H, int W, int OH, int OW,
                                                         unsigned total) {
    const unsigned quads = (total + 3u) >> 2;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < quads; q += gridDim.x * 256u) {
        const unsigned p0 = q << 2;
        unsigned row = p0 / (unsigned)OW;                      // n * OH + oy
        int ox = (int)(p0 - row * (unsigned)OW);
        int n = (int)(row / (unsigned)OH), oy = (int)(row - (unsigned)n * (unsigned)OH);
        FitTap ty = PAD ? fit_tap_pad(oy, H) : fit_tap(oy, H, OH);
        float v[12];
        const int cnt = (int)min(4u, total - p0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < cnt) {
                fit_pixel<T, PAD>(x, n, ty, ox, H, W, OW, v + 3 * k);
                if (++ox == OW) {                               // the group runs on into the next row (or image)
                    ox = 0;
                    if (++oy == OH) { oy = 0; ++n; }
                    ty = PAD ? fit_tap_pad(oy, H) : fit_tap(oy, H, OH);
                }
            } else {
                v[3 * k] = v[3 * k + 1] = v[3 * k + 2] = 0.f;
            }
        }
        float* dst = y + (size_t)p0 * 3;
        if (cnt == 4) {
            f32x4* d4 = reinterpret_cast<f32x4*>(dst);
            d4[0] = f32x4{v[0], v[1], v[2], v[3]};
            d4[1] = f32x4{v[4], v[5], v[6], v[7]};
            d4[2] = f32x4{v[8], v[9], v[10], v[11]};
        } else {
#pragma unroll
            for (int e = 0; e < 9; ++e)                         // the tail of the tensor: one to three pixels
                if (e < 3 * cnt) dst[e] = v[e];
        }
    }
}

// both channels of output pixel p (flat index over N x H x W) of the refit
template <bool PAD>
__device__ __forceinline__ f32x2 refit_pixel(const float* __restrict__ f, unsigned p, int FH, int FW, int H, int W, double su, double sv) {
    const unsigned row = p / (unsigned)W;
    const int ox = (int)(p - row * (unsigned)W);
    const int n = (int)(row / (unsigned)H), oy = (int)(row - (unsigned)n * (unsigned)H);
    const f32x2* img = reinterpret_cast<const f32x2*>(f) + (size_t)n * FH * FW;
    if (PAD) return img[(size_t)oy * FW + ox];
    const FitTap ty = fit_tap(oy, FH, H), tx = fit_tap(ox, FW, W);
    const f32x2 a = img[(size_t)ty.i0 * FW + tx.i0], b = img[(size_t)ty.i0 * FW + tx.i1];
    const f32x2 c = img[(size_t)ty.i1 * FW + tx.i0], d = img[(size_t)ty.i1 * FW + tx.i1];
    return f32x2{(float)(fit_blend(a[0], b[0], c[0], d[0], tx.f, ty.f) * su), (float)(fit_blend(a[1], b[1], c[1], d[1], tx.f, ty.f) * sv)};
}

// f: N x FH x FW x 2, y: N x H x W x 2, both dense and 8-byte aligned.  A lane takes pixels 2 q, 2 q + 1 of the flat output;
// Y16: y is 16-byte aligned and the pair goes out as one store.
template <bool PAD, bool Y16>
__global__ __launch_bounds__(256) void refit_flow_kernel(const float* __restrict__ f, float* __restrict__ y, int FH, int FW, int H, int W,
                                                         unsigned total, double su, double sv) {
    const unsigned pairs = (total + 1u) >> 1;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < pairs; q += gridDim.x * 256u) {
        const unsigned p0 = q << 1;
        const f32x2 v0 = refit_pixel<PAD>(f, p0, FH, FW, H, W, su, sv);
        if (p0 + 1 < total) {
            const f32x2 v1 = refit_pixel<PAD>(f, p0 + 1, FH, FW, H, W, su, sv);
            if (Y16) {
                *reinterpret_cast<f32x4*>(y + (size_t)p0 * 2) = f32x4{v0[0], v0[1], v1[0], v1[1]};
            } else {
                reinterpret_cast<f32x2*>(y)[p0] = v0;
                reinterpret_cast<f32x2*>(y)[p0 + 1] = v1;
            }
        } else {
            reinterpret_cast<f32x2*>(y)[p0] = v0;
        }
    }
}

// grid of a memory-bound launch: one lane per work item, capped at 2048 workgroups with a grid stride
inline unsigned fit_grid(unsigned items) { return items > 2048u * 256u ? 2048u : (items + 255u) / 256u; }

}  // namespace

extern "C" int pwc_fit_frames_f32(const void* x, int x_is_u8, float* y, int N, int H, int W, int OH, int OW, int mode,
                                  pwc_stream_t stream) {
    if (!x || !y) return PWC_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || OH < H || OW < W) return PWC_EINVAL;
    if (mode != PWC_FIT_RESIZE && mode != PWC_FIT_PAD) return PWC_EINVAL;
    if (!pwc_aligned16(y) || (!x_is_u8 && (reinterpret_cast<uintptr_t>(x) & 3u))) return PWC_EALIGN;
    if ((long long)N * OH * OW >= (1ll << 31)) return PWC_ERANGE;
    const unsigned total = (unsigned)N * (unsigned)OH * (unsigned)OW;
    const dim3 grid(fit_grid((total + 3u) >> 2)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (x_is_u8) {
        const uint8_t* xb = static_cast<const uint8_t*>(x);
        if (mode == PWC_FIT_PAD) hipLaunchKernelGGL((fit_frames_kernel<uint8_t, true>), grid, block, 0, s, xb, y, H, W, OH, OW, total);
        else hipLaunchKernelGGL((fit_frames_kernel<uint8_t, false>), grid, block, 0, s, xb, y, H, W, OH, OW, total);
    } else {
        const float* xf = static_cast<const float*>(x);
        if (mode == PWC_FIT_PAD) hipLaunchKernelGGL((fit_frames_kernel<float, true>), grid, block, 0, s, xf, y, H, W, OH, OW, total);
        else hipLaunchKernelGGL((fit_frames_kernel<float, false>), grid, block, 0, s, xf, y, H, W, OH, OW, total);
    }
    return pwc_launch_status();
}

extern "C" int pwc_refit_flow_f32(const float* f, float* y, int N, int FH, int FW, int H, int W, int mode, pwc_stream_t stream) {
    if (!f || !y) return PWC_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || FH <= 0 || FW <= 0) return PWC_EINVAL;
    if (mode != PWC_FIT_RESIZE && mode != PWC_FIT_PAD) return PWC_EINVAL;
    if (mode == PWC_FIT_PAD && (FH < H || FW < W)) return PWC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(f) & 7u) || (reinterpret_cast<uintptr_t>(y) & 7u)) return PWC_EALIGN;
    if ((long long)N * H * W >= (1ll << 31) || (long long)N * FH * FW >= (1ll << 31)) return PWC_ERANGE;
    const unsigned total = (unsigned)N * (unsigned)H * (unsigned)W;
    const dim3 grid(fit_grid((total + 1u) >> 1)), block(256);
    hipStream_t s = (hipStream_t)stream;
    const double su = (double)W / (double)FW, sv = (double)H / (double)FH;
    const bool y16 = pwc_aligned16(y);
    if (mode == PWC_FIT_PAD) {
        if (y16) hipLaunchKernelGGL((refit_flow_kernel<true, true>), grid, block, 0, s, f, y, FH, FW, H, W, total, su, sv);
        else hipLaunchKernelGGL((refit_flow_kernel<true, false>), grid, block, 0, s, f, y, FH, FW, H, W, total, su, sv);
    } else {
        if (y16) hipLaunchKernelGGL((refit_flow_kernel<false, true>), grid, block, 0, s, f, y, FH, FW, H, W, total, su, sv);
        else hipLaunchKernelGGL((refit_flow_kernel<false, false>), grid, block, 0, s, f, y, FH, FW, H, W, total, su, sv);
    }
    return pwc_launch_status();
}
