// pwc_augment.hip -- training augmentation in one launch (pwc_augment_pairs_f32, include/pwc_hip.h): an OH x OW window of both
// frames of every pair resampled through one affine map per frame, colour jitter, and the ground-truth flow carried into the
// augmented pair's geometry, out_flow(p) = I1 (q0 + flow(q0)) - p with q0 = M0 p.
//
// An elementwise gather on dense tensors like pwc_fit.hip: no LDS, no atomics, no random numbers (the host draws the 32-double
// record of every sample).  One lane per output pixel, 16 x 16 pixel workgroups -- a wave is a 16 x 4 patch, so under any
// rotation its lanes gather a compact patch of source texels -- and blockIdx.z is the sample: the record is wave-uniform.
// Every value is formed in double, every operation rounded on its own (no contraction into fused multiply-adds: the float64
// reference of the tests performs exactly these operations, and a weight of exactly 0 or 1 leaves a copy), and rounded to
// float32 once.  The uint8 source is read by byte loads, as in pwc_fit.hip.
#include "pwc_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AUG_RECORD = 32;                 // doubles per sample
constexpr int AUG_TILE = 16;

template <typename T>
__device__ __forceinline__ double aug_value(const T* p);
template <>
__device__ __forceinline__ double aug_value<float>(const float* p) { return (double)*p; }
// float(double(v) / 255.0), spelled as in pwc_fit.hip (the same float32 for all 256 values)
template <>
__device__ __forceinline__ double aug_value<uint8_t>(const uint8_t* p) { return (double)(float)((double)*p * (1.0 / 255.0)); }

__device__ __forceinline__ double aug_blend(double a, double b, double c, double d, double fx, double fy) {
    return (1.0 - fy) * ((1.0 - fx) * a + fx * b) + fy * ((1.0 - fx) * c + fx * d);
}

// (a b c; d e f) applied to (x, y)
__device__ __forceinline__ void aug_map(const double* __restrict__ m, double x, double y, double& qx, double& qy) {
    qx = (m[0] * x + m[1] * y) + m[2];
    qy = (m[3] * x + m[4] * y) + m[5];
}

__device__ __forceinline__ bool aug_photo_identity(const double* __restrict__ ph) {
    return ph[0] == 1.0 && ph[1] == 1.0 && ph[2] == 1.0 && ph[3] == 1.0 && ph[4] == 1.0 && ph[5] == 0.0;
}

__device__ __forceinline__ double aug_photo(double v, double gain, double gamma, double contrast, double brightness) {
    v = fmin(fmax(v * gain, 0.0), 1.0);
    if (gamma != 1.0) v = pow(v, gamma);
    v = ((v - 0.5) * contrast + 0.5) + brightness;
    return fmin(fmax(v, 0.0), 1.0);
}

// the three channels of one frame at position (qx, qy), clamped into the frame
template <typename T>
__device__ __forceinline__ void aug_frame(const T* __restrict__ im, const double* __restrict__ ph, double qx, double qy, int H, int W,
                                          float* __restrict__ dst) {
    qx = fmin(fmax(qx, 0.0), (double)(W - 1));                       // (a NaN becomes 0: every index stays inside)
    qy = fmin(fmax(qy, 0.0), (double)(H - 1));
    const double flx = floor(qx), fly = floor(qy);
    const double fx = qx - flx, fy = qy - fly;
    const int x0 = (int)flx, y0 = (int)fly;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const T* r0 = im + (size_t)y0 * W * 3;
    const T* r1 = im + (size_t)y1 * W * 3;
    const size_t o0 = (size_t)x0 * 3, o1 = (size_t)x1 * 3;
    double v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        v[c] = aug_blend(aug_value<T>(r0 + o0 + c), aug_value<T>(r0 + o1 + c), aug_value<T>(r1 + o0 + c), aug_value<T>(r1 + o1 + c), fx, fy);
    if (!aug_photo_identity(ph)) {                                   // wave-uniform
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = aug_photo(v[c], ph[c], ph[3], ph[4], ph[5]);
    }
    dst[0] = (float)v[0];
    dst[1] = (float)v[1];
    dst[2] = (float)v[2];
}

// im0, im1: N x H x W x 3; flow: N x H x W x 2 or null; valid: N x H x W or null; params: N x 32; outputs N x OH x OW x {3, 3, 2, 1}.
// grid (ceil(OW / 16), ceil(OH / 16), N), block (16, 16).
template <typename T>
__global__ __launch_bounds__(AUG_TILE * AUG_TILE) void augment_pairs_kernel(
    const T* __restrict__ im0, const T* __restrict__ im1, const float* __restrict__ flow, const uint8_t* __restrict__ valid,
    const double* __restrict__ params, float* __restrict__ out0, float* __restrict__ out1, float* __restrict__ out_flow,
    uint8_t* __restrict__ out_valid, int H, int W, int OH, int OW, int flow_nearest) {
    const int ox = blockIdx.x * AUG_TILE + threadIdx.x, oy = blockIdx.y * AUG_TILE + threadIdx.y;
    if (ox >= OW || oy >= OH) return;
    const int n = blockIdx.z;
    const double* __restrict__ rec = params + (size_t)n * AUG_RECORD;
    const size_t in_px = (size_t)n * H * W;                          // first pixel of sample n in the inputs
    const size_t op = ((size_t)n * OH + oy) * OW + ox;               // this output pixel
    const double x = (double)ox, y = (double)oy;

    double q0x, q0y, q1x, q1y;
    aug_map(rec, x, y, q0x, q0y);
    aug_map(rec + 6, x, y, q1x, q1y);
    aug_frame<T>(im0 + in_px * 3, rec + 18, q0x, q0y, H, W, out0 + op * 3);
    aug_frame<T>(im1 + in_px * 3, rec + 24, q1x, q1y, H, W, out1 + op * 3);
    if (!flow) return;

    // the flow at the un-clamped q0; a NaN coordinate fails the comparisons and is outside
    const f32x2* fl = reinterpret_cast<const f32x2*>(flow) + in_px;
    const uint8_t* va = valid ? valid + in_px : nullptr;
    bool ok = q0x >= 0.0 && q0x <= (double)(W - 1) && q0y >= 0.0 && q0y <= (double)(H - 1);
    double u = 0.0, v = 0.0;
    if (ok) {
        if (flow_nearest) {
            const int tx = min((int)floor(q0x + 0.5), W - 1), ty = min((int)floor(q0y + 0.5), H - 1);
            const size_t t = (size_t)ty * W + tx;
            ok = !va || va[t] != 0;
            if (ok) {
                const f32x2 a = fl[t];
                u = (double)a[0];
                v = (double)a[1];
            }
        } else {
            const double flx = floor(q0x), fly = floor(q0y);
            const double fx = q0x - flx, fy = q0y - fly;
            const int x0 = (int)flx, y0 = (int)fly;
            // a corner of weight zero is not a tap: not read, and its label does not count (fx > 0 implies x0 + 1 <= W - 1)
            const int x1 = fx > 0.0 ? x0 + 1 : x0, y1 = fy > 0.0 ? y0 + 1 : y0;
            const size_t ta = (size_t)y0 * W + x0, tb = (size_t)y0 * W + x1, tc = (size_t)y1 * W + x0, td = (size_t)y1 * W + x1;
            ok = !va || (va[ta] != 0 && va[tb] != 0 && va[tc] != 0 && va[td] != 0);
            if (ok) {
                const f32x2 a = fl[ta], b = fl[tb], c = fl[tc], d = fl[td];
                u = aug_blend((double)a[0], (double)b[0], (double)c[0], (double)d[0], fx, fy);
                v = aug_blend((double)a[1], (double)b[1], (double)c[1], (double)d[1], fx, fy);
            }
        }
    }
    f32x2 o = {0.f, 0.f};
    if (ok) {
        double p1x, p1y;
        aug_map(rec + 12, q0x + u, q0y + v, p1x, p1y);
        o = f32x2{(float)(p1x - x), (float)(p1y - y)};
    }
    reinterpret_cast<f32x2*>(out_flow)[op] = o;
    out_valid[op] = ok ? 1 : 0;
}

}  // namespace

extern "C" int pwc_augment_pairs_f32(const void* im0, const void* im1, int im_is_u8, const float* flow, const unsigned char* valid,
                                     const double* params, float* out0, float* out1, float* out_flow, unsigned char* out_valid,
                                     int N, int H, int W, int OH, int OW, int flow_nearest, pwc_stream_t stream) {
    if (!im0 || !im1 || !params || !out0 || !out1) return PWC_EINVAL;
    if (flow && (!out_flow || !out_valid)) return PWC_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return PWC_EINVAL;
    if (!im_is_u8 && (pwc_off(im0, 3u) || pwc_off(im1, 3u))) return PWC_EALIGN;
    if (pwc_off(out0, 3u) || pwc_off(out1, 3u) || pwc_off(params, 7u)) return PWC_EALIGN;
    if (flow && (pwc_off(flow, 7u) || pwc_off(out_flow, 7u))) return PWC_EALIGN;
    if ((long long)N * H * W >= (1ll << 31) || (long long)N * OH * OW >= (1ll << 31) || N > 65535 ||
        (OH + AUG_TILE - 1) / AUG_TILE > 65535)
        return PWC_ERANGE;
    const dim3 grid((OW + AUG_TILE - 1) / AUG_TILE, (OH + AUG_TILE - 1) / AUG_TILE, N), block(AUG_TILE, AUG_TILE);
    hipStream_t s = (hipStream_t)stream;
    if (im_is_u8)
        hipLaunchKernelGGL((augment_pairs_kernel<uint8_t>), grid, block, 0, s, static_cast<const uint8_t*>(im0),
                           static_cast<const uint8_t*>(im1), flow, valid, params, out0, out1, out_flow, out_valid, H, W, OH, OW,
                           flow_nearest);
    else
        hipLaunchKernelGGL((augment_pairs_kernel<float>), grid, block, 0, s, static_cast<const float*>(im0),
                           static_cast<const float*>(im1), flow, valid, params, out0, out1, out_flow, out_valid, H, W, OH, OW,
                           flow_nearest);
    return pwc_launch_status();
}
