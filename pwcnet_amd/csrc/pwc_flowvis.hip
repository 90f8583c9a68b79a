// pwc_flowvis.hip -- flow visualisation: Middlebury colour coding, frame tiles, KITTI's log-scale error map, written as RGB bytes
// into a batch of output images from a table of tiles (gfx950; C ABI in include/pwc_hip.h, "flow visualisation"; semantics,
// bounds and bytes in DESIGN.md 16).
//
//   pwc_flow_max_radius_f64     out[n] = max sqrt(u u + v v) over the known (and, with a mask, valid) pixels of image n, a double
//   pwc_flow_vis_tiles_u8       out (N, out_h, out_w, 3) bytes: every pixel from the tile whose rectangle [x0, x0 + tile_w) holds it
//   pwc_flow_vis_wheel_u8       the 55 x 3 colour wheel the kernel reads (the host test compares it with flow_io.color_wheel())
//
// Every value is formed in double from the float32 inputs, as the SAME sequence of IEEE operations flow_io.flow_to_color
// performs in numpy: no fused multiply-add is formed anywhere in this file (the pragma below), division and square root are
// the correctly rounded ones, so atan2 is the only operation whose result may differ from numpy's.  A flow's optional scale is
// ONE float32 product per component, applied first (what `f * (20.0 / 2 ** (num_levels - l))` does to a float32 array); the
// "known" rule (both components finite with |.| <= 1e9, flow_io.flow_valid) sees the product.
// The maximum: non-negative doubles order as their bit patterns do, and a maximum does not depend on order -- a workgroup takes
// the maximum of its lanes in LDS and issues one 64-bit integer atomic max into a result the entry point zeroes itself.  Two calls
// give the same bits and an image gives the same bits alone and in a batch; no workspace, no second launch.
// The pictures: 3-byte pixels.  A lane takes FOUR consecutive pixels of the flat (N, out_h, out_w) index, 4 k .. 4 k + 3: twelve
// bytes at a byte offset that is a multiple of 12, so wherever the output pointer is on a 4-byte boundary they are three whole
// dwords (a wave writes 768 consecutive bytes), whatever the tile offsets and row lengths are -- a run may cross a tile or a row,
// every pixel finds its own tile (at most 8 rectangles and two 64-bit divisions per pixel).  The last run of an output whose pixel count is no multiple of 4, and every run of an output
// off a 4-byte boundary, is written byte by byte.
#include <float.h>

#include "flow_record.h"
#include "loss_common.h"

#pragma clang fp contract(off)

#define VIS_WHEEL_N 55
#define VIS_WHEEL_INIT                                                                                                       \
    {{255, 0, 0}, {255, 17, 0}, {255, 34, 0}, {255, 51, 0}, {255, 68, 0}, {255, 85, 0}, {255, 102, 0}, {255, 119, 0},        \
     {255, 136, 0}, {255, 153, 0}, {255, 170, 0}, {255, 187, 0}, {255, 204, 0}, {255, 221, 0}, {255, 238, 0}, {255, 255, 0}, \
     {213, 255, 0}, {170, 255, 0}, {128, 255, 0}, {85, 255, 0}, {43, 255, 0}, {0, 255, 0}, {0, 255, 63}, {0, 255, 127},      \
     {0, 255, 191}, {0, 255, 255}, {0, 232, 255}, {0, 209, 255}, {0, 186, 255}, {0, 163, 255}, {0, 140, 255}, {0, 116, 255}, \
     {0, 93, 255}, {0, 70, 255}, {0, 47, 255}, {0, 24, 255}, {0, 0, 255}, {19, 0, 255}, {39, 0, 255}, {58, 0, 255},          \
     {78, 0, 255}, {98, 0, 255}, {117, 0, 255}, {137, 0, 255}, {156, 0, 255}, {176, 0, 255}, {196, 0, 255}, {215, 0, 255},   \
     {235, 0, 255}, {255, 0, 255}, {255, 0, 213}, {255, 0, 170}, {255, 0, 128}, {255, 0, 85}, {255, 0, 43}}

// flow_io.color_wheel(): RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 hues.
static const uint8_t vis_wheel_host[VIS_WHEEL_N][3] = VIS_WHEEL_INIT;
__constant__ uint8_t vis_wheel[VIS_WHEEL_N][3] = VIS_WHEEL_INIT;

// KITTI's log colour scale: the bin of n_err is the first whose upper edge exceeds it, the last one beyond 16.
__constant__ float vis_err_edge[9] = {0.0625f, 0.125f, 0.25f, 0.5f, 1.f, 2.f, 4.f, 8.f, 16.f};
__constant__ uint8_t vis_err_rgb[10][3] = {{49, 54, 149},   {69, 117, 180}, {116, 173, 209}, {171, 217, 233}, {224, 243, 248},
                                           {254, 224, 144}, {253, 174, 97}, {244, 109, 67},  {215, 48, 39},   {165, 0, 38}};

struct VisArgs {
    pwc_vis_tile t[PWC_VIS_MAX_TILES];
    uint8_t* out;
    long npix;                // N * out_h * out_w
    int ntiles, out_h, out_w;
    int dwords;               // out is on a 4-byte boundary
};

__device__ __forceinline__ unsigned vis_pack(unsigned r, unsigned g, unsigned b) { return r | (g << 8) | (b << 16); }

// The flow of a record times the scale: one float32 product per component (1.0f changes nothing).
__device__ __forceinline__ void vis_load_flow(const float* p, float scale, float& u, float& v) {
    u = pwc_mul_rounded(p[0], scale);
    v = pwc_mul_rounded(p[1], scale);
}

// flow_io.flow_to_color for one pixel whose unknown / masked flow has been replaced by (0, 0).
__device__ __forceinline__ unsigned vis_flow_color(double u, double v, double max_rad) {
    double rad = sqrt(u * u + v * v);
    const double scale = max_rad + DBL_EPSILON;
    u = u / scale; v = v / scale; rad = rad / scale;
    const double fk = (atan2(-v, -u) / 3.141592653589793 + 1.0) / 2.0 * (double)(VIS_WHEEL_N - 1);
    const double k0d = floor(fk);
    int k0 = k0d >= 0.0 ? (k0d <= (double)(VIS_WHEEL_N - 1) ? (int)k0d : VIS_WHEEL_N - 1) : 0;      // (a NaN max_rad: entry 0)
    const int k1 = (k0 + 1) % VIS_WHEEL_N;
    const double f = fk - k0d;
    unsigned c[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double col = (1.0 - f) * (double)vis_wheel[k0][j] / 255.0 + f * (double)vis_wheel[k1][j] / 255.0;
        col = rad <= 1.0 ? 1.0 - rad * (1.0 - col) : col * 0.75;
        c[j] = pwc_clamp_byte(floor(255.0 * col));
    }
    return vis_pack(c[0], c[1], c[2]);
}

// The error map's pixel: gt known (and valid), (pu, pv) the prediction.
__device__ __forceinline__ unsigned vis_error_color(float pu, float pv, float gu, float gv) {
    int bin = 9;
    if (pwc_flow_known(pu, pv)) {
        const double du = (double)pu - (double)gu, dv = (double)pv - (double)gv;
        const double d_err = sqrt(du * du + dv * dv);
        const double d_mag = sqrt((double)gu * (double)gu + (double)gv * (double)gv);
        double n_err = d_err / 3.0;
        if (d_mag != 0.0) {
            const double rel = (d_err / d_mag) / 0.05;
            n_err = rel < n_err ? rel : n_err;
        }
        bin = 0;
        while (bin < 9 && !(n_err < (double)vis_err_edge[bin])) ++bin;
    }
    return vis_pack(vis_err_rgb[bin][0], vis_err_rgb[bin][1], vis_err_rgb[bin][2]);
}

// Output pixel g of the flat (N, out_h, out_w) index: its three bytes, R in the low one.  A pixel no tile covers is black.
__device__ __forceinline__ unsigned vis_pixel(const VisArgs& a, long g) {
    const int x = (int)(g % a.out_w);
    const long r = g / a.out_w;
    const int y = (int)(r % a.out_h), n = (int)(r / a.out_h);
    int k = 0;
    while (k < a.ntiles && !(x >= a.t[k].x0 && x < a.t[k].x0 + a.t[k].tile_w)) ++k;
    if (k == a.ntiles) return 0u;
    const pwc_vis_tile& t = a.t[k];
    // pyramid_montage's integers: sy = y * src_h // out_h, sx = x * src_w // tile_w (both below src_h, src_w)
    const int sy = (int)((long)y * t.src_h / a.out_h);
    const int sx = (int)((long)(x - t.x0) * t.src_w / t.tile_w);
    const size_t pix = ((size_t)n * t.src_h + sy) * t.src_w + sx;
    if (t.kind == PWC_VIS_FRAME_U8) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(t.src) + pix * 3;
        return vis_pack(p[0], p[1], p[2]);
    }
    if (t.kind == PWC_VIS_FRAME_F32) {
        const float* p = reinterpret_cast<const float*>(t.src) + pix * 3;
        return vis_pack(pwc_clamp_byte(rint(255.0 * (double)p[0])), pwc_clamp_byte(rint(255.0 * (double)p[1])),
                        pwc_clamp_byte(rint(255.0 * (double)p[2])));
    }
    if (t.kind == PWC_VIS_ERROR) {
        if (t.valid && !t.valid[pix]) return 0u;
        const float* gp = t.gt + pix * t.gt_cs;
        const float gu = gp[0], gv = gp[1];
        if (!pwc_flow_known(gu, gv)) return 0u;
        const float* pp = reinterpret_cast<const float*>(t.src) + pix * t.src_cs;
        return vis_error_color(pp[0], pp[1], gu, gv);
    }
    double u = 0.0, v = 0.0;                                               // PWC_VIS_FLOW
    if (!(t.valid && !t.valid[pix])) {
        float uf, vf;
        vis_load_flow(reinterpret_cast<const float*>(t.src) + pix * t.src_cs, t.flow_scale, uf, vf);
        if (pwc_flow_known(uf, vf)) { u = (double)uf; v = (double)vf; }
    }
    return vis_flow_color(u, v, t.max_rad[n]);
}

// One lane per run of four output pixels.
__global__ __launch_bounds__(256) void flow_vis_tiles_kernel(const VisArgs a) {
    const long runs = (a.npix + 3) / 4;
    for (long k = blockIdx.x * 256L + threadIdx.x; k < runs; k += (long)gridDim.x * 256) {
        const long g0 = 4 * k;
        uint8_t* o = a.out + 3 * g0;
        if (a.dwords && g0 + 4 <= a.npix) {
            const unsigned p0 = vis_pixel(a, g0), p1 = vis_pixel(a, g0 + 1), p2 = vis_pixel(a, g0 + 2), p3 = vis_pixel(a, g0 + 3);
            unsigned* d = reinterpret_cast<unsigned*>(o);
            d[0] = p0 | (p1 << 24);
            d[1] = (p1 >> 8) | (p2 << 16);
            d[2] = (p2 >> 16) | (p3 << 8);
        } else {
            for (long g = g0; g < a.npix && g < g0 + 4; ++g) {
                const unsigned p = vis_pixel(a, g);
                uint8_t* b = a.out + 3 * g;
                b[0] = (uint8_t)(p & 255u); b[1] = (uint8_t)((p >> 8) & 255u); b[2] = (uint8_t)(p >> 16);
            }
        }
    }
}

// grid (parts, N): the largest radius over the known, valid pixels of image n, as the bits of a non-negative double.
__global__ __launch_bounds__(256) void flow_max_radius_kernel(const float* __restrict__ flow, int cs, const uint8_t* __restrict__ valid,
                                                              int H, int W, float scale, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long red[256];
    const int n = blockIdx.y;
    const long npix = (long)H * W;
    unsigned long long m = 0ull;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += gridDim.x * 256L) {      // (long: H * W may be close to 2^31)
        const size_t pix = (size_t)n * npix + p;
        if (valid && !valid[pix]) continue;
        float uf, vf;
        vis_load_flow(flow + pix * cs, scale, uf, vf);
        if (!pwc_flow_known(uf, vf)) continue;
        const double u = (double)uf, v = (double)vf;
        const unsigned long long b = (unsigned long long)__double_as_longlong(sqrt(u * u + v * v));
        m = b > m ? b : m;
    }
    const int t = threadIdx.x;
    red[t] = m;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) red[t] = red[t] > red[t + k] ? red[t] : red[t + k];
        __syncthreads();
    }
    if (t == 0 && red[0]) atomicMax(out + n, red[0]);
}

// ---------------------------------------------------------------- host
extern "C" int pwc_flow_vis_wheel_u8(uint8_t* wheel) {
    if (!wheel) return PWC_EINVAL;
    for (int k = 0; k < VIS_WHEEL_N; ++k)
        for (int j = 0; j < 3; ++j) wheel[3 * k + j] = vis_wheel_host[k][j];
    return PWC_OK;
}

extern "C" int pwc_flow_max_radius_f64(const float* flow, int flow_cs, const uint8_t* valid, int N, int H, int W, float flow_scale,
                                       double* max_rad, pwc_stream_t stream) {
    if (!flow || !max_rad || N < 1 || H < 1 || W < 1 || flow_cs < 2) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (pwc_off(flow, 3u) || pwc_off(max_rad, 7u)) return PWC_EALIGN;
    const hipStream_t s = (hipStream_t)stream;
    const hipError_t me = hipMemsetAsync(max_rad, 0, (size_t)N * sizeof(double), s);
    if (me != hipSuccess) { (void)hipGetLastError(); return (int)me; }          // the memset's OWN error, never PWC_OK
    const dim3 parts((unsigned)pwc_loss_parts(H, W), (unsigned)N);
    hipLaunchKernelGGL(flow_max_radius_kernel, parts, dim3(256), 0, s, flow, flow_cs, valid, H, W, flow_scale,
                       reinterpret_cast<unsigned long long*>(max_rad));
    return pwc_launch_status();
}

extern "C" int pwc_flow_vis_tiles_u8(const pwc_vis_tile* tiles, int ntiles, int N, int out_h, int out_w, uint8_t* out,
                                     pwc_stream_t stream) {
    if (!tiles || !out || ntiles < 1 || ntiles > PWC_VIS_MAX_TILES || N < 1 || out_h < 1 || out_w < 1) return PWC_EINVAL;
    for (int k = 0; k < ntiles; ++k) {
        const pwc_vis_tile& t = tiles[k];
        if (!t.src || t.src_h < 1 || t.src_w < 1 || t.tile_w < 1 || t.x0 < 0 || t.x0 > out_w - t.tile_w) return PWC_EINVAL;
        if (t.kind == PWC_VIS_FLOW) {
            if (!t.max_rad || t.src_cs < 2) return PWC_EINVAL;
        } else if (t.kind == PWC_VIS_ERROR) {
            if (!t.gt || t.src_cs < 2 || t.gt_cs < 2) return PWC_EINVAL;
        } else if (t.kind != PWC_VIS_FRAME_U8 && t.kind != PWC_VIS_FRAME_F32) {
            return PWC_EINVAL;
        }
    }
    if (!pwc_loss_in_range(N, out_h, out_w)) return PWC_ERANGE;
    for (int k = 0; k < ntiles; ++k)
        if (!pwc_loss_in_range(N, tiles[k].src_h, tiles[k].src_w)) return PWC_ERANGE;
    for (int k = 0; k < ntiles; ++k) {
        const pwc_vis_tile& t = tiles[k];
        if (t.kind != PWC_VIS_FRAME_U8 && pwc_off(t.src, 3u)) return PWC_EALIGN;
        if (t.kind == PWC_VIS_ERROR && pwc_off(t.gt, 3u)) return PWC_EALIGN;
        if (t.kind == PWC_VIS_FLOW && pwc_off(t.max_rad, 7u)) return PWC_EALIGN;
    }
    VisArgs a = {};
    for (int k = 0; k < ntiles; ++k) a.t[k] = tiles[k];
    a.out = out; a.npix = (long)N * out_h * out_w; a.ntiles = ntiles; a.out_h = out_h; a.out_w = out_w;
    a.dwords = pwc_off(out, 3u) ? 0 : 1;
    const long blocks = ((a.npix + 3) / 4 + 255) / 256;
    hipLaunchKernelGGL(flow_vis_tiles_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream, a);
    return pwc_launch_status();
}
