// pwc_interp.hip -- frame interpolation: the frames between two frames, from the two flows between them, by softmax splatting
// both frames to every time asked for and blending what arrives (gfx950; C ABI in include/pwc_hip.h, "frame interpolation";
// semantics, budget and launch plan in DESIGN.md 19).
//
//   pwc_interp_workspace_bytes   8 (N M H W 10 + 1): five 64-bit accumulators per direction, target pixel and time, the poison word
//   pwc_interp_frames            frames_t (N, M, H, W, 3) in the frames' dtype and source (N, M, H, W) bytes
//
// Three steps on the stream: the accumulators are zeroed, ONE scatter launch, ONE resolve launch.
//   scatter   a lane per source pixel and direction (k = 0: frame 0 along flows_fw, k = 1: frame 1 along flows_bw).  The lane
//             forms its pixel's weight ONCE -- the caller's, or exp(-min(alpha e, 10)) with e the mean absolute colour difference
//             between the pixel and the other frame sampled bilinearly where the flow points (pwc_fb_valid_u8's sample) -- and
//             then walks the M times: the target point p + s f, s = t (k = 0) or 1 - t (k = 1), pwc_splat's in-frame test and
//             corners, and per corner inside the frame five 64-bit integer atomics of 2^-36 steps: b w colour[0..2], b w, b.
//   resolve   a lane per run of four output pixels of the flat (N, M, H, W) index: per direction covered iff range >= min_range and
//             den > 0, colour = num / den, the blend (1 - t) c0 + t c1 of what is covered, the cross-fade of the co-located pixels
//             where nothing is, the source code 2 covered_1 + covered_0; twelve bytes (three dwords) or twelve floats per lane,
//             pwc_flowvis.hip's store arrangement.
// Every value is an IEEE double operation in the order written, no fused multiply-add is formed anywhere in this file (the pragma
// below): tests/interp_ref.py restates it in numpy operation for operation, exp is the only operation whose result may differ.
// Integer addition is associative: the order in which the atomics land cannot change a bit.
// The accumulators are PLANAR, [n][m][k][j][H W]: the lanes of a wave send neighbouring targets of one plane wherever the flow
// is smooth, and the resolve reads ten planes in runs of 32 bytes per lane.  A time's planes meet no other time's and an image's
// no other image's: a call cut along N or M gives the whole call's bits.
// Grids: scatter (min(ceil(N H W / 256), 4096), 2), resolve min(ceil(N M H W / 1024), 4096) workgroups of 256 lanes, grid-stride
// beyond.  No LDS, no host synchronisation, no process-wide state; 64-bit indices into the workspace.
#include "flow_record.h"
#include "loss_common.h"

#pragma clang fp contract(off)

// 2^36 steps per unit (pwc_splat.hip's fixed point): a contribution below 2^-37 vanishes, one that is not finite or reaches
// 2^26 raises the poison word, a cell at or beyond 2^61 is refused by the resolve.
#define INTERP_FIX 68719476736.0
#define INTERP_CLAMP 10.0

struct InterpArgs {
    const void* frame[2];     // [N][H][W] records of 3 bytes, or of frame_cs[k] floats, 3 used
    const float* flow[2];     // [N][H][W] records of flow_cs[k] floats, 2 used: 0 -> 1, 1 -> 0
    const uint8_t* valid[2];  // [N][H][W], null: every pixel
    const float* weight[2];   // [N][H][W], null: the photometric weight
    void* out;                // [N][M][H][W][3] bytes or floats
    uint8_t* source;          // [N][M][H][W]
    unsigned long long* fix;  // [N][M][2][5][H W], the poison word
    double times[PWC_INTERP_MAX_TIMES];
    int frame_cs[2], flow_cs[2];
    int N, M, H, W;
    float alpha, min_range;
    int out_vec, source_vec;  // out on a 4-byte (bytes) / 16-byte (floats) boundary, source on a 4-byte one
};

// The three channels of pixel `pix` of a frame as doubles: a byte v is v / 255, a float is widened.
template <bool U8>
__device__ __forceinline__ void interp_load(const void* frame, int cs, size_t pix, double* c) {
    if (U8) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(frame) + pix * 3;
        c[0] = (double)p[0] / 255.0; c[1] = (double)p[1] / 255.0; c[2] = (double)p[2] / 255.0;
    } else {
        const float* p = reinterpret_cast<const float*>(frame) + pix * cs;
        c[0] = (double)p[0]; c[1] = (double)p[1]; c[2] = (double)p[2];
    }
}

// One contribution (splat_add of pwc_splat.hip); returns whether it is out of the fixed point's range.
__device__ __forceinline__ bool interp_add(unsigned long long* dst, double v) {
    if (!(fabs(v) < 67108864.0)) return true;                              // (false for a NaN)
    const long long i = __double2ll_rn(v * INTERP_FIX);
    if (i) atomicAdd(dst, (unsigned long long)i);
    return false;
}

// The weight of source pixel (n, y, x) of direction k from the frames: exp(-min(alpha e, 10)), exp(-10) where the flow points out
// of the other frame.  The in-frame test is what keeps the four corner reads inside image n (fb_pixel's).
template <bool U8>
__device__ __forceinline__ double interp_match_weight(const InterpArgs& a, int k, int n, int y, int x, double f0, double f1,
                                                      const double* own) {
    const double qx = (double)x + f0, qy = (double)y + f1;
    if (!(qx >= 0.0 && qx <= (double)(a.W - 1) && qy >= 0.0 && qy <= (double)(a.H - 1))) return exp(-INTERP_CLAMP);
    const PwcBilinearF64 bl = pwc_bilinear_f64(qx, qy, a.H, a.W);
    const double wx0 = bl.wx0, wx1 = bl.wx1, wy0 = bl.wy0, wy1 = bl.wy1;
    const size_t img = (size_t)n * a.H * a.W;
    const void* other = a.frame[1 - k];
    const int cs = a.frame_cs[1 - k];
    double c00[3], c01[3], c10[3], c11[3];
    interp_load<U8>(other, cs, img + bl.o00, c00);
    interp_load<U8>(other, cs, img + bl.o01, c01);
    interp_load<U8>(other, cs, img + bl.o10, c10);
    interp_load<U8>(other, cs, img + bl.o11, c11);
    double e = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double top = wx0 * c00[c] + wx1 * c01[c], bot = wx0 * c10[c] + wx1 * c11[c];
        e = e + fabs(own[c] - (wy0 * top + wy1 * bot));
    }
    e = e / 3.0;
    const double ae = (double)a.alpha * e;
    return exp(-(ae < INTERP_CLAMP ? ae : INTERP_CLAMP));                  // (a NaN takes the clamp)
}

// grid (parts, 2): one lane per source pixel of direction blockIdx.y.
template <bool U8>
__global__ __launch_bounds__(256) void interp_scatter_kernel(const InterpArgs a) {
    const int k = blockIdx.y;
    const long npix = (long)a.N * a.H * a.W;
    const size_t hw = (size_t)a.H * a.W;
    unsigned long long* poison = a.fix + (size_t)a.N * a.M * 10 * hw;
    const float* flow = a.flow[k];
    const uint8_t* valid = a.valid[k];
    const float* weight = a.weight[k];
    const int fcs = a.flow_cs[k];
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        if (valid && !valid[p]) continue;
        const float fu = flow[p * fcs], fv = flow[p * fcs + 1];
        if (!pwc_flow_known(fu, fv)) continue;
        const PwcLossPixel q = pwc_loss_pixel(p, a.H, a.W);
        const double f0 = (double)fu, f1 = (double)fv;
        double col[3];
        interp_load<U8>(a.frame[k], a.frame_cs[k], (size_t)p, col);
        double w;
        if (weight) {
            w = (double)weight[p];
            if (!(w >= 0.0 && w < (double)INFINITY)) continue;             // (a NaN fails)
            if (w >= 67108864.0) { atomicOr(poison, 1ull); continue; }
        } else {
            w = interp_match_weight<U8>(a, k, q.n, q.y, q.x, f0, f1, col);
        }
        bool bad = false;
        for (int m = 0; m < a.M; ++m) {
            const double s = k == 0 ? a.times[m] : 1.0 - a.times[m];
            const double px = (double)q.x + s * f0, py = (double)q.y + s * f1;
            // (every comparison is false for a NaN; an Inf fails one of them)
            if (!(px > -1.0 && px < (double)a.W && py > -1.0 && py < (double)a.H)) continue;
            // (not pwc_bilinear_f64: a splat -- the position may lie up to a pixel outside, corners outside are dropped, not clipped)
            const double fx0 = floor(px), fy0 = floor(py);
            const int x0 = (int)fx0, y0 = (int)fy0;
            const double wx = px - fx0, wy = py - fy0;
            unsigned long long* plane = a.fix + (((size_t)q.n * a.M + m) * 10 + (size_t)k * 5) * hw;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int dx = c & 1, dy = c >> 1;
                const int cx = x0 + dx, cy = y0 + dy;
                if (cx < 0 || cx >= a.W || cy < 0 || cy >= a.H) continue;
                const double b = (dx ? wx : 1.0 - wx) * (dy ? wy : 1.0 - wy);
                const double bw = b * w;
                unsigned long long* t = plane + (size_t)cy * a.W + cx;
                bad |= interp_add(t, bw * col[0]);
                bad |= interp_add(t + hw, bw * col[1]);
                bad |= interp_add(t + 2 * hw, bw * col[2]);
                bad |= interp_add(t + 3 * hw, bw);
                bad |= interp_add(t + 4 * hw, b);
            }
        }
        if (bad) atomicOr(poison, 1ull);
    }
}

__device__ __forceinline__ bool interp_wild(long long v) { return v >= (1LL << 61) || v <= -(1LL << 61); }

// A double as a byte: rint(255 v), ties to even, clamped to [0, 255]; 0 for a NaN.  Not pwc_round_byte: the value is scaled first.
__device__ __forceinline__ unsigned interp_byte(double v) {
    return pwc_clamp_byte(rint(255.0 * v));
}

// Output pixel g of the flat (N, M, H, W) index: its three channels and its source code; false where the pixel is dead (the
// poison word, a wrapped cell).
template <bool U8>
__device__ __forceinline__ bool interp_pixel(const InterpArgs& a, long g, bool poisoned, double* v, unsigned& code) {
    const size_t hw = (size_t)a.H * a.W;
    const size_t pix = (size_t)g % hw;
    const size_t nm = (size_t)g / hw;
    const int n = (int)(nm / a.M), m = (int)(nm % a.M);
    const long long* cell = reinterpret_cast<const long long*>(a.fix) + nm * 10 * hw + pix;
    const double t = a.times[m];
    const double wgt[2] = {1.0 - t, t};
    double c[2][3];
    bool covered[2], dead = poisoned;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const long long n0 = cell[(k * 5 + 0) * hw], n1 = cell[(k * 5 + 1) * hw], n2 = cell[(k * 5 + 2) * hw];
        const long long den = cell[(k * 5 + 3) * hw], rng = cell[(k * 5 + 4) * hw];
        dead |= interp_wild(n0) || interp_wild(n1) || interp_wild(n2) || interp_wild(den) || interp_wild(rng);
        const double range = (double)rng * (1.0 / INTERP_FIX);
        covered[k] = range >= (double)a.min_range && den > 0;
        const double dd = (double)den;
        c[k][0] = (double)n0 / dd; c[k][1] = (double)n1 / dd; c[k][2] = (double)n2 / dd;        // (not used where den == 0)
    }
    code = (covered[0] ? 1u : 0u) | (covered[1] ? 2u : 0u);
    if (dead) { code = 0u; return false; }
    if (code == 0u) {                                                      // a hole: the cross-fade of the co-located pixels
        const size_t src = (size_t)n * hw + pix;
        interp_load<U8>(a.frame[0], a.frame_cs[0], src, c[0]);
        interp_load<U8>(a.frame[1], a.frame_cs[1], src, c[1]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
        v[j] = code == 1u ? c[0][j] : (code == 2u ? c[1][j] : wgt[0] * c[0][j] + wgt[1] * c[1][j]);
    return true;
}

// One lane per run of four output pixels.
template <bool U8>
__global__ __launch_bounds__(256) void interp_resolve_kernel(const InterpArgs a) {
    const long total = (long)a.N * a.M * a.H * a.W;
    const long runs = (total + 3) / 4;
    const bool poisoned = a.fix[(size_t)total * 10] != 0;
    const float nan = __builtin_nanf("");
    for (long r = blockIdx.x * 256L + threadIdx.x; r < runs; r += (long)gridDim.x * 256) {
        const long g0 = 4 * r;
        const bool whole = g0 + 4 <= total;
        unsigned codes = 0u, px[4] = {0u, 0u, 0u, 0u};
        float f[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (g0 + i >= total) break;
            double v[3];
            unsigned code;
            const bool ok = interp_pixel<U8>(a, g0 + i, poisoned, v, code);
            codes |= code << (8 * i);
            if (U8) {
                px[i] = ok ? interp_byte(v[0]) | (interp_byte(v[1]) << 8) | (interp_byte(v[2]) << 16) : 0u;
            } else {
                f[3 * i] = ok ? (float)v[0] : nan; f[3 * i + 1] = ok ? (float)v[1] : nan; f[3 * i + 2] = ok ? (float)v[2] : nan;
            }
        }
        if (a.source_vec && whole) {
            *reinterpret_cast<unsigned*>(a.source + g0) = codes;
        } else {
            for (int i = 0; i < 4 && g0 + i < total; ++i) a.source[g0 + i] = (uint8_t)((codes >> (8 * i)) & 255u);
        }
        if (U8) {
            uint8_t* o = reinterpret_cast<uint8_t*>(a.out) + 3 * g0;
            if (a.out_vec && whole) {
                unsigned* d = reinterpret_cast<unsigned*>(o);
                d[0] = px[0] | (px[1] << 24);
                d[1] = (px[1] >> 8) | (px[2] << 16);
                d[2] = (px[2] >> 16) | (px[3] << 8);
            } else {
                for (int i = 0; i < 4 && g0 + i < total; ++i) {
                    o[3 * i] = (uint8_t)(px[i] & 255u); o[3 * i + 1] = (uint8_t)((px[i] >> 8) & 255u); o[3 * i + 2] = (uint8_t)(px[i] >> 16);
                }
            }
        } else {
            float* o = reinterpret_cast<float*>(a.out) + 3 * g0;
            if (a.out_vec && whole) {
                f32x4* d = reinterpret_cast<f32x4*>(o);
                d[0] = f32x4{f[0], f[1], f[2], f[3]};
                d[1] = f32x4{f[4], f[5], f[6], f[7]};
                d[2] = f32x4{f[8], f[9], f[10], f[11]};
            } else {
                for (int i = 0; i < 4 && g0 + i < total; ++i) {
                    o[3 * i] = f[3 * i]; o[3 * i + 1] = f[3 * i + 1]; o[3 * i + 2] = f[3 * i + 2];
                }
            }
        }
    }
}

// ---------------------------------------------------------------- host
// Whether 8 (N M H W 10 + 1) bytes can be counted in a size_t at all.
static inline bool interp_countable(int N, int M, int H, int W) {
    const size_t per_image = (size_t)H * W * 10;                           // H W < 2^31
    return (size_t)N * M <= ((SIZE_MAX >> 4) - 1) / per_image;
}

extern "C" size_t pwc_interp_workspace_bytes(int N, int M, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || M < 1 || M > PWC_INTERP_MAX_TIMES) return 0;
    if ((long)H * W >= (1L << 31) || !interp_countable(N, M, H, W)) return 0;
    return ((size_t)N * M * H * W * 10 + 1) * sizeof(long long);
}

extern "C" int pwc_interp_frames(const void* frames_0, int dtype_0, int cs_0, const void* frames_1, int dtype_1, int cs_1,
                                 const float* flows_fw, int fw_cs, const float* flows_bw, int bw_cs, const uint8_t* valid_fw,
                                 const uint8_t* valid_bw, const float* weights_fw, const float* weights_bw, int N, int H, int W,
                                 const double* times, int M, float alpha, float min_range, void* workspace,
                                 size_t workspace_bytes, void* frames_t, uint8_t* source, pwc_stream_t stream) {
    if (!frames_0 || !frames_1 || !flows_fw || !flows_bw || !times || !workspace || !frames_t || !source) return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || M < 1 || M > PWC_INTERP_MAX_TIMES) return PWC_EINVAL;
    if (dtype_0 != dtype_1 || (dtype_0 != PWC_INTERP_U8 && dtype_0 != PWC_INTERP_F32)) return PWC_EINVAL;
    for (int m = 0; m < M; ++m)
        if (!(times[m] >= 0.0 && times[m] <= 1.0)) return PWC_EINVAL;      // (a NaN fails)
    if (!(alpha >= 0.f) || !(min_range >= 0.f)) return PWC_EINVAL;
    const bool u8 = dtype_0 == PWC_INTERP_U8;
    if (fw_cs < 2 || bw_cs < 2 || (u8 ? (cs_0 != 3 || cs_1 != 3) : (cs_0 < 3 || cs_1 < 3))) return PWC_EINVAL;
    if ((long)H * W >= (1L << 31) || !interp_countable(N, M, H, W)) return PWC_ERANGE;
    if (pwc_off(flows_fw, 3u) || pwc_off(flows_bw, 3u) || (weights_fw && pwc_off(weights_fw, 3u)) ||
        (weights_bw && pwc_off(weights_bw, 3u)) || pwc_off(workspace, 7u) ||
        (!u8 && (pwc_off(frames_0, 3u) || pwc_off(frames_1, 3u) || pwc_off(frames_t, 3u))))
        return PWC_EALIGN;
    const size_t bytes = pwc_interp_workspace_bytes(N, M, H, W);
    if (workspace_bytes < bytes) return PWC_EINVAL;
    InterpArgs a = {};
    a.frame[0] = frames_0; a.frame[1] = frames_1; a.flow[0] = flows_fw; a.flow[1] = flows_bw;
    a.valid[0] = valid_fw; a.valid[1] = valid_bw; a.weight[0] = weights_fw; a.weight[1] = weights_bw;
    a.out = frames_t; a.source = source; a.fix = reinterpret_cast<unsigned long long*>(workspace);
    for (int m = 0; m < M; ++m) a.times[m] = times[m];
    a.frame_cs[0] = cs_0; a.frame_cs[1] = cs_1; a.flow_cs[0] = fw_cs; a.flow_cs[1] = bw_cs;
    a.N = N; a.M = M; a.H = H; a.W = W; a.alpha = alpha; a.min_range = min_range;
    a.out_vec = pwc_off(frames_t, u8 ? 3u : 15u) ? 0 : 1;
    a.source_vec = pwc_off(source, 3u) ? 0 : 1;
    const hipStream_t s = (hipStream_t)stream;
    const hipError_t me = hipMemsetAsync(workspace, 0, bytes, s);
    if (me != hipSuccess) { (void)hipGetLastError(); return (int)me; }          // the memset's OWN error, never PWC_OK
    const dim3 sgrid(pwc_loss_grad_blocks(N, H, W).x, 2u);
    const dim3 rgrid = pwc_flat_grid(((long)N * M * H * W + 3) / 4);
    if (u8) {
        hipLaunchKernelGGL(interp_scatter_kernel<true>, sgrid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(interp_resolve_kernel<true>, rgrid, dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(interp_scatter_kernel<false>, sgrid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(interp_resolve_kernel<false>, rgrid, dim3(256), 0, s, a);
    }
    return pwc_launch_status();
}
