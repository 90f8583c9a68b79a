// pwc_compose.hip -- flow composition: the flow a -> c from the flows a -> b and b -> c, with a validity mask, and its gradient
// into BOTH flows (gfx950; C ABI in include/pwc_hip.h, "flow composition"; semantics, bounds and launch plan in DESIGN.md).
//
//   pwc_flow_compose_f32        out[p] = f + flow_bc sampled bilinearly at p + f, f = flow_ab[p]; valid[p] 0 / 1; an invalid
//                               pixel holds the .flo sentinel (1e10, 1e10)
//   pwc_flow_compose_grad_f32   the gradient of sum_p,k g[p,k] out[p,k] over the valid pixels with respect to both flows
//
// Pixel p = (n, y, x) is VALID iff valid_ab (where given) is non-zero at p, both components of f are finite with |.| <= 1e9 (the
// .flo sentinel rule), the sample point q = (x + f0, y + f1) lies in [0, W - 1] x [0, H - 1], and at each of the four clamped
// corners of q valid_bc (where given) is non-zero and both flow_bc components pass the sentinel rule -- all four whatever their
// weight.  Every decision is a branch: a pixel its mask rules out reads no flow, one whose f fails reads no corner, an invalid
// one reads no upstream gradient; a NaN in a place the rule excludes reaches no output.  Sample point, floor, weights (fb_valid's
// sample, word for word), the blend and the sum with f are doubles, rounded to float32 once.
// The gradient reaches flow_ab where the pixel stands (a gather, formed in double, rounded once) and flow_bc at the four corners
// (a scatter: several pixels share a corner).  The scatter adds 64-bit fixed-point integers of 2^-36 steps with integer atomics,
// as pwc_fbcheck.hip and pwc_splat.hip do -- integer addition is associative, the order in which the atomics land changes no
// bit.  Unlike there the upstream gradient varies per pixel and its scale is arbitrary (a loss mean puts it near 1 / (N H W)), so
// the step is RELATIVE: a first launch forms per image m_n = max |g| over the valid pixels (an integer atomicMax on the bits of
// non-negative floats: order independent, it stays on the device), contributions are scaled by the exact power of two 2^-e_n,
// m_n <= 2^e_n < 2 m_n, before conversion, and the finish converts each accumulator once and scales back.  The bits of |NaN| and
// |Inf| compare at or above Inf's, so the same word is the image's poison flag: every element of dflow_bc[n] is then NaN.
// Per image: two calls give the same bits, an image gives the same bits alone and in a batch, g times a power of two gives the
// gradient times that power of two.
// One lane per pixel.  Flows at any channel stride >= 2: where every flow pointer of a call is on an 8-byte boundary and every
// channel stride is even a pixel's two components are one 8-byte access, else two 4-byte ones -- the values fetched, and so
// every bit, are the same (flow_record.h).
#include "loss_common.h"
#include "flow_record.h"

#pragma clang fp contract(fast)   // (flow_record.h turns contraction off behind it; this file's arithmetic is contracted)

struct ComposeArgs {
    const float* ab;          // [N][H][W] records of ab_cs floats, 2 used
    const float* bc;
    const uint8_t* vab;       // [N][H][W], null: every pixel
    const uint8_t* vbc;
    float* out;               // (forward)
    uint8_t* vout;            // (forward) [N][H][W] 0 / 1
    const float* g;           // (grad) upstream, [N][H][W] records of g_cs floats
    float* dab;               // (grad)
    float* dbc;               // (grad)
    long long* fix;           // (grad) [N][H][W][2] accumulators
    unsigned* gmax;           // (grad) [N] words at a stride of 2: the bits of m_n
    int ab_cs, bc_cs, out_cs, g_cs, dab_cs, dbc_cs;
    int N, H, W;
    int accumulate;
};

// What a valid pixel holds: f, the flat indices of its four corners in flow_bc, the weights along x and y, the corner values.
struct ComposeSample {
    double f[2];
    size_t o00, o01, o10, o11;
    double wx0, wx1, wy0, wy1;
    double v00[2], v01[2], v10[2], v11[2];
};

// Pixel (n, y, x), pix = its flat index: whether it is valid.  The in-frame test is what keeps the four corner reads inside
// image n: 0 <= x0 <= x1 <= W - 1 and the same in y follow from it.
template <bool VEC>
__device__ __forceinline__ bool compose_pixel(const ComposeArgs& a, int n, int y, int x, size_t pix, ComposeSample& s) {
    if (a.vab && !a.vab[pix]) return false;
    float f0, f1;
    pwc_flow_load2<VEC>(a.ab + pix * a.ab_cs, f0, f1);
    if (!pwc_flow_known(f0, f1)) return false;
    const double qx = (double)x + (double)f0, qy = (double)y + (double)f1;
    if (!(qx >= 0.0 && qx <= (double)(a.W - 1) && qy >= 0.0 && qy <= (double)(a.H - 1))) return false;
    const PwcBilinearF64 bl = pwc_bilinear_f64(qx, qy, a.H, a.W);
    s.wx1 = bl.wx1; s.wy1 = bl.wy1; s.wx0 = bl.wx0; s.wy0 = bl.wy0;
    const size_t img = (size_t)n * a.H * a.W;
    s.o00 = img + bl.o00; s.o01 = img + bl.o01; s.o10 = img + bl.o10; s.o11 = img + bl.o11;
    if (a.vbc && !(a.vbc[s.o00] && a.vbc[s.o01] && a.vbc[s.o10] && a.vbc[s.o11])) return false;
    float c00[2], c01[2], c10[2], c11[2];
    pwc_flow_load2<VEC>(a.bc + s.o00 * a.bc_cs, c00[0], c00[1]);
    pwc_flow_load2<VEC>(a.bc + s.o01 * a.bc_cs, c01[0], c01[1]);
    pwc_flow_load2<VEC>(a.bc + s.o10 * a.bc_cs, c10[0], c10[1]);
    pwc_flow_load2<VEC>(a.bc + s.o11 * a.bc_cs, c11[0], c11[1]);
    if (!(pwc_flow_known(c00[0], c00[1]) && pwc_flow_known(c01[0], c01[1]) && pwc_flow_known(c10[0], c10[1]) &&
          pwc_flow_known(c11[0], c11[1])))
        return false;
    s.f[0] = (double)f0; s.f[1] = (double)f1;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        s.v00[k] = (double)c00[k]; s.v01[k] = (double)c01[k]; s.v10[k] = (double)c10[k]; s.v11[k] = (double)c11[k];
    }
    return true;
}

// One lane per pixel of the batch.
template <bool VEC>
__global__ __launch_bounds__(256) void flow_compose_kernel(const ComposeArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel px = pwc_loss_pixel(p, a.H, a.W);
        ComposeSample s;
        const bool ok = compose_pixel<VEC>(a, px.n, px.y, px.x, (size_t)p, s);
        float o0 = PWC_FLOW_SENTINEL, o1 = PWC_FLOW_SENTINEL;
        if (ok) {
            const double t0 = s.wx0 * s.v00[0] + s.wx1 * s.v01[0], b0 = s.wx0 * s.v10[0] + s.wx1 * s.v11[0];
            const double t1 = s.wx0 * s.v00[1] + s.wx1 * s.v01[1], b1 = s.wx0 * s.v10[1] + s.wx1 * s.v11[1];
            o0 = (float)(s.f[0] + (s.wy0 * t0 + s.wy1 * b0));
            o1 = (float)(s.f[1] + (s.wy0 * t1 + s.wy1 * b1));
        }
        pwc_flow_store2<VEC>(a.out + p * a.out_cs, o0, o1);
        a.vout[p] = ok ? 1 : 0;
    }
}

// ---------------------------------------------------------------- gradient
// 2^36 steps per unit of the image's scale 2^e_n, as pwc_fbcheck.hip's FBC_FIX per unit.
#define COMPOSE_FIX 68719476736.0
#define COMPOSE_INF_BITS 0x7f800000u

// The least e with m <= 2^e, for a finite m > 0: m <= 2^e < 2 m.
__device__ __forceinline__ int compose_exponent(float m) {
    int ex;
    const double fr = frexp((double)m, &ex);                              // m = fr 2^ex, fr in [0.5, 1)
    return fr == 0.5 ? ex - 1 : ex;
}

// grid (parts, N): the largest |g| over the valid pixels of image n, as the bits of a non-negative float -- they order as
// unsigned integers do, |Inf| and |NaN| at or above COMPOSE_INF_BITS.  A workgroup takes the maximum of its lanes in LDS and
// adds one atomic.
template <bool VEC>
__global__ __launch_bounds__(256) void flow_compose_max_kernel(const ComposeArgs a) {
    __shared__ unsigned red[256];
    const int n = blockIdx.y;
    const int npix = a.H * a.W;
    unsigned m = 0u;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
        const int y = p / a.W, x = p - y * a.W;
        const size_t pix = (size_t)n * npix + p;
        ComposeSample s;
        if (!compose_pixel<VEC>(a, n, y, x, pix, s)) continue;
        float g0, g1;
        pwc_flow_load2<VEC>(a.g + pix * a.g_cs, g0, g1);
        m = max(m, max(__float_as_uint(fabsf(g0)), __float_as_uint(fabsf(g1))));
    }
    const int t = threadIdx.x;
    red[t] = m;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) red[t] = max(red[t], red[t + k]);
        __syncthreads();
    }
    if (t == 0 && red[0]) atomicMax(a.gmax + 2 * (size_t)n, red[0]);
}

// One lane per pixel of the batch: the gather into dflow_ab, and the corner weight * g / 2^e_n of a valid pixel into flow_bc's
// accumulators.  An image whose maximum is 0 scatters nothing (exact zeros), a poisoned one nothing either (the finish writes
// NaN); dflow_ab is plain arithmetic in both.
template <bool VEC>
__global__ __launch_bounds__(256) void flow_compose_scatter_kernel(const ComposeArgs a) {
    unsigned long long* fix = reinterpret_cast<unsigned long long*>(a.fix);
    const long npix = (long)a.N * a.H * a.W;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel px = pwc_loss_pixel(p, a.H, a.W);
        float* o = a.dab + p * a.dab_cs;
        ComposeSample s;
        if (!compose_pixel<VEC>(a, px.n, px.y, px.x, (size_t)p, s)) {
            pwc_grad_skip2(o, a.accumulate);
            continue;
        }
        float gf0, gf1;
        pwc_flow_load2<VEC>(a.g + p * a.g_cs, gf0, gf1);
        const double g[2] = {(double)gf0, (double)gf1};
        // d S_k / d qx, d S_k / d qy: 0 where the clamp made the two corners one pixel (the difference of a value with itself)
        double dx = 0.0, dy = 0.0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            dx += g[k] * (s.wy0 * (s.v01[k] - s.v00[k]) + s.wy1 * (s.v11[k] - s.v10[k]));
            dy += g[k] * (s.wx0 * (s.v10[k] - s.v00[k]) + s.wx1 * (s.v11[k] - s.v01[k]));
        }
        pwc_grad_store2(o, a.accumulate, 1.f, (float)(g[0] + dx), (float)(g[1] + dy));
        const unsigned mb = a.gmax[2 * (size_t)px.n];
        if (mb == 0u || mb >= COMPOSE_INF_BITS) continue;
        const double scale = ldexp(COMPOSE_FIX, -compose_exponent(__uint_as_float(mb)));     // exact: a power of two
        const double w00 = s.wy0 * s.wx0, w01 = s.wy0 * s.wx1, w10 = s.wy1 * s.wx0, w11 = s.wy1 * s.wx1;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double gk = g[k] * scale;                                // exact; |gk| <= 2^36
            atomicAdd(fix + 2 * s.o00 + k, (unsigned long long)__double2ll_rn(w00 * gk));
            atomicAdd(fix + 2 * s.o01 + k, (unsigned long long)__double2ll_rn(w01 * gk));
            atomicAdd(fix + 2 * s.o10 + k, (unsigned long long)__double2ll_rn(w10 * gk));
            atomicAdd(fix + 2 * s.o11 + k, (unsigned long long)__double2ll_rn(w11 * gk));
        }
    }
}

// One lane per pixel of flow_bc: each accumulator converted once and scaled back by the image's power of two.
__global__ __launch_bounds__(256) void flow_compose_finish_kernel(const ComposeArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const int n = (int)(p / ((long)a.H * a.W));
        float* o = a.dbc + p * a.dbc_cs;
        const unsigned mb = a.gmax[2 * (size_t)n];
        if (mb >= COMPOSE_INF_BITS) {                                      // every element, whatever accumulate holds
            o[0] = __builtin_nanf("");
            o[1] = __builtin_nanf("");
            continue;
        }
        if (mb == 0u) {
            pwc_grad_skip2(o, a.accumulate);
            continue;
        }
        const double back = ldexp(1.0 / COMPOSE_FIX, compose_exponent(__uint_as_float(mb)));
        // a sum at or beyond 2^61 (2^25 in units of the image's scale) is where in-range contributions start to wrap the 64-bit
        // sum: NaN instead of a finite wrong value
        const long long v0 = a.fix[2 * p], v1 = a.fix[2 * p + 1];
        const float t0 = (v0 >= (1LL << 61) || v0 <= -(1LL << 61)) ? __builtin_nanf("") : (float)((double)v0 * back);
        const float t1 = (v1 >= (1LL << 61) || v1 <= -(1LL << 61)) ? __builtin_nanf("") : (float)((double)v1 * back);
        pwc_grad_store2(o, a.accumulate, 1.f, t0, t1);
    }
}

// ---------------------------------------------------------------- host
// per pixel and channel an accumulator, per image the word of its maximum (8 bytes each)
static inline size_t compose_fix_words(int N, int H, int W) { return (size_t)N * H * W * 2 + (size_t)N; }

extern "C" size_t pwc_flow_compose_grad_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || !pwc_loss_in_range(N, H, W)) return 0;
    return compose_fix_words(N, H, W) * sizeof(long long);
}

extern "C" int pwc_flow_compose_f32(const float* flow_ab, int ab_cs, const float* flow_bc, int bc_cs, const uint8_t* valid_ab,
                                    const uint8_t* valid_bc, int N, int H, int W, float* flow_ac, int ac_cs, uint8_t* valid_ac,
                                    pwc_stream_t stream) {
    if (!flow_ab || !flow_bc || !flow_ac || !valid_ac || N < 1 || H < 1 || W < 1 || ab_cs < 2 || bc_cs < 2 || ac_cs < 2)
        return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (pwc_off(flow_ab, 3u) || pwc_off(flow_bc, 3u) || pwc_off(flow_ac, 3u)) return PWC_EALIGN;
    ComposeArgs a = {};
    a.ab = flow_ab; a.bc = flow_bc; a.vab = valid_ab; a.vbc = valid_bc; a.out = flow_ac; a.vout = valid_ac;
    a.ab_cs = ab_cs; a.bc_cs = bc_cs; a.out_cs = ac_cs; a.N = N; a.H = H; a.W = W;
    const bool vec = pwc_flow_vec(ab_cs | bc_cs | ac_cs, {flow_ab, flow_bc, flow_ac});
    const dim3 grid = pwc_loss_grad_blocks(N, H, W);
    if (vec) hipLaunchKernelGGL(flow_compose_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(flow_compose_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return pwc_launch_status();
}

extern "C" int pwc_flow_compose_grad_f32(const float* flow_ab, int ab_cs, const float* flow_bc, int bc_cs, const uint8_t* valid_ab,
                                         const uint8_t* valid_bc, int N, int H, int W, const float* g, int g_cs, void* workspace,
                                         size_t workspace_bytes, float* dflow_ab, int dab_cs, float* dflow_bc, int dbc_cs,
                                         int accumulate, pwc_stream_t stream) {
    if (!flow_ab || !flow_bc || !g || !dflow_ab || !dflow_bc || N < 1 || H < 1 || W < 1 || ab_cs < 2 || bc_cs < 2 || g_cs < 2 ||
        dab_cs < 2 || dbc_cs < 2)
        return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (pwc_off(flow_ab, 3u) || pwc_off(flow_bc, 3u) || pwc_off(g, 3u) || pwc_off(dflow_ab, 3u) ||
        pwc_off(dflow_bc, 3u))
        return PWC_EALIGN;
    if (!workspace) return PWC_EINVAL;
    if (pwc_off(workspace, 7u)) return PWC_EALIGN;
    if (workspace_bytes < pwc_flow_compose_grad_workspace_bytes(N, H, W)) return PWC_EINVAL;
    ComposeArgs a = {};
    a.ab = flow_ab; a.bc = flow_bc; a.vab = valid_ab; a.vbc = valid_bc; a.g = g; a.dab = dflow_ab; a.dbc = dflow_bc;
    a.fix = reinterpret_cast<long long*>(workspace);
    a.gmax = reinterpret_cast<unsigned*>(a.fix + (size_t)N * H * W * 2);
    a.ab_cs = ab_cs; a.bc_cs = bc_cs; a.g_cs = g_cs; a.dab_cs = dab_cs; a.dbc_cs = dbc_cs; a.N = N; a.H = H; a.W = W;
    a.accumulate = accumulate ? 1 : 0;
    const hipStream_t s = (hipStream_t)stream;
    const hipError_t me = hipMemsetAsync(workspace, 0, compose_fix_words(N, H, W) * sizeof(long long), s);
    if (me != hipSuccess) { (void)hipGetLastError(); return (int)me; }          // the memset's OWN error, never PWC_OK
    // (dflow_ab and dflow_bc are stored 4 bytes at a time through pwc_grad_store2: their parity does not matter)
    const bool vec = pwc_flow_vec(ab_cs | bc_cs | g_cs, {flow_ab, flow_bc, g});
    const dim3 parts((unsigned)pwc_loss_parts(H, W), (unsigned)N);
    const dim3 grid = pwc_loss_grad_blocks(N, H, W);
    if (vec) {
        hipLaunchKernelGGL(flow_compose_max_kernel<true>, parts, dim3(256), 0, s, a);
        hipLaunchKernelGGL(flow_compose_scatter_kernel<true>, grid, dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(flow_compose_max_kernel<false>, parts, dim3(256), 0, s, a);
        hipLaunchKernelGGL(flow_compose_scatter_kernel<false>, grid, dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(flow_compose_finish_kernel, grid, dim3(256), 0, s, a);
    return pwc_launch_status();
}
