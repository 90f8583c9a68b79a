// pwc_splat.hip -- forward splatting: the pixels of a frame moved to where a flow sends them (gfx950; C ABI in include/pwc_hip.h,
// "forward splatting").  Every other geometric op of the library gathers along the flow; this one scatters.
//
//   pwc_splat_f32        out[target, c] = sum over the source pixels of (bilinear weight) * w * x[c], the coverage (the splatted w),
//                        and with `normalize` out / coverage where the coverage is positive
//   pwc_splat_grad_f32   its transpose: the gradient with respect to x, w and the flow, a gather
//
// Source pixel (y, x) has the target point px = x + s * f0, py = y + s * f1 (double; the product of two floats is exact in a
// double, so px is the sum rounded once however the compiler contracts it).  It contributes iff its mask passes and
// px > -1 && px < W && py > -1 && py < H -- written so that a NaN fails every comparison, as fb_pixel does.  x0 = floor(px),
// wx = px - x0, likewise y; the four corners (y0 + dy, x0 + dx) carry (dx ? wx : 1 - wx) * (dy ? wy : 1 - wy), and EACH corner
// contributes on its own iff it lies inside the frame (UFlow's compute_range_map, softsplat): a point half a pixel outside still
// splats onto the border.  Nothing is clamped.
// Several sources share a target, so the scatter adds 64-bit fixed-point integers of 2^-36 steps, as fb_consistency_scatter_kernel
// (pwc_fbcheck.hip) and the deterministic warp gradient (pwc_backward.hip) do: integer addition is associative, the order in
// which the atomics land cannot change a bit.  Three steps on the stream: the accumulators are zeroed, one lane per source pixel
// scatters, one lane per target pixel converts each accumulator once.  No LDS privatisation: the targets of a workgroup's 256
// sources are as spread as the flow makes them, and a flow that sends a whole frame to one pixel is a test, not a workload.
#include "loss_common.h"

// 2^36 steps per unit: a contribution below 2^-37 vanishes, one that is not finite or reaches 2^26 raises the poison word
// (__double2ll_rn would turn a NaN into 0 and saturate an Inf), a cell holds |sum| < 2^25 before the finish refuses it.
#define SPLAT_FIX 68719476736.0

struct SplatArgs {
    const float* x;           // [N][H][W] records of x_cs floats, C used; null with C == 0
    const float* flow;
    const float* w;           // [N][H][W] per-source weight, null: 1
    const uint8_t* valid;     // [N][H][W] source mask, null: every pixel
    const float* g_out;       // (grad) upstream of out, null: zeros
    const float* g_cov;       // (grad) upstream of the coverage, null: zeros
    float* out;
    float* cov;
    float* dx;                // (grad) any of the three may be null
    float* dw;
    float* dflow;
    long long* fix;           // [N][H][W][C] numerators, [N][H][W] denominators, the poison word
    int x_cs, flow_cs, out_cs, g_cs, dx_cs, dflow_cs;
    int N, H, W, C;
    float flow_scale;
    int normalize, accumulate;
};

// The cell a contributing source pixel lands in.  x0 is in [-1, W - 1], y0 in [-1, H - 1].
struct SplatCell {
    int x0, y0;
    double wx, wy;
};

__device__ __forceinline__ bool splat_pixel(const SplatArgs& a, long p, int y, int x, SplatCell& s) {
    if (a.valid && !a.valid[p]) return false;
    const float* fp = a.flow + p * a.flow_cs;
    const double sc = (double)a.flow_scale;
    const double px = (double)x + sc * (double)fp[0], py = (double)y + sc * (double)fp[1];
    // (every comparison is false for a NaN; an Inf fails one of them)
    if (!(px > -1.0 && px < (double)a.W && py > -1.0 && py < (double)a.H)) return false;
    const double fx0 = floor(px), fy0 = floor(py);
    s.x0 = (int)fx0; s.y0 = (int)fy0;
    s.wx = px - fx0; s.wy = py - fy0;
    return true;
}

// Corner k = 2 dy + dx of a cell: whether it is inside the frame, its flat pixel index, its weight.
__device__ __forceinline__ bool splat_corner(const SplatArgs& a, const SplatCell& s, int n, int k, long& t, double& b) {
    const int dx = k & 1, dy = k >> 1;
    const int cx = s.x0 + dx, cy = s.y0 + dy;
    if (cx < 0 || cx >= a.W || cy < 0 || cy >= a.H) return false;
    t = ((long)n * a.H + cy) * a.W + cx;
    b = (dx ? s.wx : 1.0 - s.wx) * (dy ? s.wy : 1.0 - s.wy);
    return true;
}

// One contribution; returns whether it is out of the fixed point's range.  A contribution that rounds to no step adds nothing.
__device__ __forceinline__ bool splat_add(unsigned long long* dst, double v) {
    if (!(fabs(v) < 67108864.0)) return true;                              // (false for a NaN)
    const long long i = __double2ll_rn(v * SPLAT_FIX);
    if (i) atomicAdd(dst, (unsigned long long)i);
    return false;
}

__global__ __launch_bounds__(256) void splat_scatter_kernel(const SplatArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    unsigned long long* num = reinterpret_cast<unsigned long long*>(a.fix);
    unsigned long long* den = num + npix * a.C;
    unsigned long long* poison = den + npix;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel q = pwc_loss_pixel(p, a.H, a.W);
        SplatCell s;
        if (!splat_pixel(a, p, q.y, q.x, s)) continue;
        const double wt = a.w ? (double)a.w[p] : 1.0;
        const float* xp = a.x + p * a.x_cs;                                // (not read with C == 0)
        bool bad = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            long t;
            double b;
            if (!splat_corner(a, s, q.n, k, t, b)) continue;
            const double bw = b * wt;
            bad |= splat_add(den + t, bw);
            for (int c = 0; c < a.C; ++c) bad |= splat_add(num + t * a.C + c, bw * (double)xp[c]);
        }
        if (bad) atomicOr(poison, 1ull);
    }
}

__device__ __forceinline__ bool splat_wild(long long v) { return v >= (1LL << 61) || v <= -(1LL << 61); }

// One lane per TARGET pixel: each accumulator converted once.  A sum at or beyond 2^61 is where in-range contributions start to
// wrap the 64-bit sum: NaN instead of a finite wrong value.
__global__ __launch_bounds__(256) void splat_finish_kernel(const SplatArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    const long long* num = a.fix;
    const long long* den = num + npix * a.C;
    const bool poisoned = den[npix] != 0;
    const float nan = __builtin_nanf("");
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const long long d = den[p];
        const bool dead = poisoned || splat_wild(d);
        const double dd = (double)d * (1.0 / SPLAT_FIX);
        a.cov[p] = dead ? nan : (float)dd;
        float* o = a.out + p * a.out_cs;
        for (int c = 0; c < a.C; ++c) {
            const long long v = num[p * a.C + c];
            const double vv = (double)v * (1.0 / SPLAT_FIX);
            float r;
            if (poisoned || splat_wild(v) || (a.normalize && dead)) r = nan;
            else if (a.normalize) r = d > 0 ? (float)(vv / dd) : 0.f;
            else r = (float)vv;
            o[c] = r;
        }
    }
}

// pwc_grad_store2's rule for one value: written, or (accumulate) added as fma(1, v, d) = d + v.
__device__ __forceinline__ void splat_store1(float* d, int accumulate, float v) {
    d[0] = accumulate ? __builtin_fmaf(1.f, v, d[0]) : v;
}

// One lane per SOURCE pixel: the transpose of the scatter is a gather over the pixel's own in-frame corners.  Every value is
// formed in double and rounded once.  With normalize the chain rule through out = num / den sits here, on the forward's own
// accumulators (g_num = g / den, g_den = g_cov - sum_c out_c g_c / den, both 0 where den is not positive), so that no rounded
// fp32 output enters a gradient.
__global__ __launch_bounds__(256) void splat_grad_kernel(const SplatArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    const long long* num = a.fix;
    const long long* den = num + npix * a.C;
    const bool poisoned = a.normalize && den[npix] != 0;
    const float nan = __builtin_nanf("");
    const double sc = (double)a.flow_scale;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel q = pwc_loss_pixel(p, a.H, a.W);
        float* dxp = a.dx ? a.dx + p * a.dx_cs : nullptr;
        float* dfp = a.dflow ? a.dflow + p * a.dflow_cs : nullptr;
        if (poisoned) {                                                    // every element, whatever accumulate holds
            for (int c = 0; dxp && c < a.C; ++c) dxp[c] = nan;
            if (a.dw) a.dw[p] = nan;
            if (dfp) { dfp[0] = nan; dfp[1] = nan; }
            continue;
        }
        SplatCell s;
        if (!splat_pixel(a, p, q.y, q.x, s)) {
            if (!a.accumulate) {
                for (int c = 0; dxp && c < a.C; ++c) dxp[c] = 0.f;
                if (a.dw) a.dw[p] = 0.f;
            }
            if (dfp) pwc_grad_skip2(dfp, a.accumulate);
            continue;
        }
        const double wt = a.w ? (double)a.w[p] : 1.0;
        bool ok[4];
        long t[4];
        double b[4], bx[4], by[4], dn[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            t[k] = 0; b[k] = 0.0;
            ok[k] = splat_corner(a, s, q.n, k, t[k], b[k]);
            // d b / d px = -+(1 - wy), -+wy;  d b / d py = -+(1 - wx), -+wx
            bx[k] = ((k & 1) ? 1.0 : -1.0) * ((k >> 1) ? s.wy : 1.0 - s.wy);
            by[k] = ((k >> 1) ? 1.0 : -1.0) * ((k & 1) ? s.wx : 1.0 - s.wx);
            dn[k] = (a.normalize && ok[k]) ? (double)den[t[k]] * (1.0 / SPLAT_FIX) : 0.0;
        }
        double dws = 0.0, fx = 0.0, fy = 0.0;
        const float* xp = a.x + p * a.x_cs;                                // (not read with C == 0)
        for (int c = 0; c < a.C; ++c) {
            double S = 0.0, Sx = 0.0, Sy = 0.0, D = 0.0, Dx = 0.0, Dy = 0.0;
            if (a.g_out) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!ok[k]) continue;
                    double g = (double)a.g_out[t[k] * a.g_cs + c], e = 0.0;
                    if (a.normalize) {
                        if (dn[k] > 0.0) {
                            g = g / dn[k];
                            e = -(((double)num[t[k] * a.C + c] * (1.0 / SPLAT_FIX)) / dn[k]) * g;
                        } else {
                            g = 0.0;
                        }
                    }
                    S += b[k] * g; Sx += bx[k] * g; Sy += by[k] * g;
                    D += b[k] * e; Dx += bx[k] * e; Dy += by[k] * e;
                }
            }
            if (dxp) splat_store1(dxp + c, a.accumulate, (float)(wt * S));
            const double xc = (double)xp[c];
            dws += xc * S + D; fx += xc * Sx + Dx; fy += xc * Sy + Dy;
        }
        if (a.g_cov) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!ok[k]) continue;
                const double g = (double)a.g_cov[t[k]];
                dws += b[k] * g; fx += bx[k] * g; fy += by[k] * g;
            }
        }
        if (a.dw) splat_store1(a.dw + p, a.accumulate, (float)dws);
        if (dfp) pwc_grad_store2(dfp, a.accumulate, 1.f, (float)(sc * wt * fx), (float)(sc * wt * fy));
    }
}

// The largest channel count: a lane walks its pixel's channels one by one, a record of x stays within a few cache lines.
#define SPLAT_MAX_C 64

static inline size_t splat_fix_words(int N, int H, int W, int C) { return (size_t)N * H * W * ((size_t)C + 1) + 1; }

extern "C" size_t pwc_splat_workspace_bytes(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || C < 0 || C > SPLAT_MAX_C) return 0;
    return splat_fix_words(N, H, W, C) * sizeof(long long);
}

// The checks both entry points share, in the order they report.
static int splat_check(const float* x, int x_cs, const float* flow, int flow_cs, int N, int H, int W, int C) {
    if (!flow || N <= 0 || H <= 0 || W <= 0 || C < 0 || (C > 0 && !x)) return PWC_EINVAL;
    if (C > SPLAT_MAX_C) return PWC_EUNSUPPORTED;
    if (flow_cs < 2 || x_cs < C) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    return PWC_OK;
}

static int splat_workspace_check(const void* workspace, size_t workspace_bytes, int N, int H, int W, int C) {
    if (!workspace) return PWC_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return PWC_EALIGN;
    if (workspace_bytes < pwc_splat_workspace_bytes(N, H, W, C)) return PWC_EINVAL;
    return PWC_OK;
}

extern "C" int pwc_splat_f32(const float* x, int x_cs, const float* flow, int flow_cs, float flow_scale, const float* w,
                             const uint8_t* valid, int N, int H, int W, int C, int normalize, void* workspace,
                             size_t workspace_bytes, float* out, int out_cs, float* coverage, pwc_stream_t stream) {
    int rc = splat_check(x, x_cs, flow, flow_cs, N, H, W, C);
    if (rc != PWC_OK) return rc;
    if (!coverage || (C > 0 && (!out || out_cs < C))) return PWC_EINVAL;
    rc = splat_workspace_check(workspace, workspace_bytes, N, H, W, C);
    if (rc != PWC_OK) return rc;
    SplatArgs a = {};
    a.x = x; a.flow = flow; a.w = w; a.valid = valid; a.out = out; a.cov = coverage;
    a.fix = reinterpret_cast<long long*>(workspace);
    a.x_cs = x_cs; a.flow_cs = flow_cs; a.out_cs = out_cs; a.N = N; a.H = H; a.W = W; a.C = C;
    a.flow_scale = flow_scale; a.normalize = normalize ? 1 : 0;
    const hipError_t me = hipMemsetAsync(workspace, 0, splat_fix_words(N, H, W, C) * sizeof(long long), (hipStream_t)stream);
    if (me != hipSuccess) { (void)hipGetLastError(); return (int)me; }          // the memset's OWN error, never PWC_OK
    const dim3 grid = pwc_loss_grad_blocks(N, H, W);
    hipLaunchKernelGGL(splat_scatter_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(splat_finish_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    return pwc_launch_status();
}

extern "C" int pwc_splat_grad_f32(const float* x, int x_cs, const float* flow, int flow_cs, float flow_scale, const float* w,
                                  const uint8_t* valid, int N, int H, int W, int C, int normalize, const float* g_out, int g_cs,
                                  const float* g_cov, const void* workspace, size_t workspace_bytes, float* dx, int dx_cs,
                                  float* dw, float* dflow, int dflow_cs, int accumulate, pwc_stream_t stream) {
    int rc = splat_check(x, x_cs, flow, flow_cs, N, H, W, C);
    if (rc != PWC_OK) return rc;
    if (!dx && !dw && !dflow) return PWC_EINVAL;
    if ((g_out && g_cs < C) || (dx && dx_cs < C) || (dflow && dflow_cs < 2)) return PWC_EINVAL;
    if (normalize) {                                                       // the forward's accumulators
        rc = splat_workspace_check(workspace, workspace_bytes, N, H, W, C);
        if (rc != PWC_OK) return rc;
    }
    SplatArgs a = {};
    a.x = x; a.flow = flow; a.w = w; a.valid = valid; a.g_out = g_out; a.g_cov = g_cov;
    a.dx = C > 0 ? dx : nullptr; a.dw = dw; a.dflow = dflow;
    a.fix = normalize ? const_cast<long long*>(reinterpret_cast<const long long*>(workspace)) : nullptr;
    a.x_cs = x_cs; a.flow_cs = flow_cs; a.g_cs = g_cs; a.dx_cs = dx_cs; a.dflow_cs = dflow_cs;
    a.N = N; a.H = H; a.W = W; a.C = C;
    a.flow_scale = flow_scale; a.normalize = normalize ? 1 : 0; a.accumulate = accumulate;
    hipLaunchKernelGGL(splat_grad_kernel, pwc_loss_grad_blocks(N, H, W), dim3(256), 0, (hipStream_t)stream, a);
    return pwc_launch_status();
}
