// pwc_distill.hip -- self-supervised flow distillation: the flow of a narrow view (the student) against the flow the same
// network gave on a wider view (the teacher), read in place through a window (gfx950; C ABI in include/pwc_hip.h, "flow
// distillation"; semantics and bounds in DESIGN.md).
//
//   pwc_flow_distill_sums_f32   per image the sum of rho(student[p,0] - teacher[P,0]) + rho(student[p,1] - teacher[P,1]) over the
//                               contributing student pixels p = (y, x), P = (y + y0, x + x0), and their number
//   pwc_flow_distill_grad_f32   the gradient of those sums, times an upstream gradient per image, with respect to the student
//
// A pixel contributes iff teacher_valid (where given) is non-zero at P, exclude (where given) is zero at p, both teacher components
// are finite with |.| <= 1e9 (the .flo sentinel rule) and both student components are finite.  A pixel a mask rules out reads no
// flow; one that does not contribute adds nothing and gets a zero gradient: a NaN never reaches a sum or a gradient through it.
// rho(d) = (d^2 + eps^2)^q and its derivative are formed in DOUBLE here (loss_common.h's unsup_rho is fp32): d is the exact
// difference of two floats, a pixel's two terms are added in double, the sums stay doubles through loss_common.h's two stages
// -- part b of pwc_loss_parts(h, w) takes the pixels b * 256 + t, + parts * 256, ...; a workgroup adds its lanes in the fixed
// tree; one thread per image adds the parts in index order -- and are rounded to float32 ONCE.  The layout depends on (h, w) only:
// two calls give the same bits, an image gives the same bits alone and in a batch.  The gradient is a gather, one lane per
// student pixel, its value formed in double and rounded once; no scatter, no atomics.
// Flows at any channel stride >= 2.  Where every flow pointer is on an 8-byte boundary and every channel stride is even a
// pixel's two components are one 8-byte access, else two 4-byte ones: the values fetched, and so every bit, are the same.
#include "loss_common.h"
#include "flow_record.h"

#pragma clang fp contract(fast)   // (flow_record.h turns contraction off behind it; this file's arithmetic is contracted)

struct DistillArgs {
    const float* student;     // [N][h][w] records of s_cs floats, 2 used
    const float* teacher;     // [N][H][W] records of t_cs floats, 2 used
    const uint8_t* tvalid;    // [N][H][W], null: every pixel
    const uint8_t* exclude;   // [N][h][w], null: none
    const float* dsums;       // (grad) [N]
    float* dstudent;          // (grad)
    double* part;             // (sums) [N][parts] doubles, then [N][parts] int32 counts
    int* part_n;
    int s_cs, t_cs, d_cs;
    int N, h, w, H, W, y0, x0;
    double eps2, q;
    int accumulate;
};

// Student pixel (n, y, x): whether it contributes, and then d = student - teacher per component (exact up to one double rounding).
// The window check of the host (0 <= y0, y0 + h <= H, likewise x) is what keeps P inside image n of the teacher.
template <bool VEC>
__device__ __forceinline__ bool distill_pixel(const DistillArgs& a, int n, int y, int x, double d[2]) {
    const size_t p = ((size_t)n * a.h + y) * a.w + x;
    const size_t P = ((size_t)n * a.H + (y + a.y0)) * a.W + (x + a.x0);
    if (a.exclude && a.exclude[p]) return false;
    if (a.tvalid && !a.tvalid[P]) return false;
    float s0, s1, t0, t1;
    pwc_flow_load2<VEC>(a.teacher + P * a.t_cs, t0, t1);
    if (!pwc_flow_known(t0, t1)) return false;
    pwc_flow_load2<VEC>(a.student + p * a.s_cs, s0, s1);
    if (!(fabsf(s0) < __builtin_inff() && fabsf(s1) < __builtin_inff())) return false;   // (false for a NaN)
    d[0] = (double)s0 - (double)t0;
    d[1] = (double)s1 - (double)t1;
    return true;
}

__device__ __forceinline__ double distill_rho(double d, double eps2, double q) { return pow(__builtin_fma(d, d, eps2), q); }
__device__ __forceinline__ double distill_rho_grad(double d, double eps2, double q) {
    return 2.0 * q * d * pow(__builtin_fma(d, d, eps2), q - 1.0);
}

// pwc_block_tree_sum for a double and a count: t += t + k for k = 128, 64 .. 1.  On return thread 0 holds the totals.
__device__ __forceinline__ void distill_tree_sum(double& s, int& c) {
    __shared__ double reds[256];
    __shared__ int redc[256];
    const int t = threadIdx.x;
    reds[t] = s; redc[t] = c;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) {
            reds[t] += reds[t + k];
            redc[t] += redc[t + k];
        }
        __syncthreads();
    }
    s = reds[0]; c = redc[0];
}

// grid (parts, N)
template <bool VEC>
__global__ __launch_bounds__(256) void flow_distill_parts_kernel(const DistillArgs a) {
    const int n = blockIdx.y;
    const int npix = a.h * a.w;
    double sum = 0.0;
    int cnt = 0;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
        const int y = p / a.w, x = p - y * a.w;
        double d[2];
        if (distill_pixel<VEC>(a, n, y, x, d)) {
            sum += distill_rho(d[0], a.eps2, a.q) + distill_rho(d[1], a.eps2, a.q);
            ++cnt;
        }
    }
    distill_tree_sum(sum, cnt);
    if (threadIdx.x == 0) {
        const size_t o = (size_t)n * gridDim.x + blockIdx.x;
        a.part[o] = sum;
        a.part_n[o] = cnt;
    }
}

// One thread per image: the parts in index order, the sum rounded to float32 once, the counts as integers.
__global__ void flow_distill_final_kernel(const double* __restrict__ part, const int* __restrict__ part_n, int nparts, int nimg,
                                          float* __restrict__ sums, int* __restrict__ counts) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nimg) return;
    double s = 0.0;
    int c = 0;
    for (int i = 0; i < nparts; ++i) {
        s += part[(size_t)n * nparts + i];
        c += part_n[(size_t)n * nparts + i];
    }
    sums[n] = (float)s;
    counts[n] = c;
}

// One lane per student pixel of the batch.
template <bool VEC>
__global__ __launch_bounds__(256) void flow_distill_grad_kernel(const DistillArgs a) {
    const long npix = (long)a.N * a.h * a.w;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel px = pwc_loss_pixel(p, a.h, a.w);
        float* o = a.dstudent + p * a.d_cs;
        double d[2];
        if (!distill_pixel<VEC>(a, px.n, px.y, px.x, d)) {
            pwc_grad_skip2(o, a.accumulate);
            continue;
        }
        const double up = (double)a.dsums[px.n];
        const float g0 = (float)(up * distill_rho_grad(d[0], a.eps2, a.q));
        const float g1 = (float)(up * distill_rho_grad(d[1], a.eps2, a.q));
        pwc_grad_store2(o, a.accumulate, 1.f, g0, g1);
    }
}

// ---------------------------------------------------------------- host
extern "C" size_t pwc_flow_distill_workspace_bytes(int N, int h, int w) {
    if (N <= 0 || h <= 0 || w <= 0 || !pwc_loss_in_range(N, h, w)) return 0;
    return (size_t)N * pwc_loss_parts(h, w) * (sizeof(double) + sizeof(int));
}

// The checks both entry points share behind their own null checks, in the order they report.
static int distill_check(const float* student, int s_cs, const float* teacher, int t_cs, int N, int h, int w, int H, int W, int y0,
                         int x0, double eps, double q) {
    if (!student || !teacher || N < 1 || h < 1 || w < 1 || H < 1 || W < 1 || s_cs < 2 || t_cs < 2) return PWC_EINVAL;
    if (y0 < 0 || x0 < 0 || (long)y0 + h > H || (long)x0 + w > W) return PWC_EINVAL;       // the window inside the teacher
    if (!(eps > 0.0) || !(q > 0.0 && q <= 1.0)) return PWC_EINVAL;                          // (a NaN fails both)
    if (!pwc_loss_in_range(N, h, w) || !pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (pwc_off(student, 3u) || pwc_off(teacher, 3u)) return PWC_EALIGN;
    return PWC_OK;
}

static void distill_args(DistillArgs& a, const float* student, int s_cs, const float* teacher, int t_cs, int N, int h, int w, int H,
                         int W, int y0, int x0, const uint8_t* teacher_valid, const uint8_t* exclude, double eps, double q) {
    a.student = student; a.teacher = teacher; a.tvalid = teacher_valid; a.exclude = exclude;
    a.s_cs = s_cs; a.t_cs = t_cs; a.N = N; a.h = h; a.w = w; a.H = H; a.W = W; a.y0 = y0; a.x0 = x0;
    a.eps2 = eps * eps; a.q = q;
}

extern "C" int pwc_flow_distill_sums_f32(const float* student, int s_cs, const float* teacher, int t_cs, int N, int h, int w, int H,
                                         int W, int y0, int x0, const uint8_t* teacher_valid, const uint8_t* exclude, double eps,
                                         double q, float* sums, int32_t* counts, void* workspace, size_t workspace_bytes,
                                         pwc_stream_t stream) {
    const int rc = distill_check(student, s_cs, teacher, t_cs, N, h, w, H, W, y0, x0, eps, q);
    if (rc != PWC_OK) return rc;
    if (!sums || !counts || !workspace) return PWC_EINVAL;
    if (pwc_off(workspace, 7u)) return PWC_EALIGN;
    if (workspace_bytes < pwc_flow_distill_workspace_bytes(N, h, w)) return PWC_EINVAL;
    const int parts = (int)pwc_loss_parts(h, w);
    DistillArgs a = {};
    distill_args(a, student, s_cs, teacher, t_cs, N, h, w, H, W, y0, x0, teacher_valid, exclude, eps, q);
    a.part = reinterpret_cast<double*>(workspace);
    a.part_n = reinterpret_cast<int*>(a.part + (size_t)N * parts);
    const bool vec = pwc_flow_vec(s_cs | t_cs, {student, teacher});
    const dim3 grid((unsigned)parts, (unsigned)N);
    const hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(flow_distill_parts_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(flow_distill_parts_kernel<false>, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(flow_distill_final_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s, a.part, a.part_n, parts, N, sums,
                       (int*)counts);
    return pwc_launch_status();
}

extern "C" int pwc_flow_distill_grad_f32(const float* student, int s_cs, const float* teacher, int t_cs, int N, int h, int w, int H,
                                         int W, int y0, int x0, const uint8_t* teacher_valid, const uint8_t* exclude, double eps,
                                         double q, const float* dsums, float* dstudent, int ds_cs, int accumulate,
                                         pwc_stream_t stream) {
    const int rc = distill_check(student, s_cs, teacher, t_cs, N, h, w, H, W, y0, x0, eps, q);
    if (rc != PWC_OK) return rc;
    if (!dsums || !dstudent || ds_cs < 2) return PWC_EINVAL;
    if (pwc_off(dsums, 3u) || pwc_off(dstudent, 3u)) return PWC_EALIGN;
    DistillArgs a = {};
    distill_args(a, student, s_cs, teacher, t_cs, N, h, w, H, W, y0, x0, teacher_valid, exclude, eps, q);
    a.dsums = dsums; a.dstudent = dstudent; a.d_cs = ds_cs; a.accumulate = accumulate ? 1 : 0;
    const bool vec = pwc_flow_vec(s_cs | t_cs, {student, teacher});
    const dim3 grid = pwc_loss_grad_blocks(N, h, w);
    const hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(flow_distill_grad_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(flow_distill_grad_kernel<false>, grid, dim3(256), 0, s, a);
    return pwc_launch_status();
}
