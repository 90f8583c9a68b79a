// pwc_motion.hip -- dominant motion: the one parametric motion that explains most of a flow field (a robust fit by iteratively
// reweighted least squares, wholly on the device), what the flow has left once that motion is taken out, and frames warped by an
// affine matrix (gfx950; C ABI in include/pwc_hip.h, "dominant motion"; semantics and launch plan in DESIGN.md 20).
//
//   pwc_motion_fit_workspace_bytes   8 (N parts 12 + N 6) + 4 N parts, rounded up to 8: the parts' sums and counts, the parameters
//   pwc_motion_fit_f64               matrices (N, 3, 3) doubles, ok (N) bytes, count (N) int32, weight_sum (N) doubles
//   pwc_motion_residual_f32          residual (N, H, W, 2) floats and inlier (N, H, W) bytes
//   pwc_warp_affine                  out (N, H, W, C) in the frames' dtype and covered (N, H, W) bytes
//   pwc_motion_residual_projective_f32, pwc_warp_projective   the same two with projective.h's position: all nine entries finite,
//                                    a division per pixel, nothing where D is not positive (the PROJ instantiations below)
//
// The fit is iters + 1 passes of two launches each, all on the caller's stream, the device reading what the pass before wrote:
//   sums    grid (parts, N), loss_common.h's partition: part b takes the pixels b 256 + t, + parts 256, ... of its image.  A known
//           pixel -- mask non-zero, both components finite and at most 1e9 in magnitude (flow_io.flow_valid's rule; a masked
//           pixel's flow is not loaded) -- has the normalised coordinates xh = (x - cx) / s, yh = (y - cy) / s, cx = (W - 1) / 2,
//           cy = (H - 1) / 2, s = max(H, W) / 2, the weight w = 1 (pass 0) or 1 / (1 + ((ru ru) + (rv rv)) / (scale scale)) with
//           ru = u - ((a0 + a1 xh) + a2 yh), rv likewise, against the parameters of the pass before, and adds the twelve terms
//           w, w xh, w yh, (w xh) xh, (w xh) yh, (w yh) yh, w u, (w xh) u, (w yh) u, w v, (w xh) v, (w yh) v to its lane's sums
//           and 1 to its count; the 256 lanes add in the fixed tree (pwc_block_tree_sum_f64).
//   solve   a lane per image adds the parts in index order and solves the normal equations by L D L^T elimination without
//           pivoting (motion_ldlt): 3 x 3 with two right-hand sides (affine), the 4 x 4 system in (a0, b0, alpha, beta)
//           (similarity), two quotients (translation).  Degenerate -- too few known pixels, a pivot d that fails d > 1e-9 sum(w),
//           which a NaN fails -- is final: ok = 0, zero parameters and the identity, in that pass and every later one.  The last
//           pass writes the pixel matrices.
// Every value is an IEEE double + - x /, a floor, a rint or a comparison in the order written here -- no fused multiply-add is
// formed anywhere in this file (the pragma below), no library function is called -- so tests/motion_ref.py restates it in numpy
// bit for bit.  No atomic, no host synchronisation, no process-wide state.
// Flows at any channel stride >= 2: where the pointers of a call are on an 8-byte boundary and the stride is even a record's two
// floats are one 8-byte access, else two 4-byte ones -- the values, and so every bit, are the same (flow_record.h).  The pass
// structure, the parts and the workspace are robust_fit.h's.
#include "motion_ldlt.h"
#include "projective.h"
#include "robust_fit.h"

#pragma clang fp contract(off)

#define MOTION_PIVOT 1e-9

// ---------------------------------------------------------------- the fit
struct MotionFitArgs {
    const float* flow;        // [N][H][W] records of cs floats, 2 used
    const uint8_t* valid;     // [N][H][W], null: every pixel
    double* part;             // [N][parts][12]
    double* param;            // [N][6]: a0 a1 a2 b0 b1 b2
    int* part_n;              // [N][parts]
    double* matrices;         // [N][9]
    uint8_t* ok;              // [N]
    int* count;               // [N]
    double* weight_sum;       // [N]
    double scale;
    int cs, N, H, W, parts, model;
    int first, last;          // pass 0: w = 1; the last pass writes the matrices
};

template <bool VEC>
__global__ __launch_bounds__(256) void motion_sums_kernel(const MotionFitArgs a) {
    const int n = blockIdx.y, hw = a.H * a.W;
    const size_t img = (size_t)n * hw;
    const PwcFitNorm t = pwc_fit_norm(a.H, a.W);
    const double c2 = a.scale * a.scale;
    double p[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!a.first) {
#pragma unroll
        for (int j = 0; j < 6; ++j) p[j] = a.param[(size_t)n * 6 + j];
    }
    double sum[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) sum[j] = 0.0;
    int cnt = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += (int)gridDim.x * 256) {
        if (a.valid && !a.valid[img + i]) continue;
        float fu, fv;
        pwc_flow_load2<VEC>(a.flow + (img + i) * a.cs, fu, fv);
        if (!pwc_flow_known(fu, fv)) continue;
        const double u = (double)fu, v = (double)fv;
        double xh, yh;
        pwc_fit_normalise(t, i, a.W, xh, yh);
        double w = 1.0;
        if (!a.first) {
            const double ru = u - ((p[0] + (p[1] * xh)) + (p[2] * yh)), rv = v - ((p[3] + (p[4] * xh)) + (p[5] * yh));
            w = 1.0 / (1.0 + (((ru * ru) + (rv * rv)) / c2));
        }
        const double wx = w * xh, wy = w * yh;
        sum[0] = sum[0] + w;         sum[1] = sum[1] + wx;        sum[2] = sum[2] + wy;
        sum[3] = sum[3] + (wx * xh); sum[4] = sum[4] + (wx * yh); sum[5] = sum[5] + (wy * yh);
        sum[6] = sum[6] + (w * u);   sum[7] = sum[7] + (wx * u);  sum[8] = sum[8] + (wy * u);
        sum[9] = sum[9] + (w * v);   sum[10] = sum[10] + (wx * v); sum[11] = sum[11] + (wy * v);
        cnt += 1;
    }
    pwc_fit_write_part<12>(sum, cnt, n, a.part, a.part_n);
}

// (motion_ldlt: motion_ldlt.h, shared with pwc_homography.hip.)
// One lane per image.
__global__ __launch_bounds__(64) void motion_solve_kernel(const MotionFitArgs a) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= a.N) return;
    double S[12];
    int cnt;
    pwc_fit_gather<12>(a.part, a.part_n, n, a.parts, S, cnt);
    const double tol = MOTION_PIVOT * S[0];
    double p[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool good = a.first || a.ok[n] != 0;
    if (a.model == PWC_MOTION_TRANSLATION) {
        good = good && cnt >= 1 && S[0] > tol;
        if (good) { p[0] = S[6] / S[0]; p[3] = S[9] / S[0]; }
    } else if (a.model == PWC_MOTION_SIMILARITY) {
        good = good && cnt >= 2;
        if (good) {
            const double q = S[3] + S[5];
            const double A[4][4] = {{S[0], 0.0, 0.0, 0.0}, {0.0, S[0], 0.0, 0.0}, {S[1], S[2], q, 0.0}, {-S[2], S[1], 0.0, q}};
            double r[1][4] = {{S[6], S[9], S[7] + S[11], S[10] - S[8]}};
            good = motion_ldlt<4, 1>(A, r, tol);
            if (good) { p[0] = r[0][0]; p[1] = r[0][2]; p[2] = -r[0][3]; p[3] = r[0][1]; p[4] = r[0][3]; p[5] = r[0][2]; }
        }
    } else {
        good = good && cnt >= 3;
        if (good) {
            const double A[3][3] = {{S[0], 0.0, 0.0}, {S[1], S[3], 0.0}, {S[2], S[4], S[5]}};
            double r[2][3] = {{S[6], S[7], S[8]}, {S[9], S[10], S[11]}};
            good = motion_ldlt<3, 2>(A, r, tol);
            if (good) { p[0] = r[0][0]; p[1] = r[0][1]; p[2] = r[0][2]; p[3] = r[1][0]; p[4] = r[1][1]; p[5] = r[1][2]; }
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) a.param[(size_t)n * 6 + j] = p[j];
    a.ok[n] = good ? 1 : 0;
    a.count[n] = cnt;
    a.weight_sum[n] = S[0];
    if (a.last) {
        // the identity plus (A T) row by row, A = [[p1 p2 p0] [p4 p5 p3]]
        double* m = a.matrices + (size_t)n * 9;
        double r[2][3];
        pwc_fit_row_times_t(pwc_fit_norm(a.H, a.W), p[1], p[2], p[0], r[0][0], r[0][1], r[0][2]);
        pwc_fit_row_times_t(pwc_fit_norm(a.H, a.W), p[4], p[5], p[3], r[1][0], r[1][1], r[1][2]);
        m[0] = 1.0 + r[0][0]; m[1] = r[0][1];       m[2] = r[0][2];
        m[3] = r[1][0];       m[4] = 1.0 + r[1][1]; m[5] = r[1][2];
        m[6] = 0.0; m[7] = 0.0; m[8] = 1.0;
    }
}

// ---------------------------------------------------------------- the residual
struct MotionResidualArgs {
    const float* flow;        // [N][H][W] records of cs floats
    const uint8_t* valid;     // [N][H][W], null: every pixel
    const double* matrices;   // [N][9]
    float* residual;          // [N][H][W][2]
    uint8_t* inlier;          // [N][H][W]
    double thr2;
    int cs, N, H, W;
};

// The six entries of an image's matrix; false where its last row is not exactly 0 0 1 or an entry is not finite.
__device__ __forceinline__ bool motion_affine(const double* m, double* e) {
    bool good = m[6] == 0.0 && m[7] == 0.0 && m[8] == 1.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) { e[j] = m[j]; good = good && pwc_finite(e[j]); }
    return good;
}

// One lane per pixel of the batch.  PROJ: the matrices are projective (projective.h's rule) -- all nine entries finite, the
// position with the division, no residual where there is no position.
template <bool VEC, bool PROJ>
__global__ __launch_bounds__(256) void motion_residual_kernel(const MotionResidualArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    for (long g = blockIdx.x * 256L + threadIdx.x; g < npix; g += (long)gridDim.x * 256) {
        const PwcLossPixel q = pwc_loss_pixel(g, a.H, a.W);
        float r0 = PWC_FLOW_SENTINEL, r1 = PWC_FLOW_SENTINEL;
        uint8_t in = 0;
        double m[PROJ ? 9 : 6];
        const bool good = PROJ ? pwc_projective_finite(a.matrices + (size_t)q.n * 9, m) : motion_affine(a.matrices + (size_t)q.n * 9, m);
        if (good && !(a.valid && !a.valid[g])) {
            float fu, fv;
            pwc_flow_load2<VEC>(a.flow + (size_t)g * a.cs, fu, fv);
            if (pwc_flow_known(fu, fv)) {
                const double x = (double)q.x, y = (double)q.y;
                double sx, sy;
                bool there = true;
                if (PROJ) {
                    there = pwc_projective_position(m, x, y, sx, sy);
                } else {
                    sx = ((m[0] * x) + (m[1] * y)) + m[2]; sy = ((m[3] * x) + (m[4] * y)) + m[5];
                }
                if (there) {
                    const double mu = sx - x, mv = sy - y;
                    const double ru = (double)fu - mu, rv = (double)fv - mv;
                    r0 = (float)ru; r1 = (float)rv;
                    in = ((ru * ru) + (rv * rv)) <= a.thr2 ? 1 : 0;
                }
            }
        }
        pwc_flow_store2<VEC>(a.residual + 2 * g, r0, r1);
        a.inlier[g] = in;
    }
}

// ---------------------------------------------------------------- the warp
struct MotionWarpArgs {
    const void* frames;       // [N][H][W][C] bytes or floats, dense
    const double* matrices;   // [N][9]: an OUTPUT pixel to its source position
    void* out;                // [N][H][W][C]
    uint8_t* covered;         // [N][H][W]
    int N, H, W;
    int out_vec, covered_vec; // out on a 4-byte (bytes) / 16-byte (floats) boundary, covered on a 4-byte one
};

// Output pixel g: its C channels as doubles (pwc_fb_valid_u8's sample of the source position); false where it is not covered.
// PROJ: projective.h's rule in place of the affine one.
template <bool U8, int C, bool PROJ>
__device__ __forceinline__ bool motion_warp_pixel(const MotionWarpArgs& a, long g, double* v) {
    const PwcLossPixel q = pwc_loss_pixel(g, a.H, a.W);
    double m[PROJ ? 9 : 6];
    if (!(PROJ ? pwc_projective_finite(a.matrices + (size_t)q.n * 9, m) : motion_affine(a.matrices + (size_t)q.n * 9, m))) return false;
    const double x = (double)q.x, y = (double)q.y;
    double sx, sy;
    if (PROJ) {
        if (!pwc_projective_position(m, x, y, sx, sy)) return false;
    } else {
        sx = ((m[0] * x) + (m[1] * y)) + m[2]; sy = ((m[3] * x) + (m[4] * y)) + m[5];
    }
    // (every comparison is false for a NaN; an Inf fails one of them) -- what keeps the four corner reads inside image n
    if (!(sx >= 0.0 && sx <= (double)(a.W - 1) && sy >= 0.0 && sy <= (double)(a.H - 1))) return false;
    const PwcBilinearF64 bl = pwc_bilinear_f64(sx, sy, a.H, a.W);
    const double wx0 = bl.wx0, wx1 = bl.wx1, wy0 = bl.wy0, wy1 = bl.wy1;
    const size_t img = (size_t)q.n * a.H * a.W;
    const size_t o00 = (img + bl.o00) * C, o01 = (img + bl.o01) * C;
    const size_t o10 = (img + bl.o10) * C, o11 = (img + bl.o11) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        double c00, c01, c10, c11;
        if (U8) {
            const uint8_t* f = reinterpret_cast<const uint8_t*>(a.frames);
            c00 = (double)f[o00 + c]; c01 = (double)f[o01 + c]; c10 = (double)f[o10 + c]; c11 = (double)f[o11 + c];
        } else {
            const float* f = reinterpret_cast<const float*>(a.frames);
            c00 = (double)f[o00 + c]; c01 = (double)f[o01 + c]; c10 = (double)f[o10 + c]; c11 = (double)f[o11 + c];
        }
        const double top = (wx0 * c00) + (wx1 * c01), bot = (wx0 * c10) + (wx1 * c11);
        v[c] = (wy0 * top) + (wy1 * bot);
    }
    return true;
}

// One lane per run of four output pixels of the flat (N, H, W) index: 4 C bytes (C dwords) or 4 C floats (C 16-byte stores).
template <bool U8, int C, bool PROJ>
__global__ __launch_bounds__(256) void motion_warp_kernel(const MotionWarpArgs a) {
    const long total = (long)a.N * a.H * a.W;
    const long runs = (total + 3) / 4;
    for (long r = blockIdx.x * 256L + threadIdx.x; r < runs; r += (long)gridDim.x * 256) {
        const long g0 = 4 * r;
        const bool whole = g0 + 4 <= total;
        unsigned cov = 0u, b[4 * C];
        float f[4 * C];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double v[C];
            const bool ok = g0 + i < total && motion_warp_pixel<U8, C, PROJ>(a, g0 + i, v);
            cov |= (ok ? 1u : 0u) << (8 * i);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (U8) b[C * i + c] = ok ? pwc_round_byte(v[c]) : 0u;
                else f[C * i + c] = ok ? (float)v[c] : 0.f;
            }
        }
        if (a.covered_vec && whole) {
            *reinterpret_cast<unsigned*>(a.covered + g0) = cov;
        } else {
            for (int i = 0; i < 4 && g0 + i < total; ++i) a.covered[g0 + i] = (uint8_t)((cov >> (8 * i)) & 255u);
        }
        if (U8) {
            uint8_t* o = reinterpret_cast<uint8_t*>(a.out) + C * g0;
            if (a.out_vec && whole) {
                unsigned* d = reinterpret_cast<unsigned*>(o);
#pragma unroll
                for (int j = 0; j < C; ++j) d[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4 * C; ++j)
                    if (g0 + j / C < total) o[j] = (uint8_t)b[j];
            }
        } else {
            float* o = reinterpret_cast<float*>(a.out) + C * g0;
            if (a.out_vec && whole) {
                f32x4* d = reinterpret_cast<f32x4*>(o);
#pragma unroll
                for (int j = 0; j < C; ++j) d[j] = f32x4{f[4 * j], f[4 * j + 1], f[4 * j + 2], f[4 * j + 3]};
            } else {
#pragma unroll
                for (int j = 0; j < 4 * C; ++j)
                    if (g0 + j / C < total) o[j] = f[j];
            }
        }
    }
}

// ---------------------------------------------------------------- host
extern "C" size_t pwc_motion_fit_workspace_bytes(int N, int H, int W) { return pwc_fit_workspace_bytes(N, H, W, 12, 6); }

extern "C" int pwc_motion_fit_f64(const float* flows, int flow_cs, const uint8_t* valid, int N, int H, int W, int model, int iters,
                                  double scale, void* workspace, size_t workspace_bytes, double* matrices, uint8_t* ok,
                                  int32_t* count, double* weight_sum, pwc_stream_t stream) {
    if (!matrices || !ok || !count || !weight_sum) return PWC_EINVAL;
    if (model != PWC_MOTION_TRANSLATION && model != PWC_MOTION_SIMILARITY && model != PWC_MOTION_AFFINE) return PWC_EINVAL;
    const int rc = pwc_fit_check(flows, flow_cs, N, H, W, iters, scale, workspace, workspace_bytes, pwc_motion_fit_workspace_bytes(N, H, W),
                                 pwc_off(matrices, 7u) || pwc_off(weight_sum, 7u) || pwc_off(count, 3u));
    if (rc != PWC_OK) return rc;
    const int parts = (int)pwc_loss_parts(H, W);
    MotionFitArgs a = {};
    a.flow = flows; a.valid = valid;
    pwc_fit_carve(workspace, N, parts, 12, 6, a.part, a.param, a.part_n);
    a.matrices = matrices; a.ok = ok; a.count = count; a.weight_sum = weight_sum;
    a.scale = scale; a.cs = flow_cs; a.N = N; a.H = H; a.W = W; a.parts = parts; a.model = model;
    pwc_fit_passes<motion_sums_kernel<true>, motion_sums_kernel<false>, motion_solve_kernel>(a, iters, pwc_flow_vec(flow_cs, {flows}),
                                                                                            (hipStream_t)stream);
    return pwc_launch_status();
}

static int motion_residual_call(const float* flows, int flow_cs, const uint8_t* valid, const double* matrices, int N, int H, int W,
                                double threshold, float* residual, uint8_t* inlier, bool projective, pwc_stream_t stream) {
    if (!flows || !matrices || !residual || !inlier) return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || flow_cs < 2 || !(threshold >= 0.0)) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (pwc_off(flows, 3u) || pwc_off(residual, 3u) || pwc_off(matrices, 7u)) return PWC_EALIGN;
    MotionResidualArgs a = {};
    a.flow = flows; a.valid = valid; a.matrices = matrices; a.residual = residual; a.inlier = inlier;
    a.thr2 = threshold * threshold; a.cs = flow_cs; a.N = N; a.H = H; a.W = W;
    const bool vec = pwc_flow_vec(flow_cs, {flows, residual});
    const dim3 grid = pwc_loss_grad_blocks(N, H, W);
    const hipStream_t s = (hipStream_t)stream;
    if (projective) {
        if (vec) hipLaunchKernelGGL((motion_residual_kernel<true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((motion_residual_kernel<false, true>), grid, dim3(256), 0, s, a);
    } else {
        if (vec) hipLaunchKernelGGL((motion_residual_kernel<true, false>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((motion_residual_kernel<false, false>), grid, dim3(256), 0, s, a);
    }
    return pwc_launch_status();
}

extern "C" int pwc_motion_residual_f32(const float* flows, int flow_cs, const uint8_t* valid, const double* matrices, int N, int H,
                                       int W, double threshold, float* residual, uint8_t* inlier, pwc_stream_t stream) {
    return motion_residual_call(flows, flow_cs, valid, matrices, N, H, W, threshold, residual, inlier, false, stream);
}

extern "C" int pwc_motion_residual_projective_f32(const float* flows, int flow_cs, const uint8_t* valid, const double* matrices, int N,
                                                  int H, int W, double threshold, float* residual, uint8_t* inlier,
                                                  pwc_stream_t stream) {
    return motion_residual_call(flows, flow_cs, valid, matrices, N, H, W, threshold, residual, inlier, true, stream);
}

template <bool U8, bool PROJ>
static void motion_warp_launch(int C, dim3 grid, hipStream_t s, const MotionWarpArgs& a) {
    if (C == 1) hipLaunchKernelGGL((motion_warp_kernel<U8, 1, PROJ>), grid, dim3(256), 0, s, a);
    else if (C == 2) hipLaunchKernelGGL((motion_warp_kernel<U8, 2, PROJ>), grid, dim3(256), 0, s, a);
    else if (C == 3) hipLaunchKernelGGL((motion_warp_kernel<U8, 3, PROJ>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((motion_warp_kernel<U8, 4, PROJ>), grid, dim3(256), 0, s, a);
}

static int motion_warp_call(const void* frames, int dtype, int C, const double* matrices, int N, int H, int W, void* out,
                            uint8_t* covered, bool projective, pwc_stream_t stream) {
    if (!frames || !matrices || !out || !covered) return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || C < 1 || C > 4 || (dtype != PWC_MOTION_U8 && dtype != PWC_MOTION_F32)) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    const bool u8 = dtype == PWC_MOTION_U8;
    if (pwc_off(matrices, 7u) || (!u8 && (pwc_off(frames, 3u) || pwc_off(out, 3u)))) return PWC_EALIGN;
    MotionWarpArgs a = {};
    a.frames = frames; a.matrices = matrices; a.out = out; a.covered = covered; a.N = N; a.H = H; a.W = W;
    a.out_vec = pwc_off(out, u8 ? 3u : 15u) ? 0 : 1;
    a.covered_vec = pwc_off(covered, 3u) ? 0 : 1;
    const dim3 grid = pwc_flat_grid(((long)N * H * W + 3) / 4);
    if (projective) {
        if (u8) motion_warp_launch<true, true>(C, grid, (hipStream_t)stream, a);
        else motion_warp_launch<false, true>(C, grid, (hipStream_t)stream, a);
    } else {
        if (u8) motion_warp_launch<true, false>(C, grid, (hipStream_t)stream, a);
        else motion_warp_launch<false, false>(C, grid, (hipStream_t)stream, a);
    }
    return pwc_launch_status();
}

extern "C" int pwc_warp_affine(const void* frames, int dtype, int C, const double* matrices, int N, int H, int W, void* out,
                               uint8_t* covered, pwc_stream_t stream) {
    return motion_warp_call(frames, dtype, C, matrices, N, H, W, out, covered, false, stream);
}

extern "C" int pwc_warp_projective(const void* frames, int dtype, int C, const double* matrices, int N, int H, int W, void* out,
                                   uint8_t* covered, pwc_stream_t stream) {
    return motion_warp_call(frames, dtype, C, matrices, N, H, W, out, covered, true, stream);
}
