// pwc_ssim.hip -- the SSIM photometric term of label-free training (the data term of UFlow / ARFlow): per-image sums and their
// gradient with respect to the flow (gfx950; C ABI in include/pwc_hip.h, "self-supervised losses").
//
//   pwc_ssim_sums_f32   per-image sums of (1 - SSIM) / 2 over the contributing centres and the channels, and their number
//   pwc_ssim_grad_f32   the gradient of those sums w.r.t. the flow, times an upstream gradient per image
//
// x(p, c) = images_0[p, c]; y(p, c) = the photometric term's bilinear sample of images_1 at p moved by flow_scale * flow[p]
// (in-frame rule 0 <= px <= W - 1, 0 <= py <= H - 1, a non-finite flow is out of frame; floor, clipped corners and weights are
// pwc_unsup.hip's photo_pixel's; sample point, weights and blend in double, rounded to fp32 once).  Per channel, over the
// n = (2r+1)^2 pixels of the window of centre p, in double from the fp32 x and y, in the CENTRED form (no negative variance):
//   mu_x = mean x, mu_y = mean y, s_x = mean (x - mu_x)^2, s_y = mean (y - mu_y)^2, s_xy = mean (x - mu_x)(y - mu_y),
//   A1 = 2 mu_x mu_y + c1, A2 = 2 s_xy + c2, B1 = mu_x^2 + mu_y^2 + c1, B2 = s_x + s_y + c2,
//   SSIM = A1 A2 / (B1 B2),  term(p, c) = (1 - SSIM) / 2          (no clamp, no rho).
// A centre p CONTRIBUTES iff it is at least r from every border (no padding), valid is null or valid[p] != 0, and the sample
// point of EVERY pixel of its window is in frame: a zero inside a window would wreck its means and variances, so an out-of-frame
// pixel switches off every window it belongs to (unlike pwc_census.hip, where a neighbour is always read).  `valid` selects
// centres only.  H <= 2r or W <= 2r: nothing contributes, sums, counts and gradient are 0.
//
// Three passes, every one deterministic:
//   prepare   one lane per pixel: the C planes of y, the in-frame byte and (gradient) the C planes of the sample's derivatives
//             along x and y into the workspace.
//   window    a workgroup owns 32 x 8 tiles of centres, one lane per centre; it stages the tile and an r-pixel halo of x, y and
//             the in-frame flag in the LDS ((32+2r) x (8+2r) cells per plane, at most 9 planes; a cell outside the image holds the
//             flag 0), so that the n window pixels cost LDS reads.  The sums kernel adds its tiles' terms -- part b of at most 256
//             takes the tiles b, b + parts, ... -- in loss_common.h's tree, one thread per image adds the parts in index order.
//             The gradient's kernel writes three coefficients per centre and channel instead:
//               dSSIM/dy_q = (1/n) [2 mu_x A2 / (B1 B2) + 2 (x_q - mu_x) A1 / (B1 B2) - 2 S mu_y / B1 - 2 S (y_q - mu_y) / B2]
//                          = alpha_p + beta_p x_q + gamma_p y_q            for q in the window of p,
//             times -dsums[n] / 2, and 0 where p does not contribute.  They are kept as DOUBLES: beta and gamma are of the
//             size 1 / (n B2), up to ~1e3 / n where c2 dominates the variances, and alpha + beta x_q + gamma y_q cancels down to
//             beta (x_q - mu_x) + ...; fp32 planes would put ulp(alpha) of every centre into the gradient.
//   gather    same tiling, one channel at a time: the three coefficient planes staged (0 outside the image), box sums over the
//             centres within r of q, dL/dy_c(q) = sum alpha + x_q sum beta + y_q sum gamma, and, where q is in frame,
//             dflow(q) = flow_scale * sum_c dL/dy_c(q) * (dy_c/dx, dy_c/dy), formed in double and rounded once.  A q that is out
//             of frame or has no contributing centre within r gets 0 (accumulate: is left alone).  No atomics.
#include "loss_common.h"

constexpr int SSIM_TW = 32, SSIM_TH = 8;          // centres of a tile: one per lane of the 256
constexpr int SSIM_MAXC = 4;

struct SsimArgs {
    const float* im0;
    const float* im1;
    const float* flow;
    const uint8_t* valid;    // [N][H][W], null: every pixel
    const float* dsums;      // [N] upstream gradient (grad)
    float* dflow;            // 2 channels, written or accumulated (grad)
    float* py;               // workspace planes [C][N][H][W]: y
    float* pgx;              // d y / d x, d y / d y (grad)
    float* pgy;
    double* pcoef;           // [C][3][N][H][W]: alpha, beta, gamma times -dsums[n] / 2 (grad)
    uint8_t* inframe;        // [N][H][W]
    float* partial;          // [N][gridDim.x] sums
    int* partial_n;          // [N][gridDim.x] counts of contributing centres
    int im0_cs, im1_cs, flow_cs, dflow_cs;
    int N, H, W, C;
    float flow_scale;
    double c1, c2;
    int accumulate;
};

// ------------------------------------------------------------------ prepare
template <int C, bool GRAD>
__global__ __launch_bounds__(256) void ssim_prepare_kernel(const SsimArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel px = pwc_loss_pixel(p, a.H, a.W);
        const float* fp = a.flow + p * a.flow_cs;
        const double sx = (double)px.x + (double)fp[0] * (double)a.flow_scale, sy = (double)px.y + (double)fp[1] * (double)a.flow_scale;
        float yv[C], gx[C], gy[C];
#pragma unroll
        for (int c = 0; c < C; ++c) yv[c] = gx[c] = gy[c] = 0.f;
        // (every comparison is false for a NaN; an Inf fails one of them.)  The test keeps the four corner reads inside image n.
        const bool in = sx >= 0.0 && sx <= (double)(a.W - 1) && sy >= 0.0 && sy <= (double)(a.H - 1);
        if (in) {
            const PwcBilinearF64 bl = pwc_bilinear_f64(sx, sy, a.H, a.W);
            const double wx0 = bl.wx0, wx1 = bl.wx1, wy0 = bl.wy0, wy1 = bl.wy1;
            const size_t img = (size_t)px.n * a.H * a.W;
            const float* p00 = a.im1 + (img + bl.o00) * a.im1_cs;
            const float* p01 = a.im1 + (img + bl.o01) * a.im1_cs;
            const float* p10 = a.im1 + (img + bl.o10) * a.im1_cs;
            const float* p11 = a.im1 + (img + bl.o11) * a.im1_cs;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double v00 = p00[c], v01 = p01[c], v10 = p10[c], v11 = p11[c];
                yv[c] = (float)(wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11));
                if (GRAD) {
                    gx[c] = (float)(wy0 * (v01 - v00) + wy1 * (v11 - v10));
                    gy[c] = (float)(wx0 * (v10 - v00) + wx1 * (v11 - v01));
                }
            }
        }
        a.inframe[p] = in ? 1 : 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            a.py[(size_t)c * npix + p] = yv[c];
            if (GRAD) {
                a.pgx[(size_t)c * npix + p] = gx[c];
                a.pgy[(size_t)c * npix + p] = gy[c];
            }
        }
    }
}

// ------------------------------------------------------------------ window
template <int R>
struct SsimTile {
    static constexpr int LW = SSIM_TW + 2 * R, LH = SSIM_TH + 2 * R, CELLS = LW * LH, NWIN = (2 * R + 1) * (2 * R + 1);
};

// The window statistics of the centre in LDS cell c, from one channel's planes of x and y.
struct SsimStats {
    double mux, muy, A1, A2, B1, B2, S;
};
template <int R>
__device__ __forceinline__ SsimStats ssim_stats(const float* lx, const float* ly, int c, double c1, double c2) {
    using T = SsimTile<R>;
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            const int o = c + dy * T::LW + dx;
            sx += (double)lx[o];
            sy += (double)ly[o];
        }
    }
    SsimStats s;
    s.mux = sx / (double)T::NWIN;
    s.muy = sy / (double)T::NWIN;
    double vx = 0.0, vy = 0.0, vxy = 0.0;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            const int o = c + dy * T::LW + dx;
            const double ex = (double)lx[o] - s.mux, ey = (double)ly[o] - s.muy;
            vx += ex * ex;
            vy += ey * ey;
            vxy += ex * ey;
        }
    }
    s.A1 = 2.0 * s.mux * s.muy + c1;
    s.A2 = 2.0 * (vxy / (double)T::NWIN) + c2;
    s.B1 = s.mux * s.mux + s.muy * s.muy + c1;
    s.B2 = vx / (double)T::NWIN + vy / (double)T::NWIN + c2;
    s.S = s.A1 * s.A2 / (s.B1 * s.B2);
    return s;
}

// SUMS: this workgroup's part of image blockIdx.y's sum and count.  Otherwise: the coefficient planes.
template <int R, bool SUMS>
__global__ __launch_bounds__(256) void ssim_window_kernel(const SsimArgs a) {
    using T = SsimTile<R>;
    __shared__ float lx[SSIM_MAXC][T::CELLS];
    __shared__ float ly[SSIM_MAXC][T::CELLS];
    __shared__ uint8_t lf[T::CELLS];
    const int n = blockIdx.y;
    const size_t P = (size_t)a.N * a.H * a.W;
    const int tiles_x = (a.W + SSIM_TW - 1) / SSIM_TW, tiles = tiles_x * ((a.H + SSIM_TH - 1) / SSIM_TH);
    const int ty = threadIdx.x / SSIM_TW, tx = threadIdx.x % SSIM_TW;
    const int cell = (ty + R) * T::LW + tx + R;
    float s = 0.f;
    int cnt = 0;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty0 = (tile / tiles_x) * SSIM_TH, tx0 = (tile % tiles_x) * SSIM_TW;
        // the tile and its halo; a cell outside the image: flag 0 (it belongs to no interior centre's window).  Barriers: the
        // readers of the previous tile are done before, the cells are published after.
        __syncthreads();
        for (int i = threadIdx.x; i < T::CELLS; i += 256) {
            const int cy = i / T::LW, cx = i - cy * T::LW;
            const int gy = ty0 - R + cy, gx = tx0 - R + cx;
            const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            const size_t g = in ? ((size_t)n * a.H + gy) * a.W + gx : 0;
            lf[i] = in ? a.inframe[g] : 0;
            for (int c = 0; c < a.C; ++c) {
                lx[c][i] = in ? a.im0[g * a.im0_cs + c] : 0.f;
                ly[c][i] = in ? a.py[(size_t)c * P + g] : 0.f;
            }
        }
        __syncthreads();
        const int y = ty0 + ty, x = tx0 + tx;
        if (y < a.H && x < a.W) {
            const size_t p = ((size_t)n * a.H + y) * a.W + x;
            bool contributes = y >= R && y < a.H - R && x >= R && x < a.W - R && (!a.valid || a.valid[p]);
            if (contributes) {
                int f = 0;
#pragma unroll
                for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
                    for (int dx = -R; dx <= R; ++dx) f += lf[cell + dy * T::LW + dx];
                }
                contributes = f == T::NWIN;
            }
            if (SUMS) {
                if (contributes) {
                    double t = 0.0;
                    for (int c = 0; c < a.C; ++c) t += 0.5 * (1.0 - ssim_stats<R>(lx[c], ly[c], cell, a.c1, a.c2).S);
                    s += (float)t;
                    ++cnt;
                }
            } else {
                const double u = contributes ? -0.5 * (double)a.dsums[n] / (double)T::NWIN : 0.0;
                for (int c = 0; c < a.C; ++c) {
                    double al = 0.0, be = 0.0, ga = 0.0;
                    if (contributes) {
                        const SsimStats st = ssim_stats<R>(lx[c], ly[c], cell, a.c1, a.c2);
                        be = u * 2.0 * st.A1 / (st.B1 * st.B2);
                        ga = -u * 2.0 * st.S / st.B2;
                        al = u * (2.0 * st.mux * st.A2 / (st.B1 * st.B2) - 2.0 * st.S * st.muy / st.B1) - be * st.mux - ga * st.muy;
                    }
                    double* o = a.pcoef + (size_t)c * 3 * P + p;
                    o[0] = al;
                    o[P] = be;
                    o[2 * P] = ga;
                }
            }
        }
    }
    if (SUMS) pwc_loss_write_part<true>(s, cnt, a.partial, a.partial_n);
}

// ------------------------------------------------------------------ gather
template <int R>
__global__ __launch_bounds__(256) void ssim_grad_kernel(const SsimArgs a) {
    using T = SsimTile<R>;
    __shared__ double lds[3][T::CELLS];
    const int n = blockIdx.y;
    const size_t P = (size_t)a.N * a.H * a.W;
    const int tiles_x = (a.W + SSIM_TW - 1) / SSIM_TW, tiles = tiles_x * ((a.H + SSIM_TH - 1) / SSIM_TH);
    const int ty = threadIdx.x / SSIM_TW, tx = threadIdx.x % SSIM_TW;
    const int cell = (ty + R) * T::LW + tx + R;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty0 = (tile / tiles_x) * SSIM_TH, tx0 = (tile % tiles_x) * SSIM_TW;
        const int y = ty0 + ty, x = tx0 + tx;
        const bool active = y < a.H && x < a.W;
        const size_t p = active ? ((size_t)n * a.H + y) * a.W + x : 0;
        const bool in = active && a.inframe[p];
        double dx = 0.0, dy = 0.0;
        bool any = false;
        for (int c = 0; c < a.C; ++c) {
            const double* coef = a.pcoef + (size_t)c * 3 * P;
            __syncthreads();
            for (int i = threadIdx.x; i < T::CELLS; i += 256) {
                const int cy = i / T::LW, cx = i - cy * T::LW;
                const int gy = ty0 - R + cy, gx = tx0 - R + cx;
                const bool inside = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
                const size_t g = inside ? ((size_t)n * a.H + gy) * a.W + gx : 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) lds[k][i] = inside ? coef[(size_t)k * P + g] : 0.0;
            }
            __syncthreads();
            if (in) {
                double sa = 0.0, sb = 0.0, sg = 0.0;
#pragma unroll
                for (int wy = -R; wy <= R; ++wy) {
#pragma unroll
                    for (int wx = -R; wx <= R; ++wx) {
                        const int o = cell + wy * T::LW + wx;
                        sa += lds[0][o];
                        sb += lds[1][o];
                        sg += lds[2][o];
                    }
                }
                if (sa != 0.0 || sb != 0.0 || sg != 0.0) {       // (no contributing centre within r: every cell is exactly 0)
                    any = true;
                    const double dLdy = sa + (double)a.im0[p * a.im0_cs + c] * sb + (double)a.py[(size_t)c * P + p] * sg;
                    dx += dLdy * (double)a.pgx[(size_t)c * P + p];
                    dy += dLdy * (double)a.pgy[(size_t)c * P + p];
                }
            }
        }
        if (active) {
            float* o = a.dflow + p * a.dflow_cs;
            if (!any)
                pwc_grad_skip2(o, a.accumulate);
            else        // (rounded on their own: accumulate adds exactly what a plain call writes)
                pwc_grad_store2(o, a.accumulate, 1.f, (float)((double)a.flow_scale * dx), (float)((double)a.flow_scale * dy));
        }
    }
}

// ------------------------------------------------------------------ host
// The tiles of an image are cut into at most 256 parts: part b takes the tiles b, b + parts, ...
static inline long ssim_parts(int H, int W) {
    const long tiles = (((long)W + SSIM_TW - 1) / SSIM_TW) * (((long)H + SSIM_TH - 1) / SSIM_TH);
    return tiles > 256 ? 256 : tiles;
}

// workspace: [2][N][parts] sums and counts, the C planes of y (with_grad: and 2 C of its derivatives), the in-frame bytes,
// (with_grad) one float of slack to align, and the 3 C coefficient planes of doubles
extern "C" size_t pwc_ssim_workspace_floats(int N, int H, int W, int C, int with_grad) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    const size_t P = (size_t)N * H * W;
    return 2 * (size_t)N * ssim_parts(H, W) + (with_grad ? 9 : 1) * (size_t)C * P + (P + 3) / 4 + (with_grad ? 1 : 0);
}

static int ssim_check(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs, int N, int H,
                      int W, int C, int radius, float c1, float c2, const float* workspace, size_t workspace_floats,
                      int with_grad) {
    if (!im0 || !im1 || !flow || N <= 0 || H <= 0 || W <= 0) return PWC_EINVAL;
    if (C < 1 || C > SSIM_MAXC || radius < 1 || radius > 3) return PWC_EUNSUPPORTED;
    if (im0_cs < C || im1_cs < C || flow_cs < 2) return PWC_EINVAL;
    if (!(c1 > 0.f) || !(c2 > 0.f)) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (!workspace || workspace_floats < pwc_ssim_workspace_floats(N, H, W, C, with_grad)) return PWC_EINVAL;
    return PWC_OK;
}

static SsimArgs ssim_args(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                          float flow_scale, const uint8_t* valid, int N, int H, int W, int C, float c1, float c2, float* workspace,
                          int with_grad) {
    const size_t P = (size_t)N * H * W;
    SsimArgs a;
    a.im0 = im0; a.im1 = im1; a.flow = flow; a.valid = valid; a.dsums = nullptr; a.dflow = nullptr;
    a.partial = workspace; a.partial_n = reinterpret_cast<int*>(workspace + (size_t)N * ssim_parts(H, W));
    float* planes = workspace + 2 * (size_t)N * ssim_parts(H, W);
    a.py = planes;
    a.pgx = with_grad ? planes + (size_t)C * P : nullptr; a.pgy = with_grad ? planes + 2 * (size_t)C * P : nullptr;
    float* bytes = planes + (with_grad ? 3 : 1) * (size_t)C * P;
    a.inframe = reinterpret_cast<uint8_t*>(bytes);
    a.pcoef = nullptr;
    if (with_grad) {                                  // the doubles start at the next multiple of 8 bytes
        uintptr_t d = reinterpret_cast<uintptr_t>(bytes + (P + 3) / 4);
        a.pcoef = reinterpret_cast<double*>((d + 7) & ~(uintptr_t)7);
    }
    a.im0_cs = im0_cs; a.im1_cs = im1_cs; a.flow_cs = flow_cs; a.dflow_cs = 0;
    a.N = N; a.H = H; a.W = W; a.C = C;
    a.flow_scale = flow_scale; a.c1 = (double)c1; a.c2 = (double)c2; a.accumulate = 0;
    return a;
}

template <bool GRAD>
static void ssim_prepare_launch(const SsimArgs& a, pwc_stream_t stream) {
    const dim3 grid = pwc_loss_grad_blocks(a.N, a.H, a.W);
    switch (a.C) {
    case 1: hipLaunchKernelGGL((ssim_prepare_kernel<1, GRAD>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL((ssim_prepare_kernel<2, GRAD>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 3: hipLaunchKernelGGL((ssim_prepare_kernel<3, GRAD>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL((ssim_prepare_kernel<4, GRAD>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    }
}

template <bool SUMS>
static void ssim_window_launch(const SsimArgs& a, int radius, pwc_stream_t stream) {
    const dim3 grid((unsigned)ssim_parts(a.H, a.W), (unsigned)a.N);
    switch (radius) {
    case 1: hipLaunchKernelGGL((ssim_window_kernel<1, SUMS>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL((ssim_window_kernel<2, SUMS>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL((ssim_window_kernel<3, SUMS>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    }
}

extern "C" int pwc_ssim_sums_f32(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                                 float flow_scale, const uint8_t* valid, int N, int H, int W, int C, int radius, float c1, float c2,
                                 float* workspace, size_t workspace_floats, float* out_sums, int32_t* out_counts,
                                 pwc_stream_t stream) {
    const int rc = ssim_check(im0, im0_cs, im1, im1_cs, flow, flow_cs, N, H, W, C, radius, c1, c2, workspace, workspace_floats, 0);
    if (rc != PWC_OK) return rc;
    if (!out_sums || !out_counts) return PWC_EINVAL;
    const SsimArgs a = ssim_args(im0, im0_cs, im1, im1_cs, flow, flow_cs, flow_scale, valid, N, H, W, C, c1, c2, workspace, 0);
    ssim_prepare_launch<false>(a, stream);
    ssim_window_launch<true>(a, radius, stream);
    pwc_loss_final_launch(workspace, (int)ssim_parts(H, W), N, out_sums, out_counts, stream);
    return pwc_launch_status();
}

extern "C" int pwc_ssim_grad_f32(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                                 float flow_scale, const uint8_t* valid, int N, int H, int W, int C, int radius, float c1, float c2,
                                 const float* dsums, float* workspace, size_t workspace_floats, float* dflow, int dflow_cs,
                                 int accumulate, pwc_stream_t stream) {
    const int rc = ssim_check(im0, im0_cs, im1, im1_cs, flow, flow_cs, N, H, W, C, radius, c1, c2, workspace, workspace_floats, 1);
    if (rc != PWC_OK) return rc;
    if (!dsums || !dflow || dflow_cs < 2) return PWC_EINVAL;
    SsimArgs a = ssim_args(im0, im0_cs, im1, im1_cs, flow, flow_cs, flow_scale, valid, N, H, W, C, c1, c2, workspace, 1);
    a.dsums = dsums; a.dflow = dflow; a.dflow_cs = dflow_cs; a.accumulate = accumulate;
    ssim_prepare_launch<true>(a, stream);
    ssim_window_launch<false>(a, radius, stream);
    const dim3 grid((unsigned)ssim_parts(H, W), (unsigned)N);
    switch (radius) {
    case 1: hipLaunchKernelGGL(ssim_grad_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL(ssim_grad_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL(ssim_grad_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    }
    return pwc_launch_status();
}
