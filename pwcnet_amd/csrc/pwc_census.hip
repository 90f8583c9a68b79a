// pwc_census.hip -- the soft census (ternary) photometric term of label-free training: per-image sums and their gradient with
// respect to the flow (gfx950; C ABI in include/pwc_hip.h, "self-supervised losses").
//
//   pwc_census_sums_f32   per-image sums of rho(h) over the contributing pixels and their number
//   pwc_census_grad_f32   the gradient of those sums w.r.t. the flow, times an upstream gradient per image
//
// Grey planes: a = scale * mean_c images_0, b = scale * mean_c (bilinear sample of images_1 at the pixel moved by flow_scale *
// flow), 0 where the sample point is out of frame.  Window of radius r, K = (2r+1)^2 - 1 offsets o != 0:
//   t0 = a(p+o) - a(p), t1 = b(p+o) - b(p), tau(t) = t / sqrt(c1 + t^2), d = (tau(t0) - tau(t1))^2, h(p) = (1/K) sum_o d / (c2 + d).
// A pixel CONTRIBUTES rho(h) iff it is r pixels from every border, in frame, and valid; the mask and the in-frame test select
// centres only, a neighbour is always read.
//
// Three passes, every one deterministic:
//   prepare   one lane per pixel: a, b, the in-frame flag and (gradient) the sample's derivatives along x and y into workspace
//             planes.  Sample point, weights and blend in double, rounded once: photo_pixel's arithmetic (pwc_unsup.hip).
//   window    a workgroup owns 32 x 8 tiles of centres, one lane per centre; it stages the tile and an r-pixel halo of a and b
//             in the LDS ((32+2r) x (8+2r) floats per plane; cells outside the image hold 0 and belong to no contributing
//             centre's window), so that the K neighbours cost LDS reads, not K passes over memory.  The sums kernel adds rho(h)
//             over its tiles -- part b of at most 256 takes the tiles b, b + parts, ... -- in loss_common.h's tree, one thread per
//             image adds the parts in index order.  The gradient's first kernel writes G(p) = dsums[n] rho'(h(p)) / K (0 where p
//             does not contribute) to a plane instead.
//   gather    same tiling with a, b and G staged (G is 0 outside the image).  tau is odd, so pixel q's two roles -- centre, and
//             neighbour of the centre q+o -- fold into one loop:  dL/db(q) = -sum_o (G(q) + G(q+o)) D(t0, t1) with
//             D = c2 / (c2 + d)^2 * 2 (tau(t1) - tau(t0)) * c1 / (c1 + t1^2)^(3/2), and dflow(q) = flow_scale * scale * dL/db(q) *
//             (db/dx, db/dy) where q is in frame.  No atomics.
#include "loss_common.h"

constexpr int CENSUS_TW = 32, CENSUS_TH = 8;      // centres of a tile: one per lane of the 256

struct CensusArgs {
    const float* im0;
    const float* im1;
    const float* flow;
    const uint8_t* valid;    // [N][H][W], null: every pixel
    const float* dsums;      // [N] upstream gradient (grad)
    float* dflow;            // 2 channels, written or accumulated (grad)
    float* pa;               // workspace planes [N][H][W]: a, b
    float* pb;
    float* pgx;              // mean_c d sample / d x, d y (grad)
    float* pgy;
    float* pG;               // (grad)
    uint8_t* inframe;        // [N][H][W]
    float* partial;          // [N][gridDim.x] sums
    int* partial_n;          // [N][gridDim.x] counts of contributing pixels
    int im0_cs, im1_cs, flow_cs, dflow_cs;
    int N, H, W;
    float flow_scale, scale, c1, c2, eps2, q;
    int accumulate;
};

// ------------------------------------------------------------------ prepare
template <int C, bool GRAD>
__global__ __launch_bounds__(256) void census_prepare_kernel(const CensusArgs a) {
    const long npix = (long)a.N * a.H * a.W;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        const PwcLossPixel px = pwc_loss_pixel(p, a.H, a.W);
        const float* p0 = a.im0 + p * a.im0_cs;
        double s0 = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) s0 += (double)p0[c];
        a.pa[p] = (float)((double)a.scale * (s0 / (double)C));
        const float* fp = a.flow + p * a.flow_cs;
        const double sx = (double)px.x + (double)fp[0] * (double)a.flow_scale, sy = (double)px.y + (double)fp[1] * (double)a.flow_scale;
        float b = 0.f, gx = 0.f, gy = 0.f;
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
            double sb = 0.0, dx = 0.0, dy = 0.0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double v00 = p00[c], v01 = p01[c], v10 = p10[c], v11 = p11[c];
                sb += wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11);
                if (GRAD) {
                    dx += wy0 * (v01 - v00) + wy1 * (v11 - v10);
                    dy += wx0 * (v10 - v00) + wx1 * (v11 - v01);
                }
            }
            b = (float)((double)a.scale * (sb / (double)C));
            gx = (float)(dx / (double)C);
            gy = (float)(dy / (double)C);
        }
        a.pb[p] = b;
        a.inframe[p] = in ? 1 : 0;
        if (GRAD) {
            a.pgx[p] = gx;
            a.pgy[p] = gy;
        }
    }
}

// ------------------------------------------------------------------ window
template <int R>
struct CensusTile {
    static constexpr int LW = CENSUS_TW + 2 * R, LH = CENSUS_TH + 2 * R, CELLS = LW * LH, K = (2 * R + 1) * (2 * R + 1) - 1;
};

// The tile whose first centre is (ty0, tx0) of image n, with its halo, from `planes` workspace planes into the LDS; a cell
// outside the image gets 0.  Barriers: the readers of the previous tile are done before, the cells are published after.
template <int R, int PLANES>
__device__ __forceinline__ void census_stage(int n, int ty0, int tx0, int H, int W, const float* const* planes,
                                             float (*lds)[CensusTile<R>::CELLS]) {
    using T = CensusTile<R>;
    __syncthreads();
    for (int i = threadIdx.x; i < T::CELLS; i += 256) {
        const int cy = i / T::LW, cx = i - cy * T::LW;
        const int gy = ty0 - R + cy, gx = tx0 - R + cx;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t g = in ? ((size_t)n * H + gy) * W + gx : 0;
#pragma unroll
        for (int k = 0; k < PLANES; ++k) lds[k][i] = in ? planes[k][g] : 0.f;
    }
    __syncthreads();
}

// h of the centre in LDS cell c
template <int R>
__device__ __forceinline__ float census_h(const float* sa, const float* sb, int c, float c1, float c2) {
    using T = CensusTile<R>;
    const float a0 = sa[c], b0 = sb[c];
    float h = 0.f;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const int o = c + dy * T::LW + dx;
            const float t0 = sa[o] - a0, t1 = sb[o] - b0;
            const float e = t0 / sqrtf(c1 + t0 * t0) - t1 / sqrtf(c1 + t1 * t1);
            const float d = e * e;
            h += d / (c2 + d);
        }
    }
    return h / (float)T::K;
}

// SUMS: this workgroup's part of image blockIdx.y's sum and count.  Otherwise: the plane G.
template <int R, bool SUMS>
__global__ __launch_bounds__(256) void census_window_kernel(const CensusArgs a) {
    using T = CensusTile<R>;
    __shared__ float lds[2][T::CELLS];
    const int n = blockIdx.y;
    const int tiles_x = (a.W + CENSUS_TW - 1) / CENSUS_TW, tiles = tiles_x * ((a.H + CENSUS_TH - 1) / CENSUS_TH);
    const int ly = threadIdx.x / CENSUS_TW, lx = threadIdx.x % CENSUS_TW;
    const float* planes[2] = {a.pa, a.pb};
    float s = 0.f;
    int cnt = 0;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty0 = (tile / tiles_x) * CENSUS_TH, tx0 = (tile % tiles_x) * CENSUS_TW;
        census_stage<R, 2>(n, ty0, tx0, a.H, a.W, planes, lds);
        const int y = ty0 + ly, x = tx0 + lx;
        if (y < a.H && x < a.W) {
            const size_t p = ((size_t)n * a.H + y) * a.W + x;
            const bool contributes = y >= R && y < a.H - R && x >= R && x < a.W - R && a.inframe[p] && (!a.valid || a.valid[p]);
            float h = 0.f;
            if (contributes) h = census_h<R>(lds[0], lds[1], (ly + R) * T::LW + lx + R, a.c1, a.c2);
            if (SUMS) {
                if (contributes) {
                    s += unsup_rho(h, a.eps2, a.q);
                    ++cnt;
                }
            } else {
                a.pG[p] = contributes ? a.dsums[n] * unsup_rho_grad(h, a.eps2, a.q) / (float)T::K : 0.f;
            }
        }
    }
    if (SUMS) pwc_loss_write_part<true>(s, cnt, a.partial, a.partial_n);
}

// ------------------------------------------------------------------ gather
template <int R>
__global__ __launch_bounds__(256) void census_grad_kernel(const CensusArgs a) {
    using T = CensusTile<R>;
    __shared__ float lds[3][T::CELLS];
    const int n = blockIdx.y;
    const int tiles_x = (a.W + CENSUS_TW - 1) / CENSUS_TW, tiles = tiles_x * ((a.H + CENSUS_TH - 1) / CENSUS_TH);
    const int ly = threadIdx.x / CENSUS_TW, lx = threadIdx.x % CENSUS_TW;
    const float* planes[3] = {a.pa, a.pb, a.pG};
    const float up = a.flow_scale * a.scale;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty0 = (tile / tiles_x) * CENSUS_TH, tx0 = (tile % tiles_x) * CENSUS_TW;
        census_stage<R, 3>(n, ty0, tx0, a.H, a.W, planes, lds);
        const int y = ty0 + ly, x = tx0 + lx;
        if (y < a.H && x < a.W) {
            const size_t p = ((size_t)n * a.H + y) * a.W + x;
            float* o = a.dflow + p * a.dflow_cs;
            if (!a.inframe[p]) {
                pwc_grad_skip2(o, a.accumulate);
            } else {
                const float* sa = lds[0];
                const float* sb = lds[1];
                const float* sg = lds[2];
                const int c = (ly + R) * T::LW + lx + R;
                const float a0 = sa[c], b0 = sb[c], g0 = sg[c];
                float acc = 0.f;
#pragma unroll
                for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
                    for (int dx = -R; dx <= R; ++dx) {
                        if (dy == 0 && dx == 0) continue;
                        const int k = c + dy * T::LW + dx;
                        const float t0 = sa[k] - a0, t1 = sb[k] - b0;
                        const float q1 = a.c1 + t1 * t1, s1 = sqrtf(q1);
                        const float e = t1 / s1 - t0 / sqrtf(a.c1 + t0 * t0);
                        const float den = a.c2 + e * e;
                        acc += (g0 + sg[k]) * (a.c2 / (den * den) * (2.f * e) * (a.c1 / (q1 * s1)));
                    }
                }
                // (the products are rounded on their own: accumulate adds exactly what a plain call writes)
                const float w = pwc_mul_rounded(up, -acc);
                pwc_grad_store2(o, a.accumulate, 1.f, pwc_mul_rounded(w, a.pgx[p]), pwc_mul_rounded(w, a.pgy[p]));
            }
        }
    }
}

// ------------------------------------------------------------------ host
// The tiles of an image are cut into at most 256 parts: part b takes the tiles b, b + parts, ...
static inline long census_parts(int H, int W) {
    const long tiles = (((long)W + CENSUS_TW - 1) / CENSUS_TW) * (((long)H + CENSUS_TH - 1) / CENSUS_TH);
    return tiles > 256 ? 256 : tiles;
}

// workspace: [2][N][parts] sums and counts, the planes a and b (with_grad: and d/dx, d/dy, G), the in-frame bytes
extern "C" size_t pwc_census_workspace_floats(int N, int H, int W, int with_grad) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    const size_t P = (size_t)N * H * W;
    return 2 * (size_t)N * census_parts(H, W) + (with_grad ? 5 : 2) * P + (P + 3) / 4;
}

static int census_check(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs, int N, int H,
                        int W, int C, int radius, float scale, float c1, float c2, float eps, float q, const float* workspace,
                        size_t workspace_floats, int with_grad) {
    if (!im0 || !im1 || !flow || N <= 0 || H <= 0 || W <= 0) return PWC_EINVAL;
    if (C < 1 || C > 4 || radius < 1 || radius > 3) return PWC_EUNSUPPORTED;
    if (im0_cs < C || im1_cs < C || flow_cs < 2) return PWC_EINVAL;
    if (!(eps > 0.f) || !(q > 0.f && q <= 1.f) || !(scale > 0.f) || !(c1 > 0.f) || !(c2 > 0.f)) return PWC_EINVAL;
    if (!pwc_loss_in_range(N, H, W)) return PWC_ERANGE;
    if (!workspace || workspace_floats < pwc_census_workspace_floats(N, H, W, with_grad)) return PWC_EINVAL;
    return PWC_OK;
}

static CensusArgs census_args(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                              float flow_scale, const uint8_t* valid, int N, int H, int W, float scale, float c1, float c2, float eps,
                              float q, float* workspace, int with_grad) {
    const size_t P = (size_t)N * H * W;
    CensusArgs a;
    a.im0 = im0; a.im1 = im1; a.flow = flow; a.valid = valid; a.dsums = nullptr; a.dflow = nullptr;
    a.partial = workspace; a.partial_n = reinterpret_cast<int*>(workspace + (size_t)N * census_parts(H, W));
    float* planes = workspace + 2 * (size_t)N * census_parts(H, W);
    a.pa = planes; a.pb = planes + P;
    a.pgx = with_grad ? planes + 2 * P : nullptr; a.pgy = with_grad ? planes + 3 * P : nullptr;
    a.pG = with_grad ? planes + 4 * P : nullptr;
    a.inframe = reinterpret_cast<uint8_t*>(planes + (with_grad ? 5 : 2) * P);
    a.im0_cs = im0_cs; a.im1_cs = im1_cs; a.flow_cs = flow_cs; a.dflow_cs = 0;
    a.N = N; a.H = H; a.W = W;
    a.flow_scale = flow_scale; a.scale = scale; a.c1 = c1; a.c2 = c2; a.eps2 = eps * eps; a.q = q; a.accumulate = 0;
    return a;
}

template <bool GRAD>
static void census_prepare_launch(const CensusArgs& a, int C, pwc_stream_t stream) {
    const dim3 grid = pwc_loss_grad_blocks(a.N, a.H, a.W);
    switch (C) {
    case 1: hipLaunchKernelGGL((census_prepare_kernel<1, GRAD>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL((census_prepare_kernel<2, GRAD>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 3: hipLaunchKernelGGL((census_prepare_kernel<3, GRAD>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL((census_prepare_kernel<4, GRAD>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    }
}

template <bool SUMS>
static void census_window_launch(const CensusArgs& a, int radius, pwc_stream_t stream) {
    const dim3 grid((unsigned)census_parts(a.H, a.W), (unsigned)a.N);
    switch (radius) {
    case 1: hipLaunchKernelGGL((census_window_kernel<1, SUMS>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL((census_window_kernel<2, SUMS>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL((census_window_kernel<3, SUMS>), grid, dim3(256), 0, (hipStream_t)stream, a); break;
    }
}

extern "C" int pwc_census_sums_f32(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                                   float flow_scale, const uint8_t* valid, int N, int H, int W, int C, int radius, float scale,
                                   float c1, float c2, float eps, float q, float* workspace, size_t workspace_floats,
                                   float* out_sums, int32_t* out_counts, pwc_stream_t stream) {
    const int rc = census_check(im0, im0_cs, im1, im1_cs, flow, flow_cs, N, H, W, C, radius, scale, c1, c2, eps, q, workspace,
                                workspace_floats, 0);
    if (rc != PWC_OK) return rc;
    if (!out_sums || !out_counts) return PWC_EINVAL;
    const CensusArgs a = census_args(im0, im0_cs, im1, im1_cs, flow, flow_cs, flow_scale, valid, N, H, W, scale, c1, c2, eps, q,
                                     workspace, 0);
    census_prepare_launch<false>(a, C, stream);
    census_window_launch<true>(a, radius, stream);
    pwc_loss_final_launch(workspace, (int)census_parts(H, W), N, out_sums, out_counts, stream);
    return pwc_launch_status();
}

extern "C" int pwc_census_grad_f32(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                                   float flow_scale, const uint8_t* valid, int N, int H, int W, int C, int radius, float scale,
                                   float c1, float c2, float eps, float q, const float* dsums, float* workspace,
                                   size_t workspace_floats, float* dflow, int dflow_cs, int accumulate, pwc_stream_t stream) {
    const int rc = census_check(im0, im0_cs, im1, im1_cs, flow, flow_cs, N, H, W, C, radius, scale, c1, c2, eps, q, workspace,
                                workspace_floats, 1);
    if (rc != PWC_OK) return rc;
    if (!dsums || !dflow || dflow_cs < 2) return PWC_EINVAL;
    CensusArgs a = census_args(im0, im0_cs, im1, im1_cs, flow, flow_cs, flow_scale, valid, N, H, W, scale, c1, c2, eps, q,
                               workspace, 1);
    a.dsums = dsums; a.dflow = dflow; a.dflow_cs = dflow_cs; a.accumulate = accumulate;
    census_prepare_launch<true>(a, C, stream);
    census_window_launch<false>(a, radius, stream);
    const dim3 grid((unsigned)census_parts(H, W), (unsigned)N);
    switch (radius) {
    case 1: hipLaunchKernelGGL(census_grad_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL(census_grad_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL(census_grad_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    }
    return pwc_launch_status();
}
