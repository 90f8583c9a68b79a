// pwc_temporal.hip -- motion-compensated temporal filter: every pixel of a frame averaged with what its trajectory through the
// 2 R neighbouring frames shows, each neighbour weighted by how well its patch matches and dropped, with everything beyond it,
// where the walk leaves the frame, meets an unknown flow or fails the forward-backward check (gfx950; C ABI in
// include/pwc_hip.h, "temporal filter"; semantics, launch shape and resource figures in DESIGN.md 24).
//
//   pwc_temporal_filter    filtered (i1 - i0, H, W, C) in the frames' dtype and support (i1 - i0, H, W) bytes from a clip of T
//                          frames, the T - 1 flows j -> j + 1 and the T - 1 flows j + 1 -> j
//
// One lane per output pixel, 32 x 8 tiles, grid (ceil(W / 32), ceil(H / 8), i1 - i0): a workgroup works on ONE output frame, so
// the bounds of the k loop are uniform in it.  The workgroup first stages the centre frame's tile and a halo of P pixels in the
// LDS as grey levels (doubles; coordinates clamped into the frame -- a clamped entry is never used, its offset is skipped).
// Then each lane walks +1, +2, .. +R and -1, .. -R: one step of pwc_track.hip's (temporal_step below is track_step with a
// VISIBLE state going in, operation for operation), and, where the step came through VISIBLE, the patch distance and the
// weighted sum.  A lane whose direction has ended idles to the end of the k loop; no lane waits for another (the one barrier is
// behind the LDS fill).
// The (2P+1)^2 bilinear samples around q share q's fractional part, so the (2P+2)^2 footprint is loaded once, row by row: a
// row's 2P+2 pixels give 2P+1 horizontal blends, two consecutive rows of blends give a row of samples.  Two rows of blends are
// live at a time (2 (2P+1) C doubles), not the footprint.
// Every value is an IEEE double + - x /, a floor, a rint or a comparison in the order written here -- no fused multiply-add is
// formed anywhere in this file (the pragma below) -- so tests/temporal_ref.py restates it in numpy bit for bit.  No atomics, no
// workspace, no host synchronisation, no process-wide state; frame and flow offsets are 64-bit.
#include "flow_record.h"

#pragma clang fp contract(off)

#define TEMPORAL_TILE_W 32
#define TEMPORAL_TILE_H 8

struct TemporalArgs {
    const void* frames;       // [T][H][W][C] bytes or floats, dense
    const float* fw;          // [T - 1][H][W] records of fw_cs floats, 2 used: the flows j -> j + 1
    const float* bw;          // the flows j + 1 -> j
    const uint8_t* vfw;       // [T - 1][H][W], null: every pixel
    const uint8_t* vbw;
    void* out;                // [i1 - i0][H][W][C]
    uint8_t* support;         // [i1 - i0][H][W]
    double s2;                // sigma sigma
    double md2;               // max_distance max_distance, used where md_on
    int fw_cs, bw_cs;
    int T, H, W, R, i0;
    int fb, md_on;
    float alpha1, alpha2;
};

__device__ __forceinline__ bool temporal_inside(double qx, double qy, int H, int W) {
    return qx >= 0.0 && qx <= (double)(W - 1) && qy >= 0.0 && qy <= (double)(H - 1);
}

// pwc_track.hip's track_sample: the bilinear sample of one frame's flow f (mask m or null) at a point INSIDE the frame; false
// where a corner is masked out or unknown.
__device__ __forceinline__ bool temporal_sample(const float* f, int cs, const uint8_t* m, int H, int W, double qx, double qy,
                                                double& s0, double& s1) {
    const PwcBilinearF64 bl = pwc_bilinear_f64(qx, qy, H, W);
    const double wx = bl.wx1, wy = bl.wy1;
    const size_t o00 = bl.o00, o01 = bl.o01, o10 = bl.o10, o11 = bl.o11;
    if (m && !(m[o00] && m[o01] && m[o10] && m[o11])) return false;
    const float* p00 = f + o00 * cs; const float* p01 = f + o01 * cs; const float* p10 = f + o10 * cs; const float* p11 = f + o11 * cs;
    const float a00 = p00[0], b00 = p00[1], a01 = p01[0], b01 = p01[1], a10 = p10[0], b10 = p10[1], a11 = p11[0], b11 = p11[1];
    if (!(pwc_flow_known(a00, b00) && pwc_flow_known(a01, b01) && pwc_flow_known(a10, b10) && pwc_flow_known(a11, b11))) return false;
    const double ux = bl.wx0, uy = bl.wy0;
    s0 = (uy * ((ux * (double)a00) + (wx * (double)a01))) + (wy * ((ux * (double)a10) + (wx * (double)a11)));
    s1 = (uy * ((ux * (double)b00) + (wx * (double)b01))) + (wy * ((ux * (double)b10) + (wx * (double)b11)));
    return true;
}

// pwc_track.hip's track_step for a VISIBLE point: true where it comes through VISIBLE, and then (x, y) is the new position.
__device__ __forceinline__ bool temporal_step(const TemporalArgs& a, const float* F, int f_cs, const uint8_t* Fm, const float* G,
                                              int g_cs, const uint8_t* Gm, float& x, float& y) {
    const double qx = (double)x, qy = (double)y;
    if (!temporal_inside(qx, qy, a.H, a.W)) return false;
    double S0, S1;
    if (!temporal_sample(F, f_cs, Fm, a.H, a.W, qx, qy, S0, S1)) return false;
    const double rx = qx + S0, ry = qy + S1;
    if (!temporal_inside(rx, ry, a.H, a.W)) return false;
    if (G) {
        double b0, b1;
        if (!temporal_sample(G, g_cs, Gm, a.H, a.W, rx, ry, b0, b1)) return false;
        const double d0 = S0 + b0, d1 = S1 + b1;
        const double bound = ((double)a.alpha1 * (((S0 * S0) + (S1 * S1)) + ((b0 * b0) + (b1 * b1)))) + (double)a.alpha2;
        const double margin = bound - ((d0 * d0) + (d1 * d1));
        if (!(margin >= 0.0)) return false;
    }
    x = (float)rx;
    y = (float)ry;
    return true;
}

// The grey level of one stored value: the byte, or 255 v with a NaN read as 0.
template <bool U8>
__device__ __forceinline__ double temporal_grey(const void* frames, size_t o) {
    if (U8) return (double)reinterpret_cast<const uint8_t*>(frames)[o];
    const double v = (double)reinterpret_cast<const float*>(frames)[o];
    return v == v ? 255.0 * v : 0.0;
}

template <bool U8, int C, int P>
__global__ __launch_bounds__(256) void temporal_filter_kernel(const TemporalArgs a) {
    constexpr int LW = TEMPORAL_TILE_W + 2 * P, LH = TEMPORAL_TILE_H + 2 * P, S = 2 * P + 1;
    __shared__ double centre[LH * LW * C];
    const int H = a.H, W = a.W;
    const size_t plane = (size_t)H * W;
    const int i = a.i0 + (int)blockIdx.z;
    const int bx = blockIdx.x * TEMPORAL_TILE_W, by = blockIdx.y * TEMPORAL_TILE_H;
    const size_t own = (size_t)i * plane * C;
    for (int e = threadIdx.x; e < LH * LW; e += 256) {
        const int ly = e / LW, lx = e - ly * LW;
        const int gy = min(max(by + ly - P, 0), H - 1), gx = min(max(bx + lx - P, 0), W - 1);
        const size_t o = own + ((size_t)gy * W + gx) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) centre[e * C + c] = temporal_grey<U8>(a.frames, o + c);
    }
    __syncthreads();
    const int tx = threadIdx.x & (TEMPORAL_TILE_W - 1), ty = threadIdx.x / TEMPORAL_TILE_W;
    const int px = bx + tx, py = by + ty;
    if (px >= W || py >= H) return;
    const double* mine = centre + ((ty + P) * LW + (tx + P)) * C;
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = mine[c];
    double wsum = 1.0;
    unsigned support = 0u;
    // the offsets of the patch that are inside the frame, as bits (row-major), and their number times C
    unsigned inside = 0u;
    int terms = 0;
#pragma unroll
    for (int oy = -P; oy <= P; ++oy)
#pragma unroll
        for (int ox = -P; ox <= P; ++ox)
            if (px + ox >= 0 && px + ox < W && py + oy >= 0 && py + oy < H) {
                inside |= 1u << ((oy + P) * S + (ox + P));
                terms += C;
            }
    const double count = (double)terms;
    for (int dir = 0; dir < 2; ++dir) {
        float x = (float)px, y = (float)py;
        bool alive = true;
        for (int k = 1; k <= a.R; ++k) {
            const int f = dir ? i - k : i + k;
            if (f < 0 || f >= a.T) break;                                  // (uniform in the workgroup)
            if (!alive) continue;
            const size_t j = (size_t)(dir ? i - k : i + k - 1) * plane;    // the flows between frames j and j + 1
            const float* F = dir ? a.bw + j * a.bw_cs : a.fw + j * a.fw_cs;
            const float* G = dir ? a.fw + j * a.fw_cs : a.bw + j * a.bw_cs;
            const uint8_t* Fm = dir ? a.vbw : a.vfw;
            const uint8_t* Gm = dir ? a.vfw : a.vbw;
            alive = temporal_step(a, F, dir ? a.bw_cs : a.fw_cs, Fm ? Fm + j : nullptr, a.fb ? G : nullptr, dir ? a.fw_cs : a.bw_cs,
                                  Gm ? Gm + j : nullptr, x, y);
            if (!alive) continue;
            // the samples of frame f around q = (x, y), which is inside the frame
            const double qx = (double)x, qy = (double)y;
            // (not pwc_bilinear_f64: the footprint of a patch, S + 1 rows and columns each clamped on both sides)
            const double fx0 = floor(qx), fy0 = floor(qy);
            const int x0 = (int)fx0, y0 = (int)fy0;
            const double wx = qx - fx0, wy = qy - fy0, ux = 1.0 - wx, uy = 1.0 - wy;
            const size_t other = (size_t)f * plane * C;
            double hp[S][C], hc[S][C], b[C];
            double sum = 0.0;
#pragma unroll
            for (int r = 0; r < S + 1; ++r) {                              // footprint rows y0 - P + r
                const int yy = min(max(y0 - P + r, 0), H - 1);
                const size_t row = other + (size_t)yy * W * C;
                double g0[C], g1[C];
#pragma unroll
                for (int c = 0; c < C; ++c) g0[c] = temporal_grey<U8>(a.frames, row + (size_t)min(max(x0 - P, 0), W - 1) * C + c);
#pragma unroll
                for (int jx = 0; jx < S; ++jx) {
                    const int xx = min(max(x0 - P + jx + 1, 0), W - 1);
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        g1[c] = temporal_grey<U8>(a.frames, row + (size_t)xx * C + c);
                        hc[jx][c] = (ux * g0[c]) + (wx * g1[c]);
                        g0[c] = g1[c];
                    }
                }
                if (r > 0) {                                               // the samples of patch row oy = r - 1 - P
#pragma unroll
                    for (int jx = 0; jx < S; ++jx) {
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const double v = (uy * hp[jx][c]) + (wy * hc[jx][c]);
                            if (r - 1 == P && jx == P) b[c] = v;
                            if (inside & (1u << ((r - 1) * S + jx))) {
                                const double df = mine[((r - 1 - P) * LW + (jx - P)) * C + c] - v;
                                sum = sum + (df * df);
                            }
                        }
                    }
                }
#pragma unroll
                for (int jx = 0; jx < S; ++jx)
#pragma unroll
                    for (int c = 0; c < C; ++c) hp[jx][c] = hc[jx][c];
            }
            const double d2 = sum / count;
            double w = 1.0 / (1.0 + (d2 / a.s2));
            if (a.md_on && d2 > a.md2) w = 0.0;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = acc[c] + (w * b[c]);
            wsum = wsum + w;
            if (w > 0.0) support += 1u;
        }
    }
    const size_t o = (size_t)blockIdx.z * plane + (size_t)py * W + px;
    a.support[o] = (uint8_t)support;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double v = acc[c] / wsum;
        if (U8) reinterpret_cast<uint8_t*>(a.out)[o * C + c] = (uint8_t)pwc_round_byte(v);
        else reinterpret_cast<float*>(a.out)[o * C + c] = (float)(v / 255.0);
    }
}

// ---------------------------------------------------------------- host
template <bool U8, int C>
static void temporal_launch(int P, dim3 grid, hipStream_t s, const TemporalArgs& a) {
    if (P == 0) hipLaunchKernelGGL((temporal_filter_kernel<U8, C, 0>), grid, dim3(256), 0, s, a);
    else if (P == 1) hipLaunchKernelGGL((temporal_filter_kernel<U8, C, 1>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((temporal_filter_kernel<U8, C, 2>), grid, dim3(256), 0, s, a);
}

extern "C" int pwc_temporal_filter(const void* frames, int dtype, int C, const float* flows_fw, int fw_cs, const float* flows_bw,
                                   int bw_cs, const uint8_t* valids_fw, const uint8_t* valids_bw, int T, int H, int W, int radius,
                                   int patch, double sigma, double max_distance, int fb_check, float alpha1, float alpha2, int i0,
                                   int i1, void* filtered, uint8_t* support, pwc_stream_t stream) {
    if (!frames || !filtered || !support || T < 1 || H < 1 || W < 1) return PWC_EINVAL;
    if (T > 1 && (!flows_fw || !flows_bw || fw_cs < 2 || bw_cs < 2)) return PWC_EINVAL;
    if ((dtype != PWC_TEMPORAL_U8 && dtype != PWC_TEMPORAL_F32) || (C != 1 && C != 3)) return PWC_EINVAL;
    if (radius < 1 || radius > PWC_TEMPORAL_MAX_RADIUS || patch < 0 || patch > PWC_TEMPORAL_MAX_PATCH) return PWC_EINVAL;
    // (a NaN fails; sigma sigma must be a positive finite double too)
    if (!(sigma > 0.0) || !(sigma * sigma > 0.0) || !pwc_finite(sigma * sigma) || max_distance != max_distance)
        return PWC_EINVAL;
    if (fb_check && (!(alpha1 >= 0.f) || !(alpha2 >= 0.f))) return PWC_EINVAL;
    if (i0 < 0 || i1 > T || i0 >= i1) return PWC_EINVAL;
    // (float)rx with rx <= W - 1 stays inside the frame only while W - 1 is a float32: W <= 2^24 (pwc_track.hip's bound)
    if (H > (1 << 24) || W > (1 << 24) || (long)H * W >= (1L << 31) || T > 65535 || (H + TEMPORAL_TILE_H - 1) / TEMPORAL_TILE_H > 65535)
        return PWC_ERANGE;
    const bool u8 = dtype == PWC_TEMPORAL_U8;
    if ((T > 1 && (pwc_off(flows_fw, 3u) || pwc_off(flows_bw, 3u))) || (!u8 && (pwc_off(frames, 3u) || pwc_off(filtered, 3u))))
        return PWC_EALIGN;
    TemporalArgs a = {};
    a.frames = frames; a.fw = flows_fw; a.bw = flows_bw; a.vfw = T > 1 ? valids_fw : nullptr; a.vbw = T > 1 ? valids_bw : nullptr;
    a.out = filtered; a.support = support;
    a.s2 = sigma * sigma;
    a.md_on = max_distance > 0.0 ? 1 : 0;
    a.md2 = max_distance * max_distance;
    a.fw_cs = fw_cs; a.bw_cs = bw_cs; a.T = T; a.H = H; a.W = W; a.R = radius; a.i0 = i0;
    a.fb = fb_check ? 1 : 0;
    a.alpha1 = alpha1; a.alpha2 = alpha2;
    const dim3 grid((W + TEMPORAL_TILE_W - 1) / TEMPORAL_TILE_W, (H + TEMPORAL_TILE_H - 1) / TEMPORAL_TILE_H, i1 - i0);
    const hipStream_t s = (hipStream_t)stream;
    if (u8) { if (C == 1) temporal_launch<true, 1>(patch, grid, s, a); else temporal_launch<true, 3>(patch, grid, s, a); }
    else { if (C == 1) temporal_launch<false, 1>(patch, grid, s, a); else temporal_launch<false, 3>(patch, grid, s, a); }
    return pwc_launch_status();
}
