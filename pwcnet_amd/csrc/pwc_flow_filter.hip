// pwc_flow_filter.hip -- the image-guided weighted median of a flow field: smoothing that keeps motion edges, and filling of
// unknown pixels from their known neighbours (gfx950; C ABI and the definition in include/pwc_hip.h, "flow filter"; launch plan,
// operation counts and resource figures in DESIGN.md 23).
//
//   pwc_flow_filter_workspace_bytes   one intermediate field (8 bytes of flow and a byte of mask per pixel) where iters > 1
//   pwc_flow_filter_f32               out (N, H, W) records of out_cs floats, 2 written, and out_valid (N, H, W) bytes
//
// One launch per pass.  A workgroup of 256 lanes owns 32 x 8 tiles of centres, one lane per centre; it stages the tile and an
// r-pixel apron in the LDS as three planes of (32+2r) x (8+2r) dwords -- the ordered key of u, the ordered key of v, and a dword
// packing the guide bytes (bits 0 .. 23) with the Known flag (bit 31) -- next to the space table and the colour table.  A cell
// outside the frame is staged as not Known: nothing is replicated beyond the border.
//
// The median is a SELECTION on integers, nothing is sorted and no lane keeps an array of the window in memory:
//   weights   w = space[o] * colour[d] < 2^32, d the sum of absolute differences of the guide bytes (one v_sad_u8), 0 for a cell
//             that is not Known.  n counts the w > 0, T is their 64-bit sum.
//   bits      (r >= 2) the key K is built from bit 31 down: a round walks the window and adds the weights of the cells whose key
//             is below prefix | bit, for u and v at once; the bit is set iff twice that sum is below T.  After 32 rounds K is the
//             smallest key whose cumulative weight reaches T / 2, which is a candidate's key because the cumulative weight only
//             steps at candidates.  r <= 3 keeps the (2r+1)^2 weights in registers across the rounds, r >= 4 forms them again
//             in every round (225 registers at r = 7 would not leave the rest room).
//   counting  (r = 1) the nine keys and weights sit in registers; every candidate's cumulative weight is summed directly and the
//             smallest key that reaches T / 2 wins: 81 compare-and-adds per component against 32 x 9 = 288.
// Every lane runs the same trip counts; no loop waits for another lane.  All sums are exact integers: the order cannot matter.
// The passes of iters > 1 alternate between the workspace and out so that the last one writes out; every pass reads the field and
// the mask of the pass before.
#include "flow_record.h"

#pragma clang fp contract(fast)   // (flow_record.h turns contraction off behind it; this file's arithmetic is contracted)

constexpr int FILTER_TW = 32, FILTER_TH = 8;          // centres of a tile: one per lane of the 256
constexpr int FILTER_MAX_TILES_X = 1024;              // workgroups per image, tile-stride beyond
constexpr unsigned FILTER_KNOWN = 0x80000000u;

typedef unsigned long long filter_u64;

struct FilterArgs {
    const float* flow;        // [N][H][W] records of flow_cs floats, 2 used
    const uint8_t* valid;     // [N][H][W], null: every pixel
    const void* guide;        // [N][H][W][C] bytes or floats, null: no guide
    const uint32_t* space;    // (2r+1)^2
    const uint32_t* color;    // 255 C + 1, not read without a guide
    float* out;               // [N][H][W] records of out_cs floats, 2 written
    uint8_t* out_valid;       // [N][H][W]
    int flow_cs, out_cs, guide_c, guide_f32;
    int N, H, W;
    int smooth, fill, min_count;
};

// The total order of the definition: negative floats reversed below the positive ones, -0 < +0.
__device__ __forceinline__ unsigned filter_key(unsigned b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ unsigned filter_unkey(unsigned k) { return (k >> 31) ? (k ^ 0x80000000u) : ~k; }

// A float guide value as a byte: rint(clamp(255 v, 0, 255)) in double, ties to even, 0 for a NaN.  Not pwc_round_byte: the clamp
// comes before the rint.
__device__ __forceinline__ unsigned filter_byte(float v) {
    const double t = (double)v * 255.0;
    const double c = t >= 255.0 ? 255.0 : (t >= 0.0 ? t : 0.0);           // (both comparisons are false for a NaN)
    return (unsigned)(int)rint(c);
}

template <int R>
struct FilterTile {
    static constexpr int LW = FILTER_TW + 2 * R, LH = FILTER_TH + 2 * R, CELLS = LW * LH, D = 2 * R + 1, TAPS = D * D;
};

// The guide bytes of pixel g packed into bits 0 .. 23 (a single channel in bits 0 .. 7).
__device__ __forceinline__ unsigned filter_guide(const FilterArgs& a, size_t g) {
    if (!a.guide) return 0u;
    unsigned p = 0u;
    if (a.guide_f32) {
        const float* s = reinterpret_cast<const float*>(a.guide) + g * a.guide_c;
        for (int c = 0; c < a.guide_c; ++c) p |= filter_byte(s[c]) << (8 * c);
    } else {
        const uint8_t* s = reinterpret_cast<const uint8_t*>(a.guide) + g * a.guide_c;
        for (int c = 0; c < a.guide_c; ++c) p |= (unsigned)s[c] << (8 * c);
    }
    return p;
}

// The tile whose first centre is (ty0, tx0) of image n, with its apron.  A cell outside the frame is not Known and holds zeros.
// Barriers: the readers of the previous tile are done before, the cells are published after.
template <int R>
__device__ __forceinline__ void filter_stage(const FilterArgs& a, int n, int ty0, int tx0, unsigned* ku, unsigned* kv, unsigned* gk) {
    using T = FilterTile<R>;
    __syncthreads();
    for (int i = threadIdx.x; i < T::CELLS; i += 256) {
        const int cy = i / T::LW, cx = i - cy * T::LW;
        const int gy = ty0 - R + cy, gx = tx0 - R + cx;
        unsigned u = 0u, v = 0u, g = 0u;
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
            const size_t p = ((size_t)n * a.H + gy) * a.W + gx;
            const float* f = a.flow + p * a.flow_cs;
            const float fu = f[0], fv = f[1];
            // the .flo sentinel rule (flow_io.flow_valid): false for a NaN, an Inf, the sentinel
            const bool known = (!a.valid || a.valid[p]) && pwc_flow_known(fu, fv);
            u = filter_key(__float_as_uint(fu));
            v = filter_key(__float_as_uint(fv));
            g = filter_guide(a, p) | (known ? FILTER_KNOWN : 0u);
        }
        ku[i] = u; kv[i] = v; gk[i] = g;
    }
    __syncthreads();
}

// The weight of window cell `cell` as seen from a centre whose guide bytes are `centre`: 0 for a cell that is not Known.
__device__ __forceinline__ unsigned filter_weight(unsigned cell, unsigned centre, unsigned space, const unsigned* ctab) {
    const unsigned d = __builtin_amdgcn_sad_u8(cell & 0x00FFFFFFu, centre, 0u);     // <= 765
    return (cell & FILTER_KNOWN) ? space * ctab[d] : 0u;
}

template <int R>
__global__ __launch_bounds__(256) void flow_filter_kernel(const FilterArgs a) {
    using T = FilterTile<R>;
    constexpr bool COUNTING = R == 1, CACHED = R <= 3;
    __shared__ unsigned ku[T::CELLS], kv[T::CELLS], gk[T::CELLS];
    __shared__ unsigned stab[T::TAPS], ctab[766];
    const int n = blockIdx.y;
    const int tiles_x = (a.W + FILTER_TW - 1) / FILTER_TW, tiles = tiles_x * ((a.H + FILTER_TH - 1) / FILTER_TH);
    const int ly = threadIdx.x / FILTER_TW, lx = threadIdx.x % FILTER_TW;
    // (published by the first filter_stage's barriers.)  Without a guide d is always 0 and its weight is 1.
    for (int i = threadIdx.x; i < T::TAPS; i += 256) stab[i] = a.space[i];
    const int colors = a.guide ? 255 * a.guide_c + 1 : 1;
    for (int i = threadIdx.x; i < colors; i += 256) ctab[i] = a.guide ? a.color[i] : 1u;

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty0 = (tile / tiles_x) * FILTER_TH, tx0 = (tile % tiles_x) * FILTER_TW;
        filter_stage<R>(a, n, ty0, tx0, ku, kv, gk);
        const int y = ty0 + ly, x = tx0 + lx;
        if (y >= a.H || x >= a.W) continue;                                // (no barrier below: the next one is filter_stage's)
        const int c = (ly + R) * T::LW + lx + R;
        const unsigned centre = gk[c];
        const bool known = (centre & FILTER_KNOWN) != 0u;
        const unsigned cg = centre & 0x00FFFFFFu;
        unsigned ou = ku[c], ov = kv[c];                                   // keys of the output
        bool ok = known;
        if (known ? a.smooth != 0 : a.fill != 0) {
            // ---- n and T (and, cached, the weights)
            unsigned w[CACHED ? T::TAPS : 1];
            int cnt = 0;
            filter_u64 total = 0;
            if (CACHED) {
#pragma unroll
                for (int dy = 0; dy < T::D; ++dy) {
#pragma unroll
                    for (int dx = 0; dx < T::D; ++dx) {
                        const int t = dy * T::D + dx;
                        w[t] = filter_weight(gk[c + (dy - R) * T::LW + (dx - R)], cg, stab[t], ctab);
                        cnt += w[t] != 0u;
                        total += w[t];
                    }
                }
            } else {
#pragma unroll 1
                for (int dy = 0; dy < T::D; ++dy) {
#pragma unroll
                    for (int dx = 0; dx < T::D; ++dx) {
                        const unsigned wt = filter_weight(gk[c + (dy - R) * T::LW + (dx - R)], cg, stab[dy * T::D + dx], ctab);
                        cnt += wt != 0u;
                        total += wt;
                    }
                }
            }
            const bool take = known ? cnt >= 1 : cnt >= a.min_count;
            if (take && cnt >= 1) {
                ok = true;
                if (COUNTING) {
                    // ---- every candidate's cumulative weight; the smallest key that reaches T / 2
                    unsigned wu[T::TAPS], wv[T::TAPS];
#pragma unroll
                    for (int dy = 0; dy < T::D; ++dy) {
#pragma unroll
                        for (int dx = 0; dx < T::D; ++dx) {
                            wu[dy * T::D + dx] = ku[c + (dy - R) * T::LW + (dx - R)];
                            wv[dy * T::D + dx] = kv[c + (dy - R) * T::LW + (dx - R)];
                        }
                    }
                    unsigned bu = 0xFFFFFFFFu, bv = 0xFFFFFFFFu;
#pragma unroll
                    for (int i = 0; i < T::TAPS; ++i) {
                        filter_u64 su = 0, sv = 0;
#pragma unroll
                        for (int j = 0; j < T::TAPS; ++j) {
                            su += wu[j] <= wu[i] ? w[j] : 0u;
                            sv += wv[j] <= wv[i] ? w[j] : 0u;
                        }
                        if (w[i] != 0u && 2 * su >= total) bu = min(bu, wu[i]);
                        if (w[i] != 0u && 2 * sv >= total) bv = min(bv, wv[i]);
                    }
                    ou = bu; ov = bv;
                } else {
                    // ---- 32 rounds, bit 31 down: the weight below prefix | bit, for u and v at once
                    unsigned pu = 0u, pv = 0u;
#pragma unroll 1
                    for (int b = 31; b >= 0; --b) {
                        const unsigned tu = pu | (1u << b), tv = pv | (1u << b);
                        filter_u64 su = 0, sv = 0;
                        if (CACHED) {
#pragma unroll
                            for (int dy = 0; dy < T::D; ++dy) {
#pragma unroll
                                for (int dx = 0; dx < T::D; ++dx) {
                                    const int o = c + (dy - R) * T::LW + (dx - R);
                                    const unsigned wt = w[dy * T::D + dx];
                                    su += ku[o] < tu ? wt : 0u;
                                    sv += kv[o] < tv ? wt : 0u;
                                }
                            }
                        } else {
#pragma unroll 1
                            for (int dy = 0; dy < T::D; ++dy) {
#pragma unroll
                                for (int dx = 0; dx < T::D; ++dx) {
                                    const int o = c + (dy - R) * T::LW + (dx - R);
                                    const unsigned wt = filter_weight(gk[o], cg, stab[dy * T::D + dx], ctab);
                                    su += ku[o] < tu ? wt : 0u;
                                    sv += kv[o] < tv ? wt : 0u;
                                }
                            }
                        }
                        if (2 * su < total) pu = tu;
                        if (2 * sv < total) pv = tv;
                    }
                    ou = pu; ov = pv;
                }
            }
        }
        const size_t p = ((size_t)n * a.H + y) * a.W + x;
        float* o = a.out + p * a.out_cs;
        o[0] = ok ? __uint_as_float(filter_unkey(ou)) : PWC_FLOW_SENTINEL;
        o[1] = ok ? __uint_as_float(filter_unkey(ov)) : PWC_FLOW_SENTINEL;
        a.out_valid[p] = ok ? 1 : 0;
    }
}

// ---------------------------------------------------------------- host
// Whether [p, p + bytes_p) and [q, q + bytes_q) share a byte (sizes as 128-bit numbers: N H W cs 4 may pass 2^64).
static inline bool filter_overlap(const void* p, unsigned __int128 bytes_p, const void* q, unsigned __int128 bytes_q) {
    const unsigned __int128 a0 = reinterpret_cast<uintptr_t>(p), b0 = reinterpret_cast<uintptr_t>(q);
    return a0 < b0 + bytes_q && b0 < a0 + bytes_p;
}

static inline bool filter_in_range(int N, int H, int W) { return (long)H * W < (1L << 31) && N <= 65535; }

extern "C" size_t pwc_flow_filter_workspace_bytes(int N, int H, int W, int iters) {
    if (N < 1 || H < 1 || W < 1 || iters < 2 || !filter_in_range(N, H, W)) return 0;
    const size_t P = (size_t)N * H * W;
    return 8 * P + ((P + 7) & ~(size_t)7);
}

template <int R>
static void filter_launch(const FilterArgs& a, hipStream_t s) {
    const long tiles = (((long)a.W + FILTER_TW - 1) / FILTER_TW) * (((long)a.H + FILTER_TH - 1) / FILTER_TH);
    const dim3 grid((unsigned)(tiles > FILTER_MAX_TILES_X ? FILTER_MAX_TILES_X : tiles), (unsigned)a.N);
    hipLaunchKernelGGL(flow_filter_kernel<R>, grid, dim3(256), 0, s, a);
}

extern "C" int pwc_flow_filter_f32(const float* flows, int flow_cs, const uint8_t* valid, const void* guide, int guide_dtype,
                                   int guide_c, int N, int H, int W, int radius, const uint32_t* space_table,
                                   const uint32_t* color_table, int smooth, int fill, int min_count, int iters, void* workspace,
                                   size_t workspace_bytes, float* out, int out_cs, uint8_t* out_valid, pwc_stream_t stream) {
    if (!flows || !space_table || !out || !out_valid || (guide && !color_table)) return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1) return PWC_EINVAL;
    if (radius < 1 || radius > PWC_FLOW_FILTER_MAX_RADIUS) return PWC_EINVAL;
    if ((guide_c != 1 && guide_c != 3) || (guide_dtype != PWC_FLOW_FILTER_U8 && guide_dtype != PWC_FLOW_FILTER_F32)) return PWC_EINVAL;
    if (!smooth && !fill) return PWC_EINVAL;
    if (min_count < 1 || iters < 1) return PWC_EINVAL;
    if (flow_cs < 2 || out_cs < 2) return PWC_EINVAL;
    const unsigned __int128 P = (unsigned __int128)N * H * W;
    if (filter_overlap(out, P * out_cs * 4, flows, P * flow_cs * 4) || (valid && filter_overlap(out_valid, P, valid, P)))
        return PWC_EINVAL;
    const size_t bytes = pwc_flow_filter_workspace_bytes(N, H, W, iters);
    if (bytes && (!workspace || workspace_bytes < bytes)) return PWC_EINVAL;
    if (!filter_in_range(N, H, W)) return PWC_ERANGE;
    if (pwc_off(flows, 3u) || pwc_off(out, 3u) || pwc_off(space_table, 3u) || (guide && pwc_off(color_table, 3u)) ||
        (guide && guide_dtype == PWC_FLOW_FILTER_F32 && pwc_off(guide, 3u)) || (bytes && pwc_off(workspace, 7u)))
        return PWC_EALIGN;
    FilterArgs a = {};
    a.guide = guide; a.space = space_table; a.color = color_table;
    a.guide_c = guide ? guide_c : 0; a.guide_f32 = guide && guide_dtype == PWC_FLOW_FILTER_F32 ? 1 : 0;
    a.N = N; a.H = H; a.W = W; a.smooth = smooth; a.fill = fill; a.min_count = min_count;
    float* ws_flow = reinterpret_cast<float*>(workspace);
    uint8_t* ws_valid = reinterpret_cast<uint8_t*>(workspace) + 8 * (size_t)N * H * W;
    a.flow = flows; a.flow_cs = flow_cs; a.valid = valid;
    for (int pass = 0; pass < iters; ++pass) {
        const bool to_out = ((iters - 1 - pass) & 1) == 0;                 // the last pass writes out, the others alternate
        a.out = to_out ? out : ws_flow; a.out_cs = to_out ? out_cs : 2; a.out_valid = to_out ? out_valid : ws_valid;
        switch (radius) {
        case 1: filter_launch<1>(a, (hipStream_t)stream); break;
        case 2: filter_launch<2>(a, (hipStream_t)stream); break;
        case 3: filter_launch<3>(a, (hipStream_t)stream); break;
        case 4: filter_launch<4>(a, (hipStream_t)stream); break;
        case 5: filter_launch<5>(a, (hipStream_t)stream); break;
        case 6: filter_launch<6>(a, (hipStream_t)stream); break;
        default: filter_launch<7>(a, (hipStream_t)stream); break;
        }
        a.flow = a.out; a.flow_cs = a.out_cs; a.valid = a.out_valid;
    }
    return pwc_launch_status();
}
