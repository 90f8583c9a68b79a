// pwc_plate.hip -- the background plate of a clip: every frame brought onto one canvas by its matrix and, per canvas pixel and
// channel, the lower median (or the mean) of what the frames show there; and every frame against that plate sampled where the
// frame looks (gfx950; C ABI and the definition in include/pwc_hip.h, "background plate"; the LDS budget, launch geometry and
// resource figures in DESIGN.md 25).
//
//   pwc_plate_build        plate (Hc, Wc, C) in the frames' dtype and count (Hc, Wc) bytes from T frames and T matrices
//   pwc_plate_difference   difference (T, H, W) floats, foreground and known (T, H, W) bytes from the frames, a plate and its count
//
// Build: one lane per canvas pixel, 32 x 8 tiles, tile-stride over min(tiles, 65536) workgroups.  The loop over the frames is
// bounded by T and skips a frame that is not used or whose matrix is not affine -- both uniform in the workgroup.  The mean adds
// in registers.  The median cannot keep 64 samples in registers under a run-time index, so a lane keeps them in the LDS: slot j
// of lane l is dword 256 j + l of T x 256 dwords of dynamic LDS (bank l % 32: conflict-free for every j).  The PRESENT samples
// are stored compacted, slots 0 .. n - 1.  Bytes are one packed dword per sample, all channels gathered once; a float channel is
// 4 bytes per sample, so floats go channel by channel and gather the corners of the present samples again for channels 1 .. C - 1
// (a 64-bit mask in registers says which frames those are).  A lane touches its own slots only: there is no barrier.
// Nothing is sorted: the lower median is the largest K with #{samples < K} <= (n - 1) / 2, built from the top bit down, a round
// per bit over the slots (pwc_flow_filter.hip's selection with unit weights): 8 rounds serve all byte channels at once, a float
// channel takes 32 rounds over its keys.
// Every value is an IEEE double + - x /, a floor, a rint or a comparison in the order of the header -- no fused multiply-add is
// formed anywhere in this file (the pragma below) -- so tests/plate_ref.py restates it in numpy bit for bit.  No atomics, no
// workspace, no scratch, no host synchronisation, no process-wide state; frame offsets are 64-bit.
#include "flow_record.h"
#include "projective.h"

#pragma clang fp contract(off)

#define PLATE_TILE_W 32
#define PLATE_TILE_H 8
#define PLATE_MAX_TILES 65536
#define PLATE_MAX_PIXELS (2147483647L - 65536L)

// WARP's rule (pwc_motion.hip's motion_affine): last row exactly 0 0 1, first two rows finite; e: the matrix (the last row is
// read by the projective branch only).  projective (uniform in the workgroup): projective.h's rule, all nine entries finite.
__device__ __forceinline__ bool plate_affine(const double* m, double* e, int projective) {
    if (projective) return pwc_projective_finite(m, e);
    bool good = m[6] == 0.0 && m[7] == 0.0 && m[8] == 1.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) { e[j] = m[j]; good = good && pwc_finite(e[j]); }
    e[6] = 0.0; e[7] = 0.0; e[8] = 1.0;
    return good;
}

// pwc_flow_filter.hip's total order: negative floats reversed below the positive ones, -0 < +0.
__device__ __forceinline__ unsigned plate_key(unsigned b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ unsigned plate_unkey(unsigned k) { return (k >> 31) ? (k ^ 0x80000000u) : ~k; }

// Where pixel (x, y) lands in an H x W image under the affine rows m, as the four clamped corners (pixel offsets inside the
// image) and their weights; false where the position is outside [0, W - 1] x [0, H - 1] (every comparison is false for a NaN) --
// which is what keeps the corner reads inside the image.
typedef PwcBilinearF64 PlateCorners;
__device__ __forceinline__ bool plate_corners(const double* m, int px, int py, int H, int W, PlateCorners& k, int projective) {
    const double x = (double)px, y = (double)py;
    double sx, sy;
    if (projective) {                                                      // (uniform in the workgroup)
        if (!pwc_projective_position(m, x, y, sx, sy)) return false;
    } else {
        sx = ((m[0] * x) + (m[1] * y)) + m[2]; sy = ((m[3] * x) + (m[4] * y)) + m[5];
    }
    if (!(sx >= 0.0 && sx <= (double)(W - 1) && sy >= 0.0 && sy <= (double)(H - 1))) return false;
    k = pwc_bilinear_f64(sx, sy, H, W);
    return true;
}

// Channel c of the four corners of image `img` (its first pixel's index) as doubles, blended; *fin: all four are finite.
template <bool U8>
__device__ __forceinline__ double plate_blend(const void* base, size_t img, int C, int c, const PlateCorners& k, bool* fin) {
    double c00, c01, c10, c11;
    if (U8) {
        const uint8_t* f = reinterpret_cast<const uint8_t*>(base);
        c00 = (double)f[(img + k.o00) * C + c]; c01 = (double)f[(img + k.o01) * C + c];
        c10 = (double)f[(img + k.o10) * C + c]; c11 = (double)f[(img + k.o11) * C + c];
    } else {
        const float* f = reinterpret_cast<const float*>(base);
        const float f00 = f[(img + k.o00) * C + c], f01 = f[(img + k.o01) * C + c];
        const float f10 = f[(img + k.o10) * C + c], f11 = f[(img + k.o11) * C + c];
        *fin = *fin && pwc_finite(f00) && pwc_finite(f01) && pwc_finite(f10) && pwc_finite(f11);
        c00 = (double)f00; c01 = (double)f01; c10 = (double)f10; c11 = (double)f11;
    }
    const double top = (k.wx0 * c00) + (k.wx1 * c01), bot = (k.wx0 * c10) + (k.wx1 * c11);
    return (k.wy0 * top) + (k.wy1 * bot);
}

// ---------------------------------------------------------------- the plate
struct PlateBuildArgs {
    const void* frames;       // [T][H][W][C] bytes or floats, dense
    const double* matrices;   // [T][9]: a CANVAS pixel to its position in frame t
    const uint8_t* use;       // [T], null: every frame
    const uint8_t* masks;     // [T][H][W], null: every pixel
    void* plate;              // [Hc][Wc][C]
    uint8_t* count;           // [Hc][Wc]
    int T, H, W, Hc, Wc, min_count;
    int projective;           // the matrices are projective (projective.h); 0: affine, the last row exactly 0 0 1
};

template <bool U8, int C>
__device__ __forceinline__ void plate_store(const PlateBuildArgs& a, size_t o, int c, double v, bool keep) {
    if (U8) reinterpret_cast<uint8_t*>(a.plate)[o * C + c] = keep ? (uint8_t)pwc_round_byte(v) : (uint8_t)0;
    else reinterpret_cast<float*>(a.plate)[o * C + c] = keep ? (float)v : 0.f;
}

template <bool U8, int C, bool MEAN>
__global__ __launch_bounds__(256) void plate_build_kernel(const PlateBuildArgs a) {
    extern __shared__ unsigned plate_slots[];                              // [T][256], the median's; none for the mean
    const int tiles_x = (a.Wc + PLATE_TILE_W - 1) / PLATE_TILE_W;
    const int tiles = tiles_x * ((a.Hc + PLATE_TILE_H - 1) / PLATE_TILE_H);
    const int lx = threadIdx.x & (PLATE_TILE_W - 1), ly = threadIdx.x / PLATE_TILE_W;
    const size_t plane = (size_t)a.H * a.W;
    unsigned* mine = plate_slots + threadIdx.x;                            // slot j: mine[256 j]
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty = tile / tiles_x;
        const int px = (tile - ty * tiles_x) * PLATE_TILE_W + lx, py = ty * PLATE_TILE_H + ly;
        if (px >= a.Wc || py >= a.Hc) continue;                            // (no barrier anywhere below)
        // ---- the samples, in frame order
        unsigned long long present = 0ull;                                 // floats: the frames whose sample is PRESENT
        int n = 0, used = 0;                                               // used: frames that pass the uniform conditions, >= n
        double acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0;
        for (int t = 0; t < a.T; ++t) {
            double m[9];
            if ((a.use && !a.use[t]) || !plate_affine(a.matrices + 9 * t, m, a.projective)) continue;     // (uniform in the workgroup)
            ++used;
            PlateCorners k;
            if (!plate_corners(m, px, py, a.H, a.W, k, a.projective)) continue;
            const size_t img = (size_t)t * plane;
            if (a.masks) {
                const uint8_t* mk = a.masks + img;
                if (!(mk[k.o00] && mk[k.o01] && mk[k.o10] && mk[k.o11])) continue;
            }
            double v[C];
            bool fin = true;
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = plate_blend<U8>(a.frames, img, C, c, k, &fin);
            if (!fin) continue;
            if (MEAN) {
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = acc[c] + v[c];
            } else if (U8) {
                unsigned w = 0u;
#pragma unroll
                for (int c = 0; c < C; ++c) w |= pwc_round_byte(v[c]) << (8 * c);
                mine[256 * n] = w;
            } else {
                present |= 1ull << t;
                mine[256 * n] = plate_key(__float_as_uint((float)v[0]));
            }
            ++n;
        }
        const size_t o = (size_t)py * a.Wc + px;
        const bool keep = n >= a.min_count;                                // (min_count >= 1: n = 0 is never kept)
        const int rank = (n - 1) / 2;
        a.count[o] = (uint8_t)n;
        if (MEAN) {
#pragma unroll
            for (int c = 0; c < C; ++c) plate_store<U8, C>(a, o, c, acc[c] / (double)n, keep);
        } else if (U8) {
            // ---- 8 rounds, bit 7 down, every channel in each: the samples below prefix | bit
            unsigned p[C];
#pragma unroll
            for (int c = 0; c < C; ++c) p[c] = 0u;
#pragma unroll 1
            for (int b = 7; b >= 0; --b) {
                int below[C];
#pragma unroll
                for (int c = 0; c < C; ++c) below[c] = 0;
                for (int j = 0; j < used; ++j) {
                    const unsigned w = mine[256 * j];
                    const bool live = j < n;
#pragma unroll
                    for (int c = 0; c < C; ++c) below[c] += (live && ((w >> (8 * c)) & 255u) < (p[c] | (1u << b))) ? 1 : 0;
                }
#pragma unroll
                for (int c = 0; c < C; ++c)
                    if (below[c] <= rank) p[c] |= 1u << b;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) reinterpret_cast<uint8_t*>(a.plate)[o * C + c] = keep ? (uint8_t)p[c] : (uint8_t)0;
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (c > 0) {                                               // this channel of the PRESENT samples, gathered again
                    int j = 0;
                    for (int t = 0; t < a.T; ++t) {
                        if (!((present >> t) & 1ull)) continue;
                        double m[9];
                        PlateCorners k;
                        bool fin = true;
                        plate_affine(a.matrices + 9 * t, m, a.projective);
                        plate_corners(m, px, py, a.H, a.W, k, a.projective);   // (true: the sample is PRESENT)
                        const double v = plate_blend<false>(a.frames, (size_t)t * plane, C, c, k, &fin);
                        mine[256 * j] = plate_key(__float_as_uint((float)v));
                        ++j;
                    }
                }
                // ---- 32 rounds, bit 31 down: the keys below prefix | bit
                unsigned p = 0u;
#pragma unroll 1
                for (int b = 31; b >= 0; --b) {
                    const unsigned bound = p | (1u << b);
                    int below = 0;
                    for (int j = 0; j < used; ++j) below += (j < n && mine[256 * j] < bound) ? 1 : 0;
                    if (below <= rank) p = bound;
                }
                reinterpret_cast<float*>(a.plate)[o * C + c] = keep ? __uint_as_float(plate_unkey(p)) : 0.f;
            }
        }
    }
}

// ---------------------------------------------------------------- the difference
struct PlateDiffArgs {
    const void* frames;       // [T][H][W][C]
    const void* plate;        // [Hc][Wc][C]
    const uint8_t* count;     // [Hc][Wc]
    const double* matrices;   // [T][9]: a FRAME pixel to its position on the canvas
    float* difference;        // [T][H][W]
    uint8_t* foreground;      // [T][H][W]
    uint8_t* known;           // [T][H][W]
    double threshold;
    int T, H, W, Hc, Wc, min_count;
    int projective;           // the matrices are projective (projective.h); 0: affine, the last row exactly 0 0 1
};

template <bool U8, int C>
__global__ __launch_bounds__(256) void plate_difference_kernel(const PlateDiffArgs a) {
    const long plane = (long)a.H * a.W, total = plane * a.T;
    for (long g = blockIdx.x * 256L + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
        const int t = (int)(g / plane);
        const long r = g - (long)t * plane;
        const int y = (int)(r / a.W), x = (int)(r - (long)y * a.W);
        double m[9], d = 0.0;
        PlateCorners k;
        bool ok = plate_affine(a.matrices + 9 * t, m, a.projective) && plate_corners(m, x, y, a.Hc, a.Wc, k, a.projective);
        ok = ok && (int)a.count[k.o00] >= a.min_count && (int)a.count[k.o01] >= a.min_count && (int)a.count[k.o10] >= a.min_count &&
             (int)a.count[k.o11] >= a.min_count;
        if (ok) {
            bool fin = true;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                double f;
                if (U8) {
                    f = (double)reinterpret_cast<const uint8_t*>(a.frames)[(size_t)g * C + c];
                } else {
                    const float fv = reinterpret_cast<const float*>(a.frames)[(size_t)g * C + c];
                    fin = fin && pwc_finite(fv);
                    f = (double)fv;
                }
                const double s = plate_blend<U8>(a.plate, 0, C, c, k, &fin);
                const double e = fabs(f - s);
                if (e > d) d = e;
            }
            ok = fin;
        }
        a.difference[g] = ok ? (float)d : 0.f;
        a.foreground[g] = (ok && d > a.threshold) ? 1 : 0;
        a.known[g] = ok ? 1 : 0;
    }
}

// ---------------------------------------------------------------- host
template <bool U8, int C>
static void plate_build_launch(int mean, dim3 grid, size_t lds, hipStream_t s, const PlateBuildArgs& a) {
    if (mean) hipLaunchKernelGGL((plate_build_kernel<U8, C, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((plate_build_kernel<U8, C, false>), grid, dim3(256), lds, s, a);
}

template <bool U8>
static void plate_build_channels(int C, int mean, dim3 grid, size_t lds, hipStream_t s, const PlateBuildArgs& a) {
    if (C == 1) plate_build_launch<U8, 1>(mean, grid, lds, s, a);
    else if (C == 2) plate_build_launch<U8, 2>(mean, grid, lds, s, a);
    else if (C == 3) plate_build_launch<U8, 3>(mean, grid, lds, s, a);
    else plate_build_launch<U8, 4>(mean, grid, lds, s, a);
}

static int plate_build_call(const void* frames, int dtype, int C, const double* matrices, const uint8_t* use, const uint8_t* masks,
                            int T, int H, int W, int Hc, int Wc, int mode, int min_count, void* plate, uint8_t* count, int projective,
                            pwc_stream_t stream) {
    if (!frames || !matrices || !plate || !count) return PWC_EINVAL;
    if (T < 1 || H < 1 || W < 1 || Hc < 1 || Wc < 1 || T > PWC_PLATE_MAX_FRAMES || C < 1 || C > 4) return PWC_EINVAL;
    if ((dtype != PWC_MOTION_U8 && dtype != PWC_MOTION_F32) || (mode != PWC_PLATE_MEDIAN && mode != PWC_PLATE_MEAN) || min_count < 1)
        return PWC_EINVAL;
    if ((long)H * W > PLATE_MAX_PIXELS || (long)Hc * Wc > PLATE_MAX_PIXELS) return PWC_ERANGE;
    const bool u8 = dtype == PWC_MOTION_U8;
    if (pwc_off(matrices, 7u) || (!u8 && (pwc_off(frames, 3u) || pwc_off(plate, 3u)))) return PWC_EALIGN;
    PlateBuildArgs a = {};
    a.frames = frames; a.matrices = matrices; a.use = use; a.masks = masks; a.plate = plate; a.count = count;
    a.T = T; a.H = H; a.W = W; a.Hc = Hc; a.Wc = Wc; a.min_count = min_count; a.projective = projective;
    const long tiles = (((long)Wc + PLATE_TILE_W - 1) / PLATE_TILE_W) * (((long)Hc + PLATE_TILE_H - 1) / PLATE_TILE_H);
    const dim3 grid((unsigned)(tiles > PLATE_MAX_TILES ? PLATE_MAX_TILES : tiles));
    const size_t lds = (size_t)T * 256 * sizeof(unsigned);                 // <= 64 KB
    if (u8) plate_build_channels<true>(C, mode == PWC_PLATE_MEAN, grid, lds, (hipStream_t)stream, a);
    else plate_build_channels<false>(C, mode == PWC_PLATE_MEAN, grid, lds, (hipStream_t)stream, a);
    return pwc_launch_status();
}

extern "C" int pwc_plate_build(const void* frames, int dtype, int C, const double* matrices, const uint8_t* use, const uint8_t* masks,
                               int T, int H, int W, int Hc, int Wc, int mode, int min_count, void* plate, uint8_t* count,
                               pwc_stream_t stream) {
    return plate_build_call(frames, dtype, C, matrices, use, masks, T, H, W, Hc, Wc, mode, min_count, plate, count, 0, stream);
}

extern "C" int pwc_plate_build_projective(const void* frames, int dtype, int C, const double* matrices, const uint8_t* use,
                                          const uint8_t* masks, int T, int H, int W, int Hc, int Wc, int mode, int min_count, void* plate,
                                          uint8_t* count, pwc_stream_t stream) {
    return plate_build_call(frames, dtype, C, matrices, use, masks, T, H, W, Hc, Wc, mode, min_count, plate, count, 1, stream);
}

template <bool U8>
static void plate_difference_launch(int C, dim3 grid, hipStream_t s, const PlateDiffArgs& a) {
    if (C == 1) hipLaunchKernelGGL((plate_difference_kernel<U8, 1>), grid, dim3(256), 0, s, a);
    else if (C == 2) hipLaunchKernelGGL((plate_difference_kernel<U8, 2>), grid, dim3(256), 0, s, a);
    else if (C == 3) hipLaunchKernelGGL((plate_difference_kernel<U8, 3>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((plate_difference_kernel<U8, 4>), grid, dim3(256), 0, s, a);
}

static int plate_difference_call(const void* frames, int dtype, int C, const void* plate, const uint8_t* count,
                                 const double* matrices, int T, int H, int W, int Hc, int Wc, int min_count, double threshold,
                                 float* difference, uint8_t* foreground, uint8_t* known, int projective, pwc_stream_t stream) {
    if (!frames || !plate || !count || !matrices || !difference || !foreground || !known) return PWC_EINVAL;
    if (T < 1 || H < 1 || W < 1 || Hc < 1 || Wc < 1 || C < 1 || C > 4) return PWC_EINVAL;
    if ((dtype != PWC_MOTION_U8 && dtype != PWC_MOTION_F32) || min_count < 1 || !(threshold >= 0.0)) return PWC_EINVAL;
    if ((long)H * W > PLATE_MAX_PIXELS || (long)Hc * Wc > PLATE_MAX_PIXELS || T > 65535) return PWC_ERANGE;
    const bool u8 = dtype == PWC_MOTION_U8;
    if (pwc_off(matrices, 7u) || pwc_off(difference, 3u) || (!u8 && (pwc_off(frames, 3u) || pwc_off(plate, 3u))))
        return PWC_EALIGN;
    PlateDiffArgs a = {};
    a.frames = frames; a.plate = plate; a.count = count; a.matrices = matrices; a.difference = difference;
    a.foreground = foreground; a.known = known; a.threshold = threshold;
    a.T = T; a.H = H; a.W = W; a.Hc = Hc; a.Wc = Wc; a.min_count = min_count; a.projective = projective;
    const dim3 grid = pwc_flat_grid((long)T * H * W);
    if (u8) plate_difference_launch<true>(C, grid, (hipStream_t)stream, a);
    else plate_difference_launch<false>(C, grid, (hipStream_t)stream, a);
    return pwc_launch_status();
}

extern "C" int pwc_plate_difference(const void* frames, int dtype, int C, const void* plate, const uint8_t* count,
                                    const double* matrices, int T, int H, int W, int Hc, int Wc, int min_count, double threshold,
                                    float* difference, uint8_t* foreground, uint8_t* known, pwc_stream_t stream) {
    return plate_difference_call(frames, dtype, C, plate, count, matrices, T, H, W, Hc, Wc, min_count, threshold, difference, foreground,
                                 known, 0, stream);
}

extern "C" int pwc_plate_difference_projective(const void* frames, int dtype, int C, const void* plate, const uint8_t* count,
                                               const double* matrices, int T, int H, int W, int Hc, int Wc, int min_count,
                                               double threshold, float* difference, uint8_t* foreground, uint8_t* known,
                                               pwc_stream_t stream) {
    return plate_difference_call(frames, dtype, C, plate, count, matrices, T, H, W, Hc, Wc, min_count, threshold, difference, foreground,
                                 known, 1, stream);
}
