// pwc_pyramid.hip -- block-mean pyramids of frames and block-count pyramids of masks, every requested level from ONE launch
// (gfx950; C ABI in include/pwc_hip.h, "frame and mask pyramids").  What multi-scale label-free training needs in front of the
// data terms: the frames at every level of flows_pyramid, and the occlusion masks pooled to the same sizes.
//
//   pwc_frame_pyramid_f32   out_f[n, y, x, c] = the mean of the f x f block of x, summed in double, rounded to float32 once
//   pwc_mask_pyramid_u8     out_f[n, y, x]    = (number of non-zero bytes of the f x f block) >= need_f, the count on request
//
// One kernel template serves both.  A workgroup of 256 lanes owns a tile fmax rows high and kb * fmax pixels wide (fmax the largest
// factor asked for), so every cell of every level lies inside one workgroup and every input element is read from memory once:
//   1. registers: a lane owns a span of max(F0, UNIT) pixels of F0 consecutive rows (F0 the SMALLEST factor asked for) and sums
//      each F0 x F0 cell per channel, rows top to bottom, pixels left to right.  A UNIT is the piece of a row that is loaded at
//      once: 16 pixels of bytes, 4 pixels of floats -- C loads of 16 bytes, whatever C is, and the channel and cell of every
//      element of it are compile-time constants.  The host checks the base, the row pitch and the unit size and hands down the
//      load width (16, 4 or 1 bytes): nothing is assumed.  Frames narrower than a unit (fmax < UNIT) take the variant UNIT = F0.
//   2. LDS: the F0-level sums go to LDS as doubles (ints for masks); every further level is the sum of the 2 x 2 cells of the
//      level below, ((a + b) + c) + d with a, b the upper pair, between two buffers; a level that was asked for is written out
//      on the way, a level that was not is only passed through.
// The order of every sum is fixed by the cell alone -- not by N, the tile width, the load width or the workgroup -- so two calls
// give the same bits.  For byte frames the sums are exact in double, so any order would do.  No atomics, no
// status word: a NaN or an Inf makes the cells that contain it non-finite by plain arithmetic.
#include <type_traits>

#include "pwc_common.h"

namespace {

// level k is factor 2 << k: 2, 4, 8, 16, 32, 64
#define PYR_LEVELS 6

struct PyrArgs {
    const void* x;
    void* out[PYR_LEVELS];    // float* (frames) or uint8_t* (masks); null: the level is not asked for
    int* cnt[PYR_LEVELS];     // masks: the counts, null: not asked for
    int need[PYR_LEVELS];     // masks: out = count >= need
    int N, H, W;
    int kmax;                 // the level of the largest factor
    int kb;                   // blocks of fmax x fmax pixels per tile, along x
    int tiles_x;              // tiles per row of blocks
    int vec;                  // bytes per load: 16, 4 or 1
};

typedef unsigned pyr_u32x4 __attribute__((ext_vector_type(4)));

// UE consecutive elements at p.  vec is what the host found the base, the pitch and the unit size to allow.
template <typename T, int UE>
__device__ __forceinline__ void pyr_load(const T* __restrict__ p, int vec, T (&v)[UE]) {
    constexpr int BYTES = UE * (int)sizeof(T);
    if constexpr (BYTES % 16 == 0) {
        if (vec == 16) {
            pyr_u32x4 w[BYTES / 16];
#pragma unroll
            for (int i = 0; i < BYTES / 16; ++i) w[i] = reinterpret_cast<const pyr_u32x4*>(p)[i];
            __builtin_memcpy(v, w, BYTES);
            return;
        }
    }
    if constexpr (BYTES % 4 == 0 && sizeof(T) == 1) {
        if (vec >= 4) {
            unsigned w[BYTES / 4];
#pragma unroll
            for (int i = 0; i < BYTES / 4; ++i) w[i] = reinterpret_cast<const unsigned*>(p)[i];
            __builtin_memcpy(v, w, BYTES);
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < UE; ++i) v[i] = p[i];
}

// What one element adds to its cell.  A byte of a frame enters as the float32 nearest v / 255, pwc_fit.hip's fit_value.
template <bool MASK>
__device__ __forceinline__ auto pyr_value(float v) { return (double)v; }
template <bool MASK>
__device__ __forceinline__ auto pyr_value(uint8_t v) {
    if constexpr (MASK) return v ? 1 : 0;
    else return (double)(float)((double)v * (1.0 / 255.0));
}

// One cell of level k (K a compile-time constant at every call) at flat output index o.
template <bool MASK, typename Acc>
__device__ __forceinline__ void pyr_emit(const PyrArgs& a, int k, size_t o, Acc v) {
    if constexpr (MASK) {
        if (a.out[k]) static_cast<uint8_t*>(a.out[k])[o] = v >= a.need[k] ? 1 : 0;
        if (a.cnt[k]) a.cnt[k][o] = v;
    } else {
        // (a power of two: the scaling is exact, the conversion is the one rounding)
        if (a.out[k]) static_cast<float*>(a.out[k])[o] = (float)(v * (1.0 / (double)(1 << (2 * (k + 1)))));
    }
}

template <typename T, int C, int F0, int UNIT, bool MASK>
__global__ __launch_bounds__(256) void pyramid_kernel(const PyrArgs a) {
    using Acc = typename std::conditional<MASK, int, double>::type;
    extern __shared__ double pyr_lds[];
    Acc* lds = reinterpret_cast<Acc*>(pyr_lds);
    constexpr int CELLS = UNIT > F0 ? UNIT / F0 : 1;      // F0-cells of a span, along x
    constexpr int UNITS = F0 > UNIT ? F0 / UNIT : 1;      // units of a span row
    constexpr int SPAN = F0 * CELLS;                      // pixels
    constexpr int UE = UNIT * C;                          // elements of a unit
    constexpr int ROWS_AHEAD = UNITS == 1 ? 4 : 1;        // rows of a span whose loads are issued together
    constexpr int K0 = F0 == 2 ? 0 : F0 == 4 ? 1 : F0 == 8 ? 2 : F0 == 16 ? 3 : F0 == 32 ? 4 : 5;
    static_assert((2 << K0) == F0 && SPAN == (F0 > UNIT ? F0 : UNIT), "F0 and UNIT are powers of two");

    const int fmax = 2 << a.kmax;
    const int bw = a.W / fmax, bh = a.H / fmax;
    int b = blockIdx.x;
    const int tx = b % a.tiles_x;
    b /= a.tiles_x;
    const int by = b % bh, n = b / bh;
    const int blk0 = tx * a.kb;
    const int tw = min(a.kb, bw - blk0) * fmax;           // the tile's width, pixels
    const int R0 = fmax / F0, C0 = tw / F0;               // its F0-cells
    const int spans = tw / SPAN, items = R0 * spans;
    const size_t pitch = (size_t)a.W * C;
    const T* base = static_cast<const T*>(a.x) + ((size_t)n * a.H + (size_t)by * fmax) * pitch + (size_t)blk0 * fmax * C;

    for (int item = threadIdx.x; item < items; item += 256) {
        const int r = item / spans, s = item - r * spans;
        Acc acc[CELLS * C];
#pragma unroll
        for (int i = 0; i < CELLS * C; ++i) acc[i] = 0;
        const T* p = base + (size_t)r * F0 * pitch + (size_t)s * SPAN * C;
#pragma unroll ROWS_AHEAD
        for (int dy = 0; dy < F0; ++dy, p += pitch) {
#pragma unroll
            for (int u = 0; u < UNITS; ++u) {
                T v[UE];
                pyr_load<T, UE>(p + u * UE, a.vec, v);
#pragma unroll
                for (int e = 0; e < UE; ++e) acc[(CELLS > 1 ? (e / C) / F0 : 0) * C + e % C] += pyr_value<MASK>(v[e]);
            }
        }
        const size_t o = (((size_t)n * (a.H / F0) + (size_t)by * R0 + r) * (a.W / F0) + (size_t)blk0 * R0 + s * CELLS) * C;
        Acc* l = lds + (r * C0 + s * CELLS) * C;
#pragma unroll
        for (int i = 0; i < CELLS * C; ++i) {
            pyr_emit<MASK>(a, K0, o + i, acc[i]);
            if (a.kmax > K0) l[i] = acc[i];
        }
    }
    if (a.kmax == K0) return;                             // (uniform: one level, nothing goes through LDS)
    __syncthreads();

    Acc* src = lds;
    Acc* dst = lds + R0 * (a.kb * R0) * C;                // behind the F0 level of a full tile
    int Rk = R0, Ck = C0;
#pragma unroll
    for (int k = K0 + 1; k < PYR_LEVELS; ++k) {
        if (k > a.kmax) break;                            // (uniform)
        const int Rn = Rk >> 1, Cn = Ck >> 1, cells = Rn * Cn * C;
        const int rb = fmax >> (k + 1);                   // cells of this level per block, each way
        for (int i = threadIdx.x; i < cells; i += 256) {
            const int ch = i % C, q = i / C;
            const int col = q % Cn, row = q / Cn;
            const Acc* s0 = src + ((2 * row) * Ck + 2 * col) * C + ch;
            const Acc v = ((s0[0] + s0[C]) + s0[Ck * C]) + s0[Ck * C + C];
            dst[i] = v;
            pyr_emit<MASK>(a, k, (((size_t)n * (a.H >> (k + 1)) + (size_t)by * rb + row) * (a.W >> (k + 1)) + (size_t)blk0 * rb + col) * C + ch, v);
        }
        __syncthreads();
        Acc* t = src;
        src = dst;
        dst = t;
        Rk = Rn;
        Ck = Cn;
    }
}

// The widest unit of each element type: 16 pixels of bytes, 4 pixels of floats (C loads of 16 bytes).
template <typename T>
constexpr int pyr_unit() { return sizeof(T) == 1 ? 16 : 4; }

struct PyrPlan {
    int narrow;               // fmax is below the unit: UNIT = F0
    int vec, kb, tiles_x;
    unsigned grid;
    size_t lds;
};

// LDS of a tile of kb blocks: the F0 level and, behind it, a quarter of that for the level above.
inline size_t pyr_lds_bytes(int cells_per_block, int kb, int acc_size, bool coarser) {
    return coarser ? ((size_t)cells_per_block * kb + (size_t)cells_per_block * kb / 4) * acc_size : 0;
}

// The tile and the load width.  The tile is as many blocks wide as keep 256 lanes busy in step 1, fewer where the LDS would
// pass 40 KiB or the launch would have fewer than two workgroups per compute unit.  None of this changes a bit of the result.
int pyr_plan(const void* x, int esize, int acc_size, int N, int H, int W, int C, int k0, int kmax, PyrPlan* p) {
    const int f0 = 2 << k0, fmax = 2 << kmax, unit_std = esize == 1 ? 16 : 4;
    p->narrow = fmax < unit_std;
    const int unit = p->narrow ? f0 : unit_std;
    const int span = f0 > unit ? f0 : unit;
    const size_t probe = reinterpret_cast<uintptr_t>(x) | ((size_t)W * C * esize) | ((size_t)unit * C * esize);
    p->vec = (probe & 15u) == 0 ? 16 : (probe & 3u) == 0 ? 4 : 1;
    const int per_block = (fmax / f0) * (fmax / span);
    const int cells = (fmax / f0) * (fmax / f0) * C;
    const int bw = W / fmax;
    int kb = (256 + per_block - 1) / per_block;
    kb = kb > 8 ? 8 : kb;
    kb = kb > bw ? bw : kb;
    while (kb > 1 && pyr_lds_bytes(cells, kb, acc_size, kmax > k0) > 40960) --kb;
    const long long rows = (long long)N * (H / fmax);
    while (kb > 1 && rows * ((bw + kb - 1) / kb) < 2ll * pwc_cu_count()) kb = (kb + 1) / 2;
    const long long tiles = rows * ((bw + kb - 1) / kb);
    if (tiles >= (1ll << 31)) return PWC_ERANGE;
    p->kb = kb;
    p->tiles_x = (bw + kb - 1) / kb;
    p->grid = (unsigned)tiles;
    p->lds = pyr_lds_bytes(cells, kb, acc_size, kmax > k0);
    return PWC_OK;
}

template <typename T, int C, int F0, bool MASK>
void pyr_launch_f0(const PyrPlan& p, hipStream_t s, const PyrArgs& a) {
    if constexpr (F0 < pyr_unit<T>()) {
        if (p.narrow) {
            hipLaunchKernelGGL((pyramid_kernel<T, C, F0, F0, MASK>), dim3(p.grid), dim3(256), p.lds, s, a);
            return;
        }
    }
    hipLaunchKernelGGL((pyramid_kernel<T, C, F0, pyr_unit<T>(), MASK>), dim3(p.grid), dim3(256), p.lds, s, a);
}

template <typename T, int C, bool MASK>
void pyr_launch_c(int k0, const PyrPlan& p, hipStream_t s, const PyrArgs& a) {
    switch (k0) {
        case 0: pyr_launch_f0<T, C, 2, MASK>(p, s, a); break;
        case 1: pyr_launch_f0<T, C, 4, MASK>(p, s, a); break;
        case 2: pyr_launch_f0<T, C, 8, MASK>(p, s, a); break;
        case 3: pyr_launch_f0<T, C, 16, MASK>(p, s, a); break;
        case 4: pyr_launch_f0<T, C, 32, MASK>(p, s, a); break;
        default: pyr_launch_f0<T, C, 64, MASK>(p, s, a); break;
    }
}

template <typename T>
void pyr_launch_frames(int C, int k0, const PyrPlan& p, hipStream_t s, const PyrArgs& a) {
    switch (C) {
        case 1: pyr_launch_c<T, 1, false>(k0, p, s, a); break;
        case 2: pyr_launch_c<T, 2, false>(k0, p, s, a); break;
        case 3: pyr_launch_c<T, 3, false>(k0, p, s, a); break;
        default: pyr_launch_c<T, 4, false>(k0, p, s, a); break;
    }
}

// The factors of a call: each one of 2 .. 64 and a power of two (PWC_EUNSUPPORTED), none twice (PWC_EINVAL); level[i] of
// factors[i], the smallest and the largest level.
int pyr_factors(const int* factors, int n_levels, int* level, int* k0, int* kmax) {
    if (!factors || n_levels < 1 || n_levels > PYR_LEVELS) return PWC_EINVAL;
    unsigned seen = 0;
    *k0 = PYR_LEVELS;
    *kmax = -1;
    for (int i = 0; i < n_levels; ++i) {
        int k = -1;
        for (int j = 0; j < PYR_LEVELS; ++j)
            if (factors[i] == (2 << j)) k = j;
        if (k < 0) return PWC_EUNSUPPORTED;
        if (seen & (1u << k)) return PWC_EINVAL;
        seen |= 1u << k;
        level[i] = k;
        *k0 = k < *k0 ? k : *k0;
        *kmax = k > *kmax ? k : *kmax;
    }
    return PWC_OK;
}

inline bool pyr_off4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

}  // namespace

extern "C" int pwc_frame_pyramid_f32(const void* x, int x_is_u8, int N, int H, int W, int C, const int* factors, float* const* outs,
                                     int n_levels, pwc_stream_t stream) {
    if (!x || !outs || N <= 0 || H <= 0 || W <= 0) return PWC_EINVAL;
    if (C < 1 || C > 4) return PWC_EUNSUPPORTED;
    int level[PYR_LEVELS], k0, kmax;
    int rc = pyr_factors(factors, n_levels, level, &k0, &kmax);
    if (rc != PWC_OK) return rc;
    if (H % (2 << kmax) || W % (2 << kmax)) return PWC_EINVAL;
    PyrArgs a = {};
    for (int i = 0; i < n_levels; ++i) {
        if (!outs[i]) return PWC_EINVAL;
        a.out[level[i]] = outs[i];
    }
    if (!x_is_u8 && pyr_off4(x)) return PWC_EALIGN;
    for (int i = 0; i < n_levels; ++i)
        if (pyr_off4(outs[i])) return PWC_EALIGN;
    if ((long long)N * H * W * C >= (1ll << 31)) return PWC_ERANGE;
    PyrPlan p;
    rc = pyr_plan(x, x_is_u8 ? 1 : 4, (int)sizeof(double), N, H, W, C, k0, kmax, &p);
    if (rc != PWC_OK) return rc;
    a.x = x; a.N = N; a.H = H; a.W = W; a.kmax = kmax; a.kb = p.kb; a.tiles_x = p.tiles_x; a.vec = p.vec;
    if (x_is_u8) pyr_launch_frames<uint8_t>(C, k0, p, (hipStream_t)stream, a);
    else pyr_launch_frames<float>(C, k0, p, (hipStream_t)stream, a);
    return pwc_launch_status();
}

extern "C" int pwc_mask_pyramid_u8(const unsigned char* valid, int N, int H, int W, const int* factors, const int* need,
                                   unsigned char* const* outs, int* const* counts, int n_levels, pwc_stream_t stream) {
    if (!valid || !outs || !need || N <= 0 || H <= 0 || W <= 0) return PWC_EINVAL;
    int level[PYR_LEVELS], k0, kmax;
    int rc = pyr_factors(factors, n_levels, level, &k0, &kmax);
    if (rc != PWC_OK) return rc;
    if (H % (2 << kmax) || W % (2 << kmax)) return PWC_EINVAL;
    PyrArgs a = {};
    for (int i = 0; i < n_levels; ++i) {
        if (!outs[i] || need[i] < 1 || need[i] > factors[i] * factors[i]) return PWC_EINVAL;
        a.out[level[i]] = outs[i];
        a.need[level[i]] = need[i];
        a.cnt[level[i]] = counts ? counts[i] : nullptr;
    }
    for (int i = 0; counts && i < n_levels; ++i)
        if (pyr_off4(counts[i])) return PWC_EALIGN;
    if ((long long)N * H * W >= (1ll << 31)) return PWC_ERANGE;
    PyrPlan p;
    rc = pyr_plan(valid, 1, (int)sizeof(int), N, H, W, 1, k0, kmax, &p);
    if (rc != PWC_OK) return rc;
    a.x = valid; a.N = N; a.H = H; a.W = W; a.kmax = kmax; a.kb = p.kb; a.tiles_x = p.tiles_x; a.vec = p.vec;
    pyr_launch_c<uint8_t, 1, true>(k0, p, (hipStream_t)stream, a);
    return pwc_launch_status();
}
