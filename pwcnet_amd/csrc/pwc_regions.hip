// pwc_regions.hip -- moving regions: the connected components of a mask (connectivity 4 or 8, never across images), numbered in
// raster order of their first pixel, with their areas, boxes and -- where a flow is given -- the fixed-point sums and means of
// it (gfx950; C ABI in include/pwc_hip.h, "moving regions"; semantics and launch plan in DESIGN.md 21).
//
//   pwc_regions_tile_h / _w          the tile of the first launch, 32 x 32
//   pwc_regions_workspace_bytes      4 (3 N H W + 2 N parts): the area per root, two label arrays, the scan's parts
//   pwc_label_regions                labels (N, H, W) int32, count (N) int32, area (N, R) int32, box (N, R, 4) int32,
//                                    sums (N, R, 2) int64, mean (N, R, 2) doubles
//
// The result is a function of the input alone: a component's ROOT is its smallest linear index y W + x, whatever the order in
// which lanes join it; areas, boxes and sums are integers added, minimised and maximised with integer atomics, the same in any
// order; the ids come from a prefix count over contiguous chunks of the linear index.  tests/regions_ref.py restates the
// definition (a host union-find, not these launches) and the tests hold every output to its bits.
//
// Ten launches on the caller's stream, each reading what the one before wrote:
//   clear    a lane per table row: area, box, sums zero.
//   tile     grid (tiles, N), a workgroup of 256 lanes labels one 32 x 32 tile in the LDS by union-find (four pixels a lane) and
//            writes every pixel's tile-local root as a linear index of its image into `link`, -1 for background, 0 into `areas`.
//   seam     a lane per pixel of a tile's first row or first column (tiles beyond the first): joins it with its foreground
//            neighbours across the seam -- north, and for connectivity 8 north-west and north-east; west, and for connectivity 8
//            north-west and south-west -- by atomicMin on `link`.  The two diagonal pairs at a tile corner are the north-west of
//            the corner pixel and the south-west of the pixel above it (equally: the north-east of the pixel left of it).
//   flatten  a lane per pixel follows `link` to its root and writes it to `root` (-1 for background); reads `link` only.
//   area     a lane per pixel; the lanes of a wave that hold one root add their number to areas[root] with one atomicAdd.
//   count    grid (parts, N): part b counts the KEPT roots -- root[i] == i, areas[i] >= min_area -- of the pixels
//            [b chunk, (b + 1) chunk), chunk = 256 ceil(H W / (256 parts)), parts = min(ceil(H W / 256), 256).
//   offsets  a lane per image turns the parts' counts into their exclusive prefix and writes count.
//   number   grid (parts, N): part b walks its chunk 256 pixels at a time, in order; a kept root gets id = offset + its rank
//            among the kept roots before it + 1, written over link[root] (0 for a root that is not kept); ids up to max_regions
//            start their table row: the area, and the root's own pixel as the box (the root is the first pixel in raster order:
//            its y is the box's y0).
//   final    a lane per pixel: labels = link[root] (0 for background); ids up to max_regions take x0 by atomicMin, x1 and y1 by
//            atomicMax and add the two fixed-point flow values with 64-bit atomicAdd; the lanes of a wave that hold one id
//            combine them first (__shfl_xor) and issue one set of atomics.
//   mean     a lane per table row: the two divisions.
// No host synchronisation, no process-wide state, no floating-point atomics.
//
// Inter-workgroup visibility (the seam launch is the only one in which workgroups exchange data): `link` is written there by
// other workgroups while it is read, a CU's L1 is never refreshed by another CU's stores and the XCDs' L2s are private, so EVERY
// read of `link` in that kernel is an agent-scope relaxed atomic load (it bypasses the L1) and every write an agent-scope
// atomicMin; there is no plain load of it in that kernel.  A stale value could not break the result's definition anyway -- a
// link only ever moves to a smaller index of the same component -- but it is not relied on.  Between launches the stream's
// order is the hand-off.
// Termination: no loop waits for another lane or workgroup.  A find follows parents to STRICTLY smaller indices and stops at
// the first that is not; a union retries with the value its atomicMin returned, which is strictly smaller than the index it
// was applied to.  Both are bounded by the index they start from.
#include "flow_record.h"

#pragma clang fp contract(off)

#define REGIONS_TH 32
#define REGIONS_TW 32
#define REGIONS_TILE (REGIONS_TH * REGIONS_TW)
#define REGIONS_MAX_PARTS 256
#define REGIONS_MAX_PIXELS (1L << 26)
#define REGIONS_MAX_REGIONS 65535

struct RegionsArgs {
    const uint8_t* mask;      // [N][H][W]
    const float* flow;        // [N][H][W] records of cs floats, 2 used; null: the mask alone
    int* areas;               // [N][H W]: the area of a root at its index
    int* link;                // [N][H W]: parents (tile, seam), then the ids of the roots (number)
    int* root;                // [N][H W]: every pixel's root, -1 for background
    int* part;                // [N][parts]: the kept roots of a part, then their exclusive prefix
    int* labels;              // [N][H W]
    int* count;               // [N]
    int* area;                // [N][R]
    int* box;                 // [N][R][4]
    long long* sums;          // [N][R][2], null with flow
    double* mean;             // [N][R][2], null with flow
    int invert, cs, N, H, W, conn8, min_area, R, parts, chunk, tiles_x, tiles_y;
};

// FOREGROUND: the mask byte (inverted: its absence), and a known flow where one is given; a flow the mask excludes is not loaded.
__device__ __forceinline__ bool regions_foreground(const RegionsArgs& a, size_t g) {
    if ((a.mask[g] != 0) == (a.invert != 0)) return false;
    if (!a.flow) return true;
    const float* f = a.flow + g * a.cs;
    return pwc_flow_known(f[0], f[1]);
}

// ---------------------------------------------------------------- clear
__global__ __launch_bounds__(256) void regions_clear_kernel(const RegionsArgs a) {
    const long r = blockIdx.x * 256L + threadIdx.x;
    if (r >= (long)a.N * a.R) return;
    a.area[r] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) a.box[4 * r + j] = 0;
    if (a.sums) { a.sums[2 * r] = 0; a.sums[2 * r + 1] = 0; }
}

// ---------------------------------------------------------------- tile: union-find in the LDS
#define REGIONS_LDS_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)

__device__ __forceinline__ int regions_lds_find(int* L, int x) {
    // ends by itself: every step goes to a strictly smaller index (0 <= p < x), whatever the other lanes do meanwhile
    for (;;) {
        const int p = REGIONS_LDS_LOAD(L + x);
        if (!(p >= 0 && p < x)) return x;
        x = p;
    }
}

__device__ __forceinline__ void regions_lds_union(int* L, int x, int y) {
    x = regions_lds_find(L, x);
    y = regions_lds_find(L, y);
    // ends by itself: each retry replaces the larger index by the value atomicMin returned, which is strictly smaller than
    // it, so max(x, y) falls every turn; it never waits for a value another lane has yet to write
    while (x != y) {
        if (x < y) { const int t = x; x = y; y = t; }
        const int old = __hip_atomic_fetch_min(L + x, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (!(old >= 0 && old < x)) break;           // x was a root: it hangs under y now
        x = old;                                     // x had a parent already: join that parent and y
    }
}

__global__ __launch_bounds__(256) void regions_tile_kernel(const RegionsArgs a) {
    __shared__ int L[REGIONS_TILE];
    const int t = threadIdx.x, n = blockIdx.y;
    const int y0 = (int)(blockIdx.x / a.tiles_x) * REGIONS_TH, x0 = (int)(blockIdx.x % a.tiles_x) * REGIONS_TW;
    const size_t img = (size_t)n * a.H * a.W;
#pragma unroll
    for (int k = 0; k < REGIONS_TILE / 256; ++k) {
        const int l = k * 256 + t, y = y0 + l / REGIONS_TW, x = x0 + l % REGIONS_TW;
        const bool fg = y < a.H && x < a.W && regions_foreground(a, img + (size_t)y * a.W + x);
        L[l] = fg ? l : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < REGIONS_TILE / 256; ++k) {
        const int l = k * 256 + t, ly = l / REGIONS_TW, lx = l % REGIONS_TW;
        if (REGIONS_LDS_LOAD(L + l) < 0) continue;
        if (lx > 0 && REGIONS_LDS_LOAD(L + l - 1) >= 0) regions_lds_union(L, l, l - 1);
        if (ly > 0 && REGIONS_LDS_LOAD(L + l - REGIONS_TW) >= 0) regions_lds_union(L, l, l - REGIONS_TW);
        if (a.conn8 && ly > 0) {
            if (lx > 0 && REGIONS_LDS_LOAD(L + l - REGIONS_TW - 1) >= 0) regions_lds_union(L, l, l - REGIONS_TW - 1);
            if (lx < REGIONS_TW - 1 && REGIONS_LDS_LOAD(L + l - REGIONS_TW + 1) >= 0) regions_lds_union(L, l, l - REGIONS_TW + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < REGIONS_TILE / 256; ++k) {
        const int l = k * 256 + t, y = y0 + l / REGIONS_TW, x = x0 + l % REGIONS_TW;
        if (y >= a.H || x >= a.W) continue;
        int r = -1;
        if (L[l] >= 0) {
            const int q = regions_lds_find(L, l);
            r = (y0 + q / REGIONS_TW) * a.W + (x0 + q % REGIONS_TW);
        }
        const size_t g = img + (size_t)y * a.W + x;
        a.link[g] = r;
        a.areas[g] = 0;
    }
}

// ---------------------------------------------------------------- seam: union-find across tiles, on the global array
#define REGIONS_AGENT_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__device__ __forceinline__ int regions_seam_find(int* G, int x) {
    // ends by itself: every step goes to a strictly smaller index (0 <= p < x), whatever the other workgroups do meanwhile
    for (;;) {
        const int p = REGIONS_AGENT_LOAD(G + x);
        if (!(p >= 0 && p < x)) return x;
        x = p;
    }
}

__device__ __forceinline__ void regions_seam_union(int* G, int x, int y) {
    x = regions_seam_find(G, x);
    y = regions_seam_find(G, y);
    // ends by itself: each retry replaces the larger index by the value atomicMin returned, which is strictly smaller than
    // it, so max(x, y) falls every turn; it never waits for a value another workgroup has yet to write
    while (x != y) {
        if (x < y) { const int t = x; x = y; y = t; }
        const int old = __hip_atomic_fetch_min(G + x, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!(old >= 0 && old < x)) break;           // x was a root: it hangs under y now
        x = old;                                     // x had a parent already: join that parent and y
    }
}

// Joins pixel i (foreground) with the pixel at (x, y) where that is inside the image and foreground.
__device__ __forceinline__ void regions_seam_join(const RegionsArgs& a, int* G, int i, int x, int y) {
    if (x < 0 || x >= a.W || y < 0 || y >= a.H) return;
    const int j = y * a.W + x;
    if (REGIONS_AGENT_LOAD(G + j) >= 0) regions_seam_union(G, i, j);
}

// Lane l of an image: l < (tiles_y - 1) W is pixel x = l % W of the first row of tile row l / W + 1; the lanes behind are pixel
// y = l' % H of the first column of tile column l' / H + 1.
__global__ __launch_bounds__(256) void regions_seam_kernel(const RegionsArgs a) {
    const int rows = (a.tiles_y - 1) * a.W, cols = (a.tiles_x - 1) * a.H;
    const long l = blockIdx.x * 256L + threadIdx.x;
    if (l >= (long)rows + cols) return;
    int* G = a.link + (size_t)blockIdx.y * a.H * a.W;
    if (l < rows) {
        const int x = (int)(l % a.W), y = ((int)(l / a.W) + 1) * REGIONS_TH, i = y * a.W + x;
        if (REGIONS_AGENT_LOAD(G + i) < 0) return;
        regions_seam_join(a, G, i, x, y - 1);
        if (a.conn8) {
            regions_seam_join(a, G, i, x - 1, y - 1);
            regions_seam_join(a, G, i, x + 1, y - 1);
        }
    } else {
        const int c = (int)(l - rows);
        const int y = c % a.H, x = (c / a.H + 1) * REGIONS_TW, i = y * a.W + x;
        if (REGIONS_AGENT_LOAD(G + i) < 0) return;
        regions_seam_join(a, G, i, x - 1, y);
        if (a.conn8) {
            regions_seam_join(a, G, i, x - 1, y - 1);
            regions_seam_join(a, G, i, x - 1, y + 1);
        }
    }
}

// ---------------------------------------------------------------- flatten, area
__global__ __launch_bounds__(256) void regions_flatten_kernel(const RegionsArgs a) {
    const int hw = a.H * a.W;
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= hw) return;
    const size_t img = (size_t)blockIdx.y * hw;
    const int* G = a.link + img;
    int r = G[i];
    if (r >= 0) {
        // ends by itself: every step goes to a strictly smaller index; nothing writes `link` in this launch
        for (;;) {
            const int p = G[r];
            if (!(p >= 0 && p < r)) break;
            r = p;
        }
    }
    a.root[img + i] = r;
}

// The runs of one key within a wave leave together: a turn takes the key of the first lane that is still waiting, and every
// waiting lane that holds it is combined and retired, one atomic for all of them.  Ends by itself: a turn retires at least the
// lane whose key it took, so there are at most 64 turns (one per distinct key of the wave); the lanes of a wave run in lockstep
// and the loop's condition is wave-uniform -- nothing is waited for.
__global__ __launch_bounds__(256) void regions_area_kernel(const RegionsArgs a) {
    const int hw = a.H * a.W, lane = threadIdx.x & 63;
    const long i = blockIdx.x * 256L + threadIdx.x;
    const size_t img = (size_t)blockIdx.y * hw;
    const int r = i < hw ? a.root[img + i] : -1;     // (no early return: the whole wave takes part in the votes)
    bool waiting = r >= 0;
    for (;;) {
        const unsigned long long rest = __ballot(waiting);
        if (!rest) break;
        const int leader = __ffsll(rest) - 1;
        const int key = __shfl(r, leader);
        const bool mine = waiting && r == key;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(a.areas + img + key, __popcll(same));
        waiting = waiting && !mine;
    }
}

// ---------------------------------------------------------------- scan: count, offsets, number
__device__ __forceinline__ bool regions_kept(const RegionsArgs& a, size_t img, int i) {
    return a.root[img + i] == i && a.areas[img + i] >= a.min_area;
}

__global__ __launch_bounds__(256) void regions_count_kernel(const RegionsArgs a) {
    const int hw = a.H * a.W, n = blockIdx.y;
    const size_t img = (size_t)n * hw;
    const int begin = (int)blockIdx.x * a.chunk, end = min(begin + a.chunk, hw);
    int c = 0;
    for (int i = begin + (int)threadIdx.x; i < end; i += 256) c += regions_kept(a, img, i) ? 1 : 0;
    __shared__ int red[256];
    red[threadIdx.x] = c;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.part[(size_t)n * a.parts + blockIdx.x] = red[0];
}

// One lane per image: the exclusive prefix of its parts, in place, and K.
__global__ __launch_bounds__(64) void regions_offsets_kernel(const RegionsArgs a) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= a.N) return;
    int* p = a.part + (size_t)n * a.parts;
    int run = 0;
    for (int b = 0; b < a.parts; ++b) {
        const int c = p[b];
        p[b] = run;
        run += c;
    }
    a.count[n] = run;
}

__global__ __launch_bounds__(256) void regions_number_kernel(const RegionsArgs a) {
    __shared__ int wave_total[4];
    const int hw = a.H * a.W, n = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t img = (size_t)n * hw;
    const int begin = (int)blockIdx.x * a.chunk, end = min(begin + a.chunk, hw);
    int base = a.part[(size_t)n * a.parts + blockIdx.x];
    // (the trip count is the same for the 256 lanes: the barriers inside are reached by all of them)
    for (int s = begin; s < end; s += 256) {
        const int i = s + t;
        const bool in = i < end;
        const bool is_root = in && a.root[img + i] == i;
        const bool kept = is_root && a.areas[img + i] >= a.min_area;
        const unsigned long long votes = __ballot(kept);
        const int rank = __popcll(votes & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c = wave_total[w];
            before += w < wave ? c : 0;
            all += c;
        }
        if (is_root) {
            const int id = kept ? base + before + rank + 1 : 0;
            a.link[img + i] = id;
            if (id >= 1 && id <= a.R) {
                const size_t row = (size_t)n * a.R + (id - 1);
                const int x = i % a.W, y = i / a.W;
                a.area[row] = a.areas[img + i];
                a.box[4 * row] = x; a.box[4 * row + 1] = y; a.box[4 * row + 2] = x; a.box[4 * row + 3] = y;
            }
        }
        base += all;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- final, mean
// q = (int64) rint(clamp(u, -65536, 65536) * 65536.0): |q| <= 2^32, so 2^26 pixels sum below 2^58.
__device__ __forceinline__ long long regions_fixed(float u) {
    const double d = (double)u;
    return (long long)rint(fmin(fmax(d, -65536.0), 65536.0) * 65536.0);
}

__global__ __launch_bounds__(256) void regions_final_kernel(const RegionsArgs a) {
    const int hw = a.H * a.W;
    const long i = blockIdx.x * 256L + threadIdx.x;
    const size_t img = (size_t)blockIdx.y * hw;
    int id = 0;
    if (i < hw) {
        const int r = a.root[img + i];
        id = r >= 0 ? a.link[img + r] : 0;
        a.labels[img + i] = id;
    }
    const bool row_lane = id >= 1 && id <= a.R;      // (no early return: the whole wave takes part in the vote)
    int x = 0, y = 0;
    long long qu = 0, qv = 0;
    if (row_lane) {
        x = (int)(i % a.W); y = (int)(i / a.W);
        if (a.flow) {
            const float* f = a.flow + (img + i) * a.cs;
            qu = regions_fixed(f[0]); qv = regions_fixed(f[1]);
        }
    }
    const int lane = threadIdx.x & 63;
    bool waiting = row_lane;
    // the turns of regions_area_kernel: at most 64, one per distinct id of the wave, nothing waited for
    for (;;) {
        const unsigned long long rest = __ballot(waiting);
        if (!rest) break;
        const int leader = __ffsll(rest) - 1;
        const int key = __shfl(id, leader);
        const bool mine = waiting && id == key;
        int xmin = mine ? x : 0x7fffffff, xmax = mine ? x : -1, ymax = mine ? y : -1;
        long long su = mine ? qu : 0, sv = mine ? qv : 0;
        if (__popcll(__ballot(mine)) > 1) {          // (wave-uniform: every lane shuffles or none)
#pragma unroll
            for (int k = 32; k > 0; k >>= 1) {
                xmin = min(xmin, __shfl_xor(xmin, k)); xmax = max(xmax, __shfl_xor(xmax, k)); ymax = max(ymax, __shfl_xor(ymax, k));
                su += __shfl_xor(su, k); sv += __shfl_xor(sv, k);
            }
        }
        if (lane == leader) {
            const size_t row = (size_t)blockIdx.y * a.R + (key - 1);
            atomicMin(a.box + 4 * row, xmin);
            atomicMax(a.box + 4 * row + 2, xmax);
            atomicMax(a.box + 4 * row + 3, ymax);
            if (a.flow) {
                atomicAdd(reinterpret_cast<unsigned long long*>(a.sums + 2 * row), (unsigned long long)su);
                atomicAdd(reinterpret_cast<unsigned long long*>(a.sums + 2 * row + 1), (unsigned long long)sv);
            }
        }
        waiting = waiting && !mine;
    }
}

__global__ __launch_bounds__(256) void regions_mean_kernel(const RegionsArgs a) {
    const long r = blockIdx.x * 256L + threadIdx.x;
    if (r >= (long)a.N * a.R) return;
    const int n = a.area[r];
#pragma unroll
    for (int j = 0; j < 2; ++j) a.mean[2 * r + j] = n > 0 ? ((double)a.sums[2 * r + j] / 65536.0) / (double)n : 0.0;
}

// ---------------------------------------------------------------- host
static inline bool regions_in_range(int N, int H, int W) { return (long)H * W <= REGIONS_MAX_PIXELS && N <= 65535; }
static inline int regions_parts(int H, int W) {
    const long parts = ((long)H * W + 255) / 256;
    return (int)(parts > REGIONS_MAX_PARTS ? REGIONS_MAX_PARTS : parts);
}

extern "C" int pwc_regions_tile_h(void) { return REGIONS_TH; }
extern "C" int pwc_regions_tile_w(void) { return REGIONS_TW; }

extern "C" size_t pwc_regions_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || !regions_in_range(N, H, W)) return 0;
    return 4 * (3 * (size_t)N * H * W + 2 * (size_t)N * regions_parts(H, W));
}

extern "C" int pwc_label_regions(const uint8_t* mask, int invert, const float* flows, int flow_cs, int N, int H, int W,
                                 int connectivity, int min_area, int max_regions, void* workspace, size_t workspace_bytes,
                                 int32_t* labels, int32_t* count, int32_t* area, int32_t* box, int64_t* sums, double* mean,
                                 pwc_stream_t stream) {
    if (!mask || !workspace || !labels || !count || !area || !box) return PWC_EINVAL;
    if ((flows != nullptr) != (sums != nullptr) || (flows != nullptr) != (mean != nullptr)) return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || (connectivity != 4 && connectivity != 8) || min_area < 1 || max_regions < 1 ||
        max_regions > REGIONS_MAX_REGIONS || (flows && flow_cs < 2))
        return PWC_EINVAL;
    if (!regions_in_range(N, H, W)) return PWC_ERANGE;
    if (pwc_off(flows, 3u) || pwc_off(workspace, 7u) || pwc_off(labels, 3u) || pwc_off(count, 3u) ||
        pwc_off(area, 3u) || pwc_off(box, 3u) || pwc_off(sums, 7u) || pwc_off(mean, 7u))
        return PWC_EALIGN;
    if (workspace_bytes < pwc_regions_workspace_bytes(N, H, W)) return PWC_EINVAL;
    const size_t npix = (size_t)N * H * W;
    const int hw = H * W;
    RegionsArgs a = {};
    a.mask = mask; a.flow = flows;
    a.areas = reinterpret_cast<int*>(workspace);
    a.link = a.areas + npix;
    a.root = a.link + npix;
    a.part = a.root + npix;
    a.labels = labels; a.count = count; a.area = area; a.box = box;
    a.sums = reinterpret_cast<long long*>(sums); a.mean = mean;
    a.invert = invert ? 1 : 0; a.cs = flow_cs; a.N = N; a.H = H; a.W = W; a.conn8 = connectivity == 8 ? 1 : 0;
    a.min_area = min_area; a.R = max_regions;
    a.parts = regions_parts(H, W);
    a.chunk = (int)((((long)hw + 256L * a.parts - 1) / (256L * a.parts)) * 256L);
    a.tiles_x = (W + REGIONS_TW - 1) / REGIONS_TW;
    a.tiles_y = (H + REGIONS_TH - 1) / REGIONS_TH;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 rows((unsigned)(((long)N * max_regions + 255) / 256));
    const dim3 pixels((unsigned)((hw + 255) / 256), (unsigned)N);
    const dim3 parts((unsigned)a.parts, (unsigned)N);
    const long seam = (long)(a.tiles_y - 1) * W + (long)(a.tiles_x - 1) * H;
    hipLaunchKernelGGL(regions_clear_kernel, rows, dim3(256), 0, s, a);
    hipLaunchKernelGGL(regions_tile_kernel, dim3((unsigned)(a.tiles_x * a.tiles_y), (unsigned)N), dim3(256), 0, s, a);
    if (seam > 0) hipLaunchKernelGGL(regions_seam_kernel, dim3((unsigned)((seam + 255) / 256), (unsigned)N), dim3(256), 0, s, a);
    hipLaunchKernelGGL(regions_flatten_kernel, pixels, dim3(256), 0, s, a);
    hipLaunchKernelGGL(regions_area_kernel, pixels, dim3(256), 0, s, a);
    hipLaunchKernelGGL(regions_count_kernel, parts, dim3(256), 0, s, a);
    hipLaunchKernelGGL(regions_offsets_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s, a);
    hipLaunchKernelGGL(regions_number_kernel, parts, dim3(256), 0, s, a);
    hipLaunchKernelGGL(regions_final_kernel, pixels, dim3(256), 0, s, a);
    if (flows) hipLaunchKernelGGL(regions_mean_kernel, rows, dim3(256), 0, s, a);
    return pwc_launch_status();
}
