// pwc_region_links.hip -- region tracking: the join between the label images of consecutive pairs.  label_regions numbers the
// regions of every image on its own; this file says which region of image b a region of image a becomes under the flow a -> b
// (a MUTUAL best overlap), carries identities along those links through a sequence, and paints them (gfx950; C ABI in
// include/pwc_hip.h, "region tracking"; semantics and launch plan in DESIGN.md 22).
//
//   pwc_region_links_workspace_bytes  4 N R (R + 2), rounded up to 8: the vote table
//   pwc_link_regions                  succ, pred, best_succ, best_pred (N, R) int32, votes (N, R, 4) int32
//   pwc_region_identities             ids, age (S, R) int32, next_id_out (1) int32
//   pwc_relabel_regions               out (S, H, W) int32
//
// The result is a function of the input alone: every count is an integer added by atomics, the same in any order; a best is the
// largest count with ties to the smallest index, whatever the order in which lanes meet the candidates.  tests/region_links_ref.py
// restates the definition (not these launches) and the tests hold every output to its bits.
//
// pwc_link_regions, five launches on the caller's stream, each reading what the one before wrote:
//   clear    a lane per table element.  The table is [N][R][R + 2]: row a - 1 holds overlap[a][0 .. R] and, in column R + 1,
//            left[a] -- so that a vote is ONE key and one atomic whichever kind it is.
//   vote     a lane per pixel of image a.  A voter computes its key (la - 1)(R + 2) + c; the lanes of a wave that hold one key
//            leave together with one atomicAdd of their number (the turns of regions_area_kernel: at most 64, wave-uniform).
//   rows     a wave per row: lane l looks at the columns 1 + l, 65 + l, ... and keeps its best; a butterfly over the wave with
//            (count descending, column ascending) as the order gives best_succ; the sum of the whole row is the row's voters.
//   columns  a workgroup per 64 columns: wave w walks the rows of the w-th quarter in ascending order, a lane per column; the four
//            candidates of a column meet in the LDS in ascending order of their rows.
//   match    a lane per table row: succ of region a = row + 1 and pred of region b = row + 1.
// pwc_region_identities is one launch of one workgroup of 1024 lanes, a lane per table row, the loop over the images inside;
// pwc_relabel_regions one launch with a lane per pixel.
// No host synchronisation, no process-wide state, no floating-point atomic, and no loop that waits for another lane or
// workgroup: every loop's bound is stated next to it.  Between launches the stream's order is the hand-off.
#include "flow_record.h"

#pragma clang fp contract(off)

#define LINKS_MAX_REGIONS 1024
#define LINKS_MAX_PIXELS (1L << 26)
#define LINKS_MAX_IMAGES 65535

struct LinksArgs {
    const int* labels_a;      // [N][H][W]
    const int* labels_b;      // [N][H][W]
    const int* area_a;        // [N][R]
    const int* area_b;        // [N][R]
    const float* flow;        // [N][H][W] records of cs floats, 2 used
    const uint8_t* valid;     // [N][H][W] or null
    int* table;               // [N][R][R + 2]: overlap[a][0 .. R], left[a]
    int* succ;                // [N][R]
    int* pred;                // [N][R]
    int* best_succ;           // [N][R]
    int* best_pred;           // [N][R]
    int* votes;               // [N][R][4]
    double min_fraction;
    int cs, N, H, W, R, min_overlap;
};

// ---------------------------------------------------------------- clear
__global__ __launch_bounds__(256) void links_clear_kernel(const LinksArgs a) {
    const long per = (long)a.R * (a.R + 2);
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= per) return;
    a.table[(size_t)blockIdx.y * per + i] = 0;
}

// ---------------------------------------------------------------- vote
__global__ __launch_bounds__(256) void links_vote_kernel(const LinksArgs a) {
    const int hw = a.H * a.W, lane = threadIdx.x & 63;
    const long i = blockIdx.x * 256L + threadIdx.x;
    const size_t img = (size_t)blockIdx.y * hw;
    int key = -1;                                    // (no early return: the whole wave takes part in the votes)
    if (i < hw) {
        const int la = a.labels_a[img + i];
        if (la >= 1 && la <= a.R && (!a.valid || a.valid[img + i] != 0)) {
            const float* f = a.flow + (img + i) * a.cs;
            const float u = f[0], v = f[1];
            if (pwc_flow_known(u, v)) {
                const int x = (int)(i % a.W), y = (int)(i / a.W);
                const double qx = rint((double)x + (double)u), qy = rint((double)y + (double)v);
                int c = a.R + 1;                     // the column of left[a]
                if (qx >= 0.0 && qx <= (double)(a.W - 1) && qy >= 0.0 && qy <= (double)(a.H - 1)) {
                    const int lb = a.labels_b[img + (size_t)((int)qy) * a.W + (int)qx];
                    c = lb >= 1 && lb <= a.R ? lb : 0;
                }
                key = (la - 1) * (a.R + 2) + c;      // < 1024 * 1026
            }
        }
    }
    int* table = a.table + (size_t)blockIdx.y * a.R * (a.R + 2);
    bool waiting = key >= 0;
    // ends by itself: a turn retires at least the lane whose key it took, so there are at most 64 turns; the loop's condition
    // is wave-uniform and nothing is waited for
    for (;;) {
        const unsigned long long rest = __ballot(waiting);
        if (!rest) break;
        const int leader = __ffsll(rest) - 1;
        const int k = __shfl(key, leader);
        const bool mine = waiting && key == k;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(table + k, __popcll(same));
        waiting = waiting && !mine;
    }
}

// ---------------------------------------------------------------- rows: best_succ and the votes
// (count, index) in the order "larger count first, then smaller index": true where (c1, i1) comes before (c0, i0).
__device__ __forceinline__ bool links_before(int c1, int i1, int c0, int i0) { return c1 > c0 || (c1 == c0 && i1 < i0); }

__global__ __launch_bounds__(256) void links_rows_kernel(const LinksArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);       // (wave-uniform)
    if (row >= a.R) return;
    const size_t r = (size_t)blockIdx.y * a.R + row;
    const int* t = a.table + r * (a.R + 2);
    int best = 0, at = 0x7fffffff, total = 0;
    // columns 1 .. R in ascending order per lane: only a strictly larger count replaces, so a lane keeps its smallest column
    for (int c = 1 + lane; c <= a.R; c += 64) {
        const int v = t[c];
        total += v;
        if (v > best) { best = v; at = c; }
    }
    const int bg = t[0], left = t[a.R + 1];
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) {
        const int ob = __shfl_xor(best, k), oa = __shfl_xor(at, k);
        total += __shfl_xor(total, k);
        if (links_before(ob, oa, best, at)) { best = ob; at = oa; }
    }
    if (lane == 0) {
        a.best_succ[r] = best > 0 ? at : 0;
        a.votes[4 * r] = best; a.votes[4 * r + 1] = bg; a.votes[4 * r + 2] = left; a.votes[4 * r + 3] = total + bg + left;
    }
}

// ---------------------------------------------------------------- columns: best_pred
__global__ __launch_bounds__(256) void links_columns_kernel(const LinksArgs a) {
    __shared__ int cand_count[4][64], cand_row[4][64];
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane + 1;                // region b
    const int quarter = (a.R + 3) / 4, begin = part * quarter, end = min(begin + quarter, a.R);
    const int* t = a.table + (size_t)blockIdx.y * a.R * (a.R + 2);
    int best = 0, at = 0;
    if (col <= a.R) {
        // rows in ascending order: only a strictly larger count replaces, so the smallest row of the largest count stays
        for (int row = begin; row < end; ++row) {
            const int v = t[(size_t)row * (a.R + 2) + col];
            if (v > best) { best = v; at = row + 1; }
        }
    }
    cand_count[part][lane] = best; cand_row[part][lane] = at;
    __syncthreads();
    if (part == 0 && col <= a.R) {
#pragma unroll
        for (int p = 1; p < 4; ++p)                            // (the quarters in ascending order of their rows)
            if (cand_count[p][lane] > best) { best = cand_count[p][lane]; at = cand_row[p][lane]; }
        a.best_pred[(size_t)blockIdx.y * a.R + col - 1] = best > 0 ? at : 0;
    }
}

// ---------------------------------------------------------------- match
__device__ __forceinline__ bool links_accept(const LinksArgs& a, size_t n, int ra, int rb) {       // regions ra -> rb, both 1 .. R
    const int ov = a.table[(n * a.R + (ra - 1)) * (a.R + 2) + rb];
    const int m = min(a.area_a[n * a.R + ra - 1], a.area_b[n * a.R + rb - 1]);
    return ov >= a.min_overlap && (double)ov >= a.min_fraction * (double)m;
}

__global__ __launch_bounds__(256) void links_match_kernel(const LinksArgs a) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= a.R) return;
    const size_t n = blockIdx.y, r = n * a.R + row;
    const int me = row + 1;
    const int b = a.best_succ[r];
    a.succ[r] = b != 0 && a.best_pred[n * a.R + b - 1] == me && links_accept(a, n, me, b) ? b : 0;
    const int p = a.best_pred[r];
    a.pred[r] = p != 0 && a.best_succ[n * a.R + p - 1] == me && links_accept(a, n, p, me) ? p : 0;
}

// ---------------------------------------------------------------- identities
struct IdentArgs {
    const int* pred;          // [S - 1][R]: the link s - 1 -> s; null where S == 1
    const int* count;         // [S]
    const int* ids_prev;      // [R] or null
    const int* age_prev;      // [R], with ids_prev
    const int* pred_prev;     // [R], with ids_prev: the link from the earlier call's last image to image 0
    const int* next_id_in;    // [1] or null: the first fresh id, where it is on the device
    int* ids;                 // [S][R]
    int* age;                 // [S][R]
    int* next_id_out;         // [1]
    int next_id, S, R;
};

// One workgroup, lane r is table row r.  The previous image's ids and ages are in the LDS; a step reads them, meets at a barrier
// (every read is done, the waves' fresh counts are there), writes the image's own over them and meets again.  The trip count S
// is the same for the 1024 lanes: the barriers inside are reached by all of them.
__global__ __launch_bounds__(1024) void links_identities_kernel(const IdentArgs a) {
    __shared__ int ids_l[LINKS_MAX_REGIONS], age_l[LINKS_MAX_REGIONS], wave_total[16];
    const int r = threadIdx.x, lane = r & 63, wave = r >> 6;
    int next = a.next_id_in ? a.next_id_in[0] : a.next_id;
    const bool row = r < a.R;
    ids_l[r] = a.ids_prev && row ? a.ids_prev[r] : 0;
    age_l[r] = a.ids_prev && row ? a.age_prev[r] : 0;
    __syncthreads();
    for (int s = 0; s < a.S; ++s) {
        const int* link = s == 0 ? a.pred_prev : a.pred + (size_t)(s - 1) * a.R;       // null: image 0 of a first call
        const bool live = row && r < a.count[s];
        int id = 0, ag = 0;
        if (live && link) {
            const int p = link[r];
            if (p >= 1 && p <= a.R && ids_l[p - 1] != 0) { id = ids_l[p - 1]; ag = age_l[p - 1] + 1; }
        }
        const bool fresh = live && id == 0;
        const unsigned long long votes = __ballot(fresh);
        const int rank = __popcll(votes & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int c = wave_total[w];
            before += w < wave ? c : 0;
            all += c;
        }
        if (fresh) { id = next + before + rank; ag = 1; }
        next += all;
        ids_l[r] = id; age_l[r] = ag;
        if (row) { a.ids[(size_t)s * a.R + r] = id; a.age[(size_t)s * a.R + r] = ag; }
        __syncthreads();
    }
    if (r == 0) a.next_id_out[0] = next;
}

// ---------------------------------------------------------------- relabel
__global__ __launch_bounds__(256) void links_relabel_kernel(const int* __restrict__ labels, const int* __restrict__ ids, int hw, int R,
                                                            int* __restrict__ out) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= hw) return;
    const size_t g = (size_t)blockIdx.y * hw + i;
    const int la = labels[g];
    out[g] = la >= 1 && la <= R ? ids[(size_t)blockIdx.y * R + la - 1] : 0;
}

// ---------------------------------------------------------------- host
static inline bool links_in_range(int N, int H, int W) { return (long)H * W <= LINKS_MAX_PIXELS && N <= LINKS_MAX_IMAGES; }

extern "C" size_t pwc_region_links_workspace_bytes(int N, int max_regions) {
    if (N < 1 || N > LINKS_MAX_IMAGES || max_regions < 1 || max_regions > LINKS_MAX_REGIONS) return 0;
    return (4 * (size_t)N * max_regions * (max_regions + 2) + 7) & ~(size_t)7;
}

extern "C" int pwc_link_regions(const int32_t* labels_a, const int32_t* labels_b, const int32_t* area_a, const int32_t* area_b,
                                const float* flows_ab, int flow_cs, const uint8_t* valid_ab, int N, int H, int W, int max_regions,
                                int min_overlap, double min_fraction, void* workspace, size_t workspace_bytes, int32_t* succ,
                                int32_t* pred, int32_t* best_succ, int32_t* best_pred, int32_t* votes, pwc_stream_t stream) {
    if (!labels_a || !labels_b || !area_a || !area_b || !flows_ab || !workspace || !succ || !pred || !best_succ || !best_pred || !votes)
        return PWC_EINVAL;
    if (N < 1 || H < 1 || W < 1 || max_regions < 1 || min_overlap < 1 || !(min_fraction >= 0.0 && min_fraction <= 1.0) || flow_cs < 2)
        return PWC_EINVAL;
    if (!links_in_range(N, H, W) || max_regions > LINKS_MAX_REGIONS) return PWC_ERANGE;
    if (pwc_off(labels_a, 3u) || pwc_off(labels_b, 3u) || pwc_off(area_a, 3u) || pwc_off(area_b, 3u) || pwc_off(flows_ab, 3u) ||
        pwc_off(workspace, 7u) || pwc_off(succ, 3u) || pwc_off(pred, 3u) || pwc_off(best_succ, 3u) || pwc_off(best_pred, 3u) ||
        pwc_off(votes, 3u))
        return PWC_EALIGN;
    if (workspace_bytes < pwc_region_links_workspace_bytes(N, max_regions)) return PWC_EINVAL;
    LinksArgs a = {};
    a.labels_a = labels_a; a.labels_b = labels_b; a.area_a = area_a; a.area_b = area_b; a.flow = flows_ab; a.valid = valid_ab;
    a.table = reinterpret_cast<int*>(workspace);
    a.succ = succ; a.pred = pred; a.best_succ = best_succ; a.best_pred = best_pred; a.votes = votes;
    a.min_fraction = min_fraction;
    a.cs = flow_cs; a.N = N; a.H = H; a.W = W; a.R = max_regions; a.min_overlap = min_overlap;
    const hipStream_t s = (hipStream_t)stream;
    const int R = max_regions;
    const long per = (long)R * (R + 2);
    hipLaunchKernelGGL(links_clear_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)N), dim3(256), 0, s, a);
    hipLaunchKernelGGL(links_vote_kernel, dim3((unsigned)(((long)H * W + 255) / 256), (unsigned)N), dim3(256), 0, s, a);
    hipLaunchKernelGGL(links_rows_kernel, dim3((unsigned)((R + 3) / 4), (unsigned)N), dim3(256), 0, s, a);
    hipLaunchKernelGGL(links_columns_kernel, dim3((unsigned)((R + 63) / 64), (unsigned)N), dim3(256), 0, s, a);
    hipLaunchKernelGGL(links_match_kernel, dim3((unsigned)((R + 255) / 256), (unsigned)N), dim3(256), 0, s, a);
    return pwc_launch_status();
}

extern "C" int pwc_region_identities(const int32_t* pred, const int32_t* count, const int32_t* ids_prev, const int32_t* age_prev,
                                     const int32_t* pred_prev, int next_id, const int32_t* next_id_in, int S, int max_regions,
                                     int32_t* ids, int32_t* age, int32_t* next_id_out, pwc_stream_t stream) {
    if (!count || !ids || !age || !next_id_out || (S > 1 && !pred)) return PWC_EINVAL;
    if ((ids_prev != nullptr) != (age_prev != nullptr) || (ids_prev != nullptr) != (pred_prev != nullptr)) return PWC_EINVAL;
    if (S < 1 || max_regions < 1 || next_id < 1) return PWC_EINVAL;
    if (max_regions > LINKS_MAX_REGIONS || (long)next_id + (long)S * max_regions >= (1L << 31)) return PWC_ERANGE;
    if (pwc_off(pred, 3u) || pwc_off(count, 3u) || pwc_off(ids_prev, 3u) || pwc_off(age_prev, 3u) || pwc_off(pred_prev, 3u) ||
        pwc_off(next_id_in, 3u) || pwc_off(ids, 3u) || pwc_off(age, 3u) || pwc_off(next_id_out, 3u))
        return PWC_EALIGN;
    IdentArgs a = {};
    a.pred = pred; a.count = count; a.ids_prev = ids_prev; a.age_prev = age_prev; a.pred_prev = pred_prev; a.next_id_in = next_id_in;
    a.ids = ids; a.age = age; a.next_id_out = next_id_out;
    a.next_id = next_id; a.S = S; a.R = max_regions;
    hipLaunchKernelGGL(links_identities_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    return pwc_launch_status();
}

extern "C" int pwc_relabel_regions(const int32_t* labels, const int32_t* ids, int S, int H, int W, int max_regions, int32_t* out,
                                   pwc_stream_t stream) {
    if (!labels || !ids || !out) return PWC_EINVAL;
    if (S < 1 || H < 1 || W < 1 || max_regions < 1) return PWC_EINVAL;
    if (!links_in_range(S, H, W) || max_regions > LINKS_MAX_REGIONS) return PWC_ERANGE;
    if (pwc_off(labels, 3u) || pwc_off(ids, 3u) || pwc_off(out, 3u)) return PWC_EALIGN;
    hipLaunchKernelGGL(links_relabel_kernel, dim3((unsigned)(((long)H * W + 255) / 256), (unsigned)S), dim3(256), 0,
                       (hipStream_t)stream, labels, ids, H * W, max_regions, out);
    return pwc_launch_status();
}
