// pwc_trajectory.hip -- the baseline scale chained across the pairs of ONE sequence, and the camera's path through it, wholly on the
// device (gfx950; C ABI and every operation's order in include/pwc_hip.h, "scale chain and camera trajectory"; launch plan, digit
// choice and figures in DESIGN.md 29).
//
//   pwc_scale_links_workspace_bytes   per seam a 16-byte selection record, 5120 int32 bins and H W 32-bit keys
//   pwc_scale_links_f32               ratio (T) floats, samples (T) int32: per seam the lower median of the per-pixel scale ratio
//   pwc_camera_trajectory_f64         trajectory (T + 1, 3, 4), scales (T) doubles, segment (T) int32, linked (T) bytes
//
// A seam lies between pair j - 1 (frames j - 1 -> j) and pair j (frames j -> j + 1).  A rigid point that pair j - 1 sees at pixel p
// has the depth Z1 in camera j in pair j - 1's baselines (two_view.h's triangulation, recomputed from the flow and the pose) and the
// depth d in camera j in pair j's baselines (pair j's depth map sampled at p + flow(p) under compose_flows' four-corner rule).
// ratio = Z1 / d = b_j / b_(j-1) is what multiplies scale[j - 1] to give scale[j]; the seam's ratio is the LOWER MEDIAN over the image.
// pwc_scale_links_f32 is 2 memsets and 6 launches on the caller's stream, each reading what the one before wrote:
//   keys      grid (parts, seams), loss_common.h's partition: every pixel's key -- the bits of its float32 ratio, 0 where it is no
//             sample -- into the workspace, and the histogram of the keys' top 11 bits.
//   select 0  a workgroup per seam: n = the samples, the wanted rank (n - 1) / 2, the top digit that holds it, the rank inside it.
//   hist 1    grid (parts, seams): the histogram of the middle 11 bits of the keys whose top digit is the chosen one.
//   select 1, hist 2 (the low 10 bits), select 2: the same; select 2 writes ratio and samples.
// Positive float32 values order like their bit patterns, so this is an exact selection: no sort, no floating-point atomic.  A
// workgroup's histogram lives in the LDS (8 KB at most) and is merged into the seam's table with one integer atomic per non-empty
// bin: integers, the same in any order.  The ratios of a rigid scene agree to a few ulps -- every lane of a wave then adds to ONE
// bin -- so a wave whose samples all share a digit adds their number with one LDS atomic (trj_hist_add).  No lane and no workgroup
// waits for another; no host synchronisation.
// pwc_camera_trajectory_f64 is one launch, one lane, sequential over the pairs: IEEE double + - x and comparisons in the order
// written here, no fused multiply-add (the pragma below), no library call.  tests/trajectory_ref.py restates both in numpy bit for bit.
#include "loss_common.h"
#include "two_view.h"

#pragma clang fp contract(off)

#define TRJ_MAX_PIXELS (1L << 26)
#define TRJ_TOP_BINS 2048     // key >> 21
#define TRJ_MID_BINS 2048     // (key >> 10) & 2047
#define TRJ_LOW_BINS 1024     // key & 1023
#define TRJ_BINS (TRJ_TOP_BINS + TRJ_MID_BINS + TRJ_LOW_BINS)
#define TRJ_SEL 4             // int32 per seam: the key's chosen bits so far, the rank inside them, n, unused

struct LinkArgs {
    const float* flow;        // [T][H][W] records of cs floats, 2 used
    const double* rotation;   // [T][9]
    const double* translation;// [T][3]
    const double* intrinsics; // [T][4]
    const float* depth;       // [T][H][W]
    const uint8_t* known;     // [T][H][W]
    const float* pflow;       // the previous pair's, null without one: [H][W] records of pcs floats
    const double* protation;  // [9]
    const double* ptranslation; // [3]
    const double* pintrinsics;  // [4]
    const uint8_t* pknown;    // [H][W]
    unsigned* keys;           // [seams][H W]
    int* hist;                // [seams][TRJ_BINS]
    int* sel;                 // [seams][TRJ_SEL]
    float* ratio;             // [T]
    int* samples;             // [T]
    int cs, pcs, T, H, W;
    int first;                // the pair behind seam 0: 0 with a previous pair, else 1
};

// One more key in a workgroup's histogram.  Every lane of the wave calls it (has: this lane holds a sample).  Where all the wave's
// samples share their digit one lane adds their number, else every sample adds 1: integer additions, the same table either way.
__device__ __forceinline__ void trj_hist_add(int* h, unsigned digit, bool has) {
    const unsigned long long m = __ballot(has);
    if (m == 0ull) return;
    const int lead = __ffsll((long long)m) - 1;
    const unsigned d0 = (unsigned)__shfl((int)digit, lead);
    const unsigned long long same = __ballot(has && digit == d0);
    if (same == m) {
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(h + d0, (int)__popcll(m));
    } else if (has) {
        atomicAdd(h + digit, 1);
    }
}

template <int BINS>
__device__ __forceinline__ void trj_hist_clear(int* h) {
#pragma unroll
    for (int i = threadIdx.x; i < BINS; i += 256) h[i] = 0;
    __syncthreads();
}
template <int BINS>
__device__ __forceinline__ void trj_hist_merge(const int* h, int* table) {
    __syncthreads();
#pragma unroll
    for (int i = threadIdx.x; i < BINS; i += 256) {
        const int c = h[i];
        if (c != 0) atomicAdd(table + i, c);
    }
}

// ---------------------------------------------------------------- keys: grid (parts, seams)
template <bool VEC>
__global__ __launch_bounds__(256) void trj_keys_kernel(const LinkArgs a) {
    __shared__ int h[TRJ_TOP_BINS];
    const int s = blockIdx.y, hw = a.H * a.W;
    const int jb = a.first + s, ja = jb - 1;                               // the seam's later and earlier pair; ja = -1: the previous pair
    const float* flow = ja < 0 ? a.pflow : a.flow + (size_t)ja * hw * a.cs;
    const int cs = ja < 0 ? a.pcs : a.cs;
    const double* Rp = ja < 0 ? a.protation : a.rotation + (size_t)ja * 9;
    const double* tp = ja < 0 ? a.ptranslation : a.translation + (size_t)ja * 3;
    const double* kp = ja < 0 ? a.pintrinsics : a.intrinsics + (size_t)ja * 4;
    const uint8_t* known = ja < 0 ? a.pknown : a.known + (size_t)ja * hw;
    const float* depth = a.depth + (size_t)jb * hw;
    const uint8_t* known_b = a.known + (size_t)jb * hw;
    double R[9], t[3], k[4];
    bool zero_a = true, zero_b = true;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        R[j] = Rp[j];
        zero_a = zero_a && R[j] == 0.0;
        zero_b = zero_b && a.rotation[(size_t)jb * 9 + j] == 0.0;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = tp[j];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = kp[j];
    const bool dead = zero_a || zero_b || !two_view_intrinsics_fine(k);    // (the whole seam: every key is 0)
    trj_hist_clear<TRJ_TOP_BINS>(h);
    unsigned* keys = a.keys + (size_t)s * hw;
    for (int base = blockIdx.x * 256; base < hw; base += (int)gridDim.x * 256) {
        const int i = base + threadIdx.x;
        unsigned key = 0u;
        if (i < hw && !dead && known[i]) {
            float fu, fv;
            pwc_flow_load2<VEC>(flow + (size_t)i * cs, fu, fv);
            if (pwc_flow_known(fu, fv)) {
                const double x = (double)(i % a.W), y = (double)(i / a.W);
                const double qx = x + (double)fu, qy = y + (double)fv;
                // compose_flows' rule: q in frame (which keeps the four corner reads inside the image) and ALL FOUR corners known
                if (qx >= 0.0 && qx <= (double)(a.W - 1) && qy >= 0.0 && qy <= (double)(a.H - 1)) {
                    const PwcBilinearF64 bl = pwc_bilinear_f64(qx, qy, a.H, a.W);
                    const size_t o00 = bl.o00, o01 = bl.o01, o10 = bl.o10, o11 = bl.o11;
                    if (known_b[o00] && known_b[o01] && known_b[o10] && known_b[o11]) {
                        const double wx0 = bl.wx0, wx1 = bl.wx1, wy0 = bl.wy0, wy1 = bl.wy1;
                        const double top = (wx0 * (double)depth[o00]) + (wx1 * (double)depth[o01]);
                        const double bot = (wx0 * (double)depth[o10]) + (wx1 * (double)depth[o11]);
                        const double d = (wy0 * top) + (wy1 * bot);
                        const double d0x = (x - k[2]) / k[0], d0y = (y - k[3]) / k[1], d1x = (qx - k[2]) / k[0], d1y = (qy - k[3]) / k[1];
                        const TwoViewPoint pt = two_view_triangulate(R, t, d0x, d0y, d1x, d1y);
                        if (pt.den > 0.0 && pt.z1 > 0.0 && d > 0.0) {
                            const float r = (float)(pt.z1 / d);
                            if (r > 0.f && r <= 3.4028234663852886e38f) key = __float_as_uint(r);
                        }
                    }
                }
            }
        }
        if (i < hw) keys[i] = key;
        trj_hist_add(h, key >> 21, key != 0u);
    }
    trj_hist_merge<TRJ_TOP_BINS>(h, a.hist + (size_t)s * TRJ_BINS);
}

// ---------------------------------------------------------------- hist: grid (parts, seams); PASS 1 the middle digit, PASS 2 the low one
template <int PASS>
__global__ __launch_bounds__(256) void trj_hist_kernel(const LinkArgs a) {
    constexpr int BINS = PASS == 1 ? TRJ_MID_BINS : TRJ_LOW_BINS;
    constexpr int SHIFT = PASS == 1 ? 21 : 10;                             // the bits chosen so far are those above SHIFT
    __shared__ int h[BINS];
    const int s = blockIdx.y, hw = a.H * a.W;
    const int* sel = a.sel + (size_t)s * TRJ_SEL;
    if (sel[2] == 0) return;                                               // (the whole workgroup: the seam has no sample)
    const unsigned chosen = (unsigned)sel[0] >> SHIFT;
    trj_hist_clear<BINS>(h);
    const unsigned* keys = a.keys + (size_t)s * hw;
    for (int base = blockIdx.x * 256; base < hw; base += (int)gridDim.x * 256) {
        const int i = base + threadIdx.x;
        const unsigned key = i < hw ? keys[i] : 0u;
        const unsigned digit = PASS == 1 ? (key >> 10) & (TRJ_MID_BINS - 1) : key & (TRJ_LOW_BINS - 1);
        trj_hist_add(h, digit, key != 0u && (key >> SHIFT) == chosen);
    }
    trj_hist_merge<BINS>(h, a.hist + (size_t)s * TRJ_BINS + (PASS == 1 ? TRJ_TOP_BINS : TRJ_TOP_BINS + TRJ_MID_BINS));
}

// ---------------------------------------------------------------- select: a workgroup per seam
// The bin that holds the wanted rank: 256 lanes add BINS / 256 bins each, lane 0 walks the 256 sums and then the bins of one.
template <int PASS>
__global__ __launch_bounds__(256) void trj_select_kernel(const LinkArgs a) {
    constexpr int BINS = PASS == 2 ? TRJ_LOW_BINS : TRJ_MID_BINS;
    constexpr int PER = BINS / 256;
    constexpr int SHIFT = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
    __shared__ int part[256];
    const int s = blockIdx.x;
    const int* h = a.hist + (size_t)s * TRJ_BINS + (PASS == 0 ? 0 : (PASS == 1 ? TRJ_TOP_BINS : TRJ_TOP_BINS + TRJ_MID_BINS));
    int sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) sum += h[threadIdx.x * PER + k];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int* sel = a.sel + (size_t)s * TRJ_SEL;
    int n, rank;
    if (PASS == 0) {
        n = 0;
        for (int g = 0; g < 256; ++g) n += part[g];
        rank = n > 0 ? (n - 1) / 2 : 0;
    } else {
        n = sel[2];
        rank = sel[1];
    }
    unsigned bits = PASS == 0 ? 0u : (unsigned)sel[0];
    if (n > 0) {
        int g = 0, before = 0;
        while (g < 255 && before + part[g] <= rank) { before += part[g]; ++g; }
        int b = g * PER;
        while (b < g * PER + PER - 1 && before + h[b] <= rank) { before += h[b]; ++b; }
        bits |= (unsigned)b << SHIFT;
        rank -= before;
    }
    if (PASS < 2) {
        sel[0] = (int)bits; sel[1] = rank; sel[2] = n; sel[3] = 0;
    } else {
        a.ratio[a.first + s] = n > 0 ? __uint_as_float(bits) : 0.f;
        a.samples[a.first + s] = n;
    }
}

// ---------------------------------------------------------------- trajectory: one lane
struct TrajectoryArgs {
    const double* rotation;   // [T][9]
    const double* translation;// [T][3]
    const float* ratio;       // [T]
    const int* samples;       // [T]
    const double* protation;  // the previous pair's [9], null without a state
    const double* prow;       // [12]: the state's trajectory row
    const double* pscale;     // [1]
    const int* psegment;      // [2]: the previous pair's segment, the segments opened so far
    double* trajectory;       // [T + 1][12]
    double* scales;           // [T]
    int* segment;             // [T]
    uint8_t* linked;          // [T]
    int* segment_state;       // [2]
    int T, min_samples;
};

__global__ __launch_bounds__(64) void trj_chain_kernel(const TrajectoryArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double A[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, c[3] = {0.0, 0.0, 0.0};
    double scale = 0.0;
    int seg = -1, opened = 0;
    bool before_ok = false;
    if (a.protation) {
        bool zero = true;
#pragma unroll
        for (int j = 0; j < 9; ++j) zero = zero && a.protation[j] == 0.0;
        before_ok = !zero;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int q = 0; q < 3; ++q) A[3 * r + q] = a.prow[4 * r + q];
            c[r] = a.prow[4 * r + 3];
        }
        scale = a.pscale[0];
        seg = a.psegment[0];
        opened = a.psegment[1];
    }
    for (int j = 0; j < a.T; ++j) {
        double R[9], t[3];
        bool zero = true;
#pragma unroll
        for (int q = 0; q < 9; ++q) { R[q] = a.rotation[(size_t)j * 9 + q]; zero = zero && R[q] == 0.0; }
#pragma unroll
        for (int q = 0; q < 3; ++q) t[q] = a.translation[(size_t)j * 3 + q];
        const float ratio = a.ratio[j];
        const bool link = !zero && before_ok && a.samples[j] >= a.min_samples && ratio > 0.f && ratio <= 3.4028234663852886e38f;
        if (!zero && !link) {                                              // the world frame restarts at this pair's first camera
#pragma unroll
            for (int q = 0; q < 9; ++q) A[q] = (q == 0 || q == 4 || q == 8) ? 1.0 : 0.0;
            c[0] = 0.0; c[1] = 0.0; c[2] = 0.0;
        }
        double* row = a.trajectory + (size_t)j * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int q = 0; q < 3; ++q) row[4 * r + q] = A[3 * r + q];
            row[4 * r + 3] = c[r];
        }
        if (zero) {
            scale = 0.0;
            seg = -1;
        } else if (link) {
            scale = scale * (double)ratio;
        } else {
            scale = 1.0;
            seg = opened;
            opened += 1;
        }
        a.scales[j] = scale;
        a.segment[j] = seg;
        a.linked[j] = link ? 1 : 0;
        if (!zero) {
            double B[9], e[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int q = 0; q < 3; ++q) B[3 * r + q] = ((R[3 * r] * A[q]) + (R[3 * r + 1] * A[3 + q])) + (R[3 * r + 2] * A[6 + q]);
                e[r] = (((R[3 * r] * c[0]) + (R[3 * r + 1] * c[1])) + (R[3 * r + 2] * c[2])) + (scale * t[r]);
            }
#pragma unroll
            for (int q = 0; q < 9; ++q) A[q] = B[q];
            c[0] = e[0]; c[1] = e[1]; c[2] = e[2];
        } else {
#pragma unroll
            for (int q = 0; q < 9; ++q) A[q] = (q == 0 || q == 4 || q == 8) ? 1.0 : 0.0;
            c[0] = 0.0; c[1] = 0.0; c[2] = 0.0;
        }
        before_ok = !zero;
    }
    double* row = a.trajectory + (size_t)a.T * 12;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int q = 0; q < 3; ++q) row[4 * r + q] = A[3 * r + q];
        row[4 * r + 3] = c[r];
    }
    a.segment_state[0] = seg;
    a.segment_state[1] = opened;
}

// ---------------------------------------------------------------- host
static inline bool trj_in_range(int T, int H, int W) { return (long)H * W <= TRJ_MAX_PIXELS && T <= 65535; }

// per seam: the selection record and the three tables (one memset clears them), then the keys
static inline size_t trj_table_words(int seams) { return (size_t)seams * (TRJ_SEL + TRJ_BINS); }

extern "C" size_t pwc_scale_links_workspace_bytes(int T, int H, int W, int has_prev) {
    if (T < 1 || H < 1 || W < 1 || !trj_in_range(T, H, W)) return 0;
    const int seams = T - 1 + (has_prev ? 1 : 0);
    return 4 * (trj_table_words(seams) + (size_t)seams * H * W) + 16;      // (never 0 for a valid shape: T = 1 without a previous pair)
}

extern "C" int pwc_scale_links_f32(const float* flows, int flow_cs, const double* rotation, const double* translation,
                                   const double* intrinsics, const float* depth, const uint8_t* known, int T, int H, int W,
                                   const float* prev_flow, int prev_cs, const double* prev_rotation, const double* prev_translation,
                                   const double* prev_intrinsics, const uint8_t* prev_known, void* workspace, size_t workspace_bytes,
                                   float* ratio, int32_t* samples, pwc_stream_t stream) {
    if (!flows || !rotation || !translation || !intrinsics || !depth || !known || !workspace || !ratio || !samples) return PWC_EINVAL;
    if (T < 1 || H < 1 || W < 1 || flow_cs < 2) return PWC_EINVAL;
    const bool has_prev = prev_flow != nullptr;
    if (has_prev && (!prev_rotation || !prev_translation || !prev_intrinsics || !prev_known || prev_cs < 2)) return PWC_EINVAL;
    if (!trj_in_range(T, H, W)) return PWC_ERANGE;
    if (pwc_off(flows, 3u) || pwc_off(prev_flow, 3u) || pwc_off(depth, 3u) || pwc_off(ratio, 3u) || pwc_off(samples, 3u) ||
        pwc_off(rotation, 7u) || pwc_off(translation, 7u) || pwc_off(intrinsics, 7u) || pwc_off(prev_rotation, 7u) ||
        pwc_off(prev_translation, 7u) || pwc_off(prev_intrinsics, 7u) || pwc_off(workspace, 7u))
        return PWC_EALIGN;
    if (workspace_bytes < pwc_scale_links_workspace_bytes(T, H, W, has_prev ? 1 : 0)) return PWC_EINVAL;
    const int seams = T - 1 + (has_prev ? 1 : 0);
    LinkArgs a = {};
    a.flow = flows; a.rotation = rotation; a.translation = translation; a.intrinsics = intrinsics; a.depth = depth; a.known = known;
    a.pflow = prev_flow; a.protation = prev_rotation; a.ptranslation = prev_translation; a.pintrinsics = prev_intrinsics;
    a.pknown = prev_known;
    a.sel = reinterpret_cast<int*>(workspace);
    a.hist = a.sel + (size_t)seams * TRJ_SEL;
    a.keys = reinterpret_cast<unsigned*>(a.hist + (size_t)seams * TRJ_BINS);
    a.ratio = ratio; a.samples = samples;
    a.cs = flow_cs; a.pcs = has_prev ? prev_cs : flow_cs; a.T = T; a.H = H; a.W = W; a.first = has_prev ? 0 : 1;
    const hipStream_t s = (hipStream_t)stream;
    hipError_t me = hipMemsetAsync(ratio, 0, 4 * (size_t)T, s);            // (entry 0 without a previous pair; T = 1: all there is)
    if (me == hipSuccess) me = hipMemsetAsync(samples, 0, 4 * (size_t)T, s);
    if (me == hipSuccess && seams > 0) me = hipMemsetAsync(workspace, 0, 4 * trj_table_words(seams), s);
    if (me != hipSuccess) { (void)hipGetLastError(); return (int)me; }      // the memset's OWN error, never PWC_OK
    if (seams == 0) return pwc_launch_status();
    const bool vec = pwc_flow_vec(flow_cs | a.pcs, {flows, prev_flow});
    const dim3 parts((unsigned)pwc_loss_parts(H, W), (unsigned)seams), one((unsigned)seams);
    if (vec) hipLaunchKernelGGL(trj_keys_kernel<true>, parts, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(trj_keys_kernel<false>, parts, dim3(256), 0, s, a);
    hipLaunchKernelGGL(trj_select_kernel<0>, one, dim3(256), 0, s, a);
    hipLaunchKernelGGL(trj_hist_kernel<1>, parts, dim3(256), 0, s, a);
    hipLaunchKernelGGL(trj_select_kernel<1>, one, dim3(256), 0, s, a);
    hipLaunchKernelGGL(trj_hist_kernel<2>, parts, dim3(256), 0, s, a);
    hipLaunchKernelGGL(trj_select_kernel<2>, one, dim3(256), 0, s, a);
    return pwc_launch_status();
}

extern "C" int pwc_camera_trajectory_f64(const double* rotation, const double* translation, const float* ratio, const int32_t* samples,
                                         int T, int min_samples, const double* prev_rotation, const double* prev_row,
                                         const double* prev_scale, const int32_t* prev_segment, double* trajectory, double* scales,
                                         int32_t* segment, uint8_t* linked, int32_t* segment_state, pwc_stream_t stream) {
    if (!rotation || !translation || !ratio || !samples || !trajectory || !scales || !segment || !linked || !segment_state)
        return PWC_EINVAL;
    if (T < 1 || min_samples < 1) return PWC_EINVAL;
    if (prev_rotation && (!prev_row || !prev_scale || !prev_segment)) return PWC_EINVAL;
    if (T > 65535) return PWC_ERANGE;
    if (pwc_off(rotation, 7u) || pwc_off(translation, 7u) || pwc_off(prev_rotation, 7u) || pwc_off(prev_row, 7u) ||
        pwc_off(prev_scale, 7u) || pwc_off(trajectory, 7u) || pwc_off(scales, 7u) || pwc_off(ratio, 3u) || pwc_off(samples, 3u) ||
        pwc_off(prev_segment, 3u) || pwc_off(segment, 3u) || pwc_off(segment_state, 3u))
        return PWC_EALIGN;
    TrajectoryArgs a = {};
    a.rotation = rotation; a.translation = translation; a.ratio = ratio; a.samples = samples;
    a.protation = prev_rotation; a.prow = prev_row; a.pscale = prev_scale; a.psegment = prev_segment;
    a.trajectory = trajectory; a.scales = scales; a.segment = segment; a.linked = linked; a.segment_state = segment_state;
    a.T = T; a.min_samples = min_samples;
    hipLaunchKernelGGL(trj_chain_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    return pwc_launch_status();
}
