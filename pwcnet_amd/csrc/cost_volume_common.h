// cost_volume_common.h -- what the correlation kernels of cost_volume*.hip share: argument checks and launch plumbing on the
// host; on the device the F16-matrix-pipe pieces of cost_volume_h2.hip / cost_volume_blk.hip.
// (The bilinear corner table and its blend are in pwc_common.h: the stand-alone warps use them too.)
#pragma once
#include "pwc_common.h"
#include <type_traits>

#define CVM_OOB 0x80000000u            // a byte offset no buffer resource covers: the load returns zeros, the store is dropped
typedef unsigned int cvm_u32x4 __attribute__((ext_vector_type(4)));

// f(std::integral_constant<int, i>{}) for i = 0 .. N-1
template <int N, int I = 0, class F>
__device__ __forceinline__ void cvm_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        cvm_for<N, I + 1>(f);
    }
}

// ---------------------------------------------------------------- host: checks
// The argument checks every correlation entry point shares, in the order they report: null pointers and non-positive sizes
// (PWC_EINVAL), a search range outside r_min .. 4 (PWC_EUNSUPPORTED), a channel stride below the channel count or an `out`
// record below (2R+1)^2 floats -- and the family's further stride rules, `strides_ok` false -- (PWC_EINVAL), C or a stride of
// f0 / f1 that is not whole 16-byte quads and f0 / f1 off a 16-byte boundary (PWC_EALIGN).  What a family checks besides stays
// with it, in front of or behind this call as the code it reports has to win or lose.
static inline int cv_io_check(const float* f0, int f0_cs, const float* f1, int f1_cs, const float* out, int out_cs, int N, int H,
                              int W, int C, int R, int r_min, bool strides_ok = true) {
    if (!f0 || !f1 || !out) return PWC_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return PWC_EINVAL;
    if (R < r_min || R > 4) return PWC_EUNSUPPORTED;
    if (f0_cs < C || f1_cs < C || out_cs < (2 * R + 1) * (2 * R + 1) || !strides_ok) return PWC_EINVAL;
    if ((C & 3) || (f0_cs & 3) || (f1_cs & 3) || !pwc_aligned16(f0) || !pwc_aligned16(f1)) return PWC_EALIGN;
    return PWC_OK;
}

// The kernels that address every operand through per-image buffer resources (cost_volume_mfma / _h2 / _blk.hip): search range 4,
// a channel count of the family (`channels`), whole 16-byte quads everywhere, a 4-byte aligned flow, and byte extents of one
// image below 2^31 (the out-of-range marker).
static inline bool cv_rsrc_eligible(const float* f0, int f0_cs, const float* f1, int f1_cs, const float* flow, int flow_cs,
                                    const float* out, int out_cs, const float* f0_copy, int f0_copy_cs, int H, int W, int C, int R,
                                    bool (*channels)(int)) {
    if (R != 4 || !channels(C)) return false;
    if ((f0_cs & 3) || (f1_cs & 3) || (out_cs & 3) || !pwc_aligned16(f0) || !pwc_aligned16(f1) || !pwc_aligned16(out)) return false;
    if (f0_copy && ((f0_copy_cs & 3) || !pwc_aligned16(f0_copy))) return false;
    if (flow && (reinterpret_cast<uintptr_t>(flow) & 3u)) return false;
    const long px = (long)H * W;
    if (px * f0_cs * 4 >= (1L << 31) || px * f1_cs * 4 >= (1L << 31) || px * out_cs * 4 >= (1L << 31)) return false;
    if (f0_copy && px * f0_copy_cs * 4 >= (1L << 31)) return false;
    if (flow && px * flow_cs * 4 >= (1L << 31)) return false;
    return true;
}

// The checks of the three warp + cost volume + concat entry points, in the order they report.  `pad2` says whether the family
// takes out_pad_writable == 2 (the flow in channels 81, 82: cost_volume_h2.hip only).
static inline int cv_concat_check(const float* f0, int f0_cs, const float* f1, int f1_cs, const float* flow, int flow_cs,
                                  const float* out, int out_cs, int out_pad_writable, const float* f0_copy, int f0_copy_cs, int N,
                                  int H, int W, int C, int R, bool pad2, bool (*channels)(int)) {
    const int rc = cv_io_check(f0, f0_cs, f1, f1_cs, out, out_cs, N, H, W, C, R, 1);
    if (rc) return rc;
    if ((flow && flow_cs < 2) || (f0_copy && f0_copy_cs < C)) return PWC_EINVAL;
    if (out_pad_writable && out_cs < 84) return PWC_EINVAL;
    if (out_pad_writable == 2 && !pad2) return PWC_EUNSUPPORTED;
    if (R != 4 || !channels(C)) return PWC_EUNSUPPORTED;
    if (!cv_rsrc_eligible(f0, f0_cs, f1, f1_cs, flow, flow_cs, out, out_cs, f0_copy, f0_copy_cs, H, W, C, R, channels))
        return ((long)H * W * (long)(out_cs > f0_cs ? out_cs : f0_cs) * 4 >= (1L << 31)) ? PWC_ERANGE : PWC_EALIGN;
    return PWC_OK;
}

// ---------------------------------------------------------------- host: launch
// The operand fields CvmArgs (cost_volume_mfma.hip, cost_volume_h2.hip) and CvbArgs (cost_volume_blk.hip) have in common.
template <class Args>
static inline Args cv_rsrc_args(const float* f0, int f0_cs, const float* f1, int f1_cs, const float* flow, int flow_cs,
                                float flow_scale, float* out, int out_cs, int pad_ok, float* f0_copy, int f0_copy_cs, int N, int H,
                                int W, int C, float slope) {
    Args a;
    a.f0 = f0; a.f1 = f1; a.flow = flow; a.out = out; a.f0_copy = f0_copy;
    a.f0_cs = f0_cs; a.f1_cs = f1_cs; a.flow_cs = flow_cs; a.out_cs = out_cs; a.f0_copy_cs = f0_copy_cs;
    a.N = N; a.H = H; a.W = W; a.flow_scale = flow_scale; a.slope = slope;
    a.inv_c = 1.0f / (float)C;               // reduce_mean: x * (1/C), within 1 ulp of x / C
    a.pad_ok = pad_ok;
    return a;
}

// launch(cg, warp, pad) -- three integral constants -- for the channel count C = 16 cg among CGS, warp = a flow is given,
// pad = channels 81..83 of the `out` records are the kernel's to write.
template <int... CGS, class F>
static inline int cv_dispatch_cg(int C, bool warp, bool pad, F&& launch) {
    int rc = PWC_EUNSUPPORTED;
    auto one = [&](auto cg) {
        if (C != 16 * decltype(cg)::value) return false;
        rc = warp ? (pad ? launch(cg, std::true_type{}, std::true_type{}) : launch(cg, std::true_type{}, std::false_type{}))
                  : (pad ? launch(cg, std::false_type{}, std::true_type{}) : launch(cg, std::false_type{}, std::false_type{}));
        return true;
    };
    (void)(one(std::integral_constant<int, CGS>{}) || ...);
    return rc;
}

// ---------------------------------------------------------------- device
// The f0 operand of a 4 x 4 block, 2 NP channel quads per lane, as the two-term fp16 split in MFMA layout: k slot e of lane
// quarter kq = channel 32 j + 4 kq + e for e < 4, 32 j + 16 + 4 kq + e - 4 else -- what the Q images hold.
template <int NP>
__device__ __forceinline__ void cv_split_rows(const f32x4* A, pwc_f16x8* AH, pwc_f16x8* AM) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        pwc_f16x4 h0, m0, h1, m1;
        pwc_split4(A[2 * j], h0, m0);
        pwc_split4(A[2 * j + 1], h1, m1);
        AH[j] = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
        AM[j] = __builtin_shufflevector(m0, m1, 0, 1, 2, 3, 4, 5, 6, 7);
    }
}

// leaky-relu max(x, slope * x) of a quad: ONE v_max_f32 per value (fmaxf costs a second one that quiets a possible signalling
// NaN first; fmed3 with +inf is folded back into fmaxf).  The multiply in front is compiler-visible and reads the same registers.
__device__ __forceinline__ f32x4 cv_lrelu_quad(const f32x4 v, const float slope) {
    const f32x4 sv = v * slope;
    f32x4 y;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float yk;
        asm("v_max_f32 %0, %1, %2" : "=v"(yk) : "v"(v[k]), "v"(sv[k]));
        y[k] = yk;
    }
    return y;
}
