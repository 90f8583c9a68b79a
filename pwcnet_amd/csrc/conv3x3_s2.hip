// conv3x3_s2.hip -- stride-2 3x3 convolution (+ bias, + leaky-relu) for FULL-CHIP launches on the F16 matrix pipe: the strided
// tile kernel behind pwc_conv3x3_sk_f32 (fp_extractor/conv2d_9, 64 -> 96) and pwc_conv3x3_h2_stride2_f32 (conv2d_6, 32 -> 64).
// libpwc_hip.so, gfx950 only.
//
// Replaces (reference modules.py:57-60, the extractor's down-sampling layers): tf.layers.Conv2D(f, (3, 3), 2, 'same') +
// LeakyReLU(0.1) on NHWC fp32.
//
// Why another kernel.  The two families that served these layers are shaped for other launches: conv3x3_sk deals K to the eight
// waves of a workgroup that owns 32 pixels x 32 output channels -- every workgroup fetches its tile's whole weights, the patch is
// fetched once per output-channel tile -- and the parity-plane form of conv3x3_h2 walks 4 C / 16 stages with 4 of 9 tap slots in
// use (16 C products per output, the stage's fixed cost each time).  Here a workgroup owns 4 rows x 32 columns of output pixels
// and ALL output channels:
//   * the input patch (9 rows x 65 columns, 64 channels at a time) is fetched once, as whole lines, split once into h | m'
//     (pwc_split4) and written to the LDS de-interleaved by column parity: [patch row][16 channels][h | m'][33 even columns, 32 odd
//     columns][16 fp16].  Tap dx of output column c is even column c, odd column c, even column c + 1: the 16 pixels of a fragment
//     are 16 neighbouring 32-byte records at every tap, and the four 16-lane groups of a ds_read_b128 each cover all 64 banks
//     (lanes kq = 2 i and 2 i + 1 read the two 16-byte halves of a record);
//   * wave w owns output row w / 2 (two 16-pixel fragments) and one half of the output-channel blocks: pixels and channels are
//     dealt, not K, so each output has ONE accumulation chain over K in a fixed order (launches repeat bitwise) and nothing is
//     reduced across waves;
//   * weights are read in the pwc_conv3x3_sk_pack_f32 layout as it is, one K step (tap x 32 channels) ahead, straight into
//     registers; they are the ROW operand of the matrix instruction and the pixels the column operand, so a lane ends up with four
//     neighbouring output channels of one pixel: 16-byte stores without a transpose.
// Nine real taps: 9 C products per output.
//
// Arithmetic: the two-term fp16 split of conv3x3_h2.hip (x = h + 2^-11 m', three v_mfma_f32_16x16x32_f16 per K step and tile,
// fp32 accumulation: hh and the cross terms in separate accumulators, combined once in the epilogue).  RANGE as there: |x|, |w| <
// 65520, beyond: NaN on the outputs that read the operand.  C_in (physical) % 32 == 0, C_out % 16 == 0, C_out <= 128.
#include "pwc_common.h"

typedef unsigned int s2_u32x4 __attribute__((ext_vector_type(4)));
#define S2_OOB 0x80000000u

constexpr int S2_PC = 2 * PWC_S2_TILE_COLS + 1;             // patch columns (65): 33 even, 32 odd
constexpr int S2_PR = 2 * PWC_S2_TILE_ROWS + 1;             // patch rows (9)
constexpr int S2_NPX = S2_PR * S2_PC;
constexpr int S2_EVEN = PWC_S2_TILE_COLS + 1;               // records of the even-column plane, the odd columns follow
constexpr int S2_LINE = S2_PC * 32;                         // bytes of a (patch row, 16 channels, h | m') line of 32-byte records
constexpr int S2_CC = 64;                                   // channels of the patch that are in the LDS at a time
constexpr int S2_UB = 5;                                    // 8-channel units a thread requests at a time

struct S2Args {
    const float* x;
    const float* wp;        // packed split weights (pwc_conv3x3_sk_pack_f32): [C_out / 16][nsteps][h | m'][64 lanes][8 fp16]
    const float* bias;
    float* y;
    int x_cs, y_cs;
    int N, H, W, Ho, Wo;
    int Cin_phys, Cout;
    int pad_t, pad_l;
    int apply_act;
    float slope;
    int ntx, nty;           // tiles per image row / column
    int cg;                 // C_in / 32
    int nsteps;             // 9 cg
};

// NBW: 16-channel output blocks of a wave (the workgroup's two wave columns hold 2 NBW >= C_out / 16 of them)
template <int NBW>
__global__ __launch_bounds__(512) void conv3x3_s2_kernel(const S2Args a) {
    extern __shared__ __attribute__((aligned(16))) char s2_smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    int b = blockIdx.x;
    const int tx = b % a.ntx;
    b /= a.ntx;
    const int ty = b % a.nty, n = b / a.nty;

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.x, 0, (int)((size_t)a.N * a.H * a.W * a.x_cs * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.wp, 0, (int)((size_t)a.Cout * a.nsteps * 128), 0x00020000);
    const int m = lane & 15, kq = lane >> 4;
    const int row = wave >> 1, cb0 = (wave & 1) * NBW, nb = a.Cout >> 4;

    f32x4 hh[2][NBW], xx[2][NBW];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int j = 0; j < NBW; ++j) {
            hh[hf][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            xx[hf][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

    // K step s (global index: tap x C_in / 32 + channel group) of this wave's output blocks; a block past C_out reads zeros
    auto fetch_b = [&](s2_u32x4 (&bv)[NBW][2], int s, bool live) {
#pragma unroll
        for (int j = 0; j < NBW; ++j) {
            const int cb = cb0 + j;
            const unsigned vo = (live && cb < nb) ? (unsigned)((cb * a.nsteps + s) * 2048 + lane * 16) : S2_OOB;
            bv[j][0] = __builtin_amdgcn_raw_buffer_load_b128(rw, (int)vo, 0, 0);
            bv[j][1] = __builtin_amdgcn_raw_buffer_load_b128(rw, (int)vo, 1024, 0);
        }
    };

    const int gy0 = 2 * PWC_S2_TILE_ROWS * ty - a.pad_t, gx0 = 2 * PWC_S2_TILE_COLS * tx - a.pad_l;
    for (int c0 = 0; c0 < a.Cin_phys; c0 += S2_CC) {
        const int cc = a.Cin_phys - c0 < S2_CC ? a.Cin_phys - c0 : S2_CC;          // 32 or 64
        const int cgc = cc >> 5, ng16 = cc >> 4, cqs = 1 + cgc;                      // 8-channel units per pixel: 1 << cqs
        const int nst = 9 * cgc, sbase = c0 >> 5;
        auto gstep = [&](int si) { const int tap = si / cgc; return tap * a.cg + sbase + (si - tap * cgc); };
        if (c0) __syncthreads();                                                     // (every wave is done with the last patch)
        s2_u32x4 b0[NBW][2], b1[NBW][2];
        fetch_b(b0, gstep(0), true);                                                 // lands under the patch fetch
        // ---- the patch: unit u = (pixel u >> cqs, 8 channels), neighbouring lanes ask for neighbouring bytes of a line
        const int nu = S2_NPX << cqs;
#pragma unroll 1
        for (int u0 = t; u0 < nu; u0 += 512 * S2_UB) {
            f32x4 v[S2_UB][2];
            int dst[S2_UB];
#pragma unroll
            for (int k = 0; k < S2_UB; ++k) {
                const int u = u0 + 512 * k;
                const int px = u >> cqs, j = u - (px << cqs);
                const int pr = px / S2_PC, pc = px - pr * S2_PC;
                const int gy = gy0 + pr, gx = gx0 + pc;
                const bool ok = u < nu && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
                const unsigned vo = ok ? (unsigned)(((n * a.H + gy) * a.W + gx) * a.x_cs + c0 + j * 8) * 4u : S2_OOB;
                v[k][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, (int)vo, 0, 0));
                v[k][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, (int)vo, 16, 0));
                const int pos = (pc & 1) ? S2_EVEN + (pc >> 1) : pc >> 1;
                dst[k] = u < nu ? ((pr * ng16 + (j >> 1)) * 2) * S2_LINE + pos * 32 + (j & 1) * 16 : -1;
            }
#pragma unroll
            for (int k = 0; k < S2_UB; ++k)
                if (dst[k] >= 0) {
                    pwc_f16x4 h0, m0, h1, m1;
                    pwc_split4(v[k][0], h0, m0);
                    pwc_split4(v[k][1], h1, m1);
                    *reinterpret_cast<pwc_f16x8*>(s2_smem + dst[k]) = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
                    *reinterpret_cast<pwc_f16x8*>(s2_smem + dst[k] + S2_LINE) = __builtin_shufflevector(m0, m1, 0, 1, 2, 3, 4, 5, 6, 7);
                }
        }
        __syncthreads();

        // ---- K loop: step si = (tap, 32 channels of the patch), weights one step ahead
        auto step = [&](const s2_u32x4 (&bv)[NBW][2], int si) {
            const int tap = si / cgc, c32 = si - tap * cgc;
            const int dy = tap / 3, dx = tap - 3 * dy;
            const int pos = (dx == 1 ? S2_EVEN : 0) + (dx >> 1) + m;
            const char* p = s2_smem + (((2 * row + dy) * ng16 + 2 * c32 + (kq >> 1)) * 2) * S2_LINE + pos * 32 + (kq & 1) * 16;
            pwc_f16x8 ah[2], am[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                ah[hf] = *reinterpret_cast<const pwc_f16x8*>(p + hf * 512);
                am[hf] = *reinterpret_cast<const pwc_f16x8*>(p + hf * 512 + S2_LINE);
            }
#pragma unroll
            for (int j = 0; j < NBW; ++j) {
                const pwc_f16x8 wh = __builtin_bit_cast(pwc_f16x8, bv[j][0]);
                const pwc_f16x8 wm = __builtin_bit_cast(pwc_f16x8, bv[j][1]);
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    xx[hf][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wm, ah[hf], xx[hf][j], 0, 0, 0);
                    hh[hf][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, ah[hf], hh[hf][j], 0, 0, 0);
                    xx[hf][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, am[hf], xx[hf][j], 0, 0, 0);
                }
            }
        };
#pragma unroll 1
        for (int si = 0; si < nst; si += 2) {
            fetch_b(b1, gstep(si + 1 < nst ? si + 1 : 0), si + 1 < nst);
            step(b0, si);
            fetch_b(b0, gstep(si + 2 < nst ? si + 2 : 0), si + 2 < nst);
            if (si + 1 < nst) step(b1, si + 1);
        }
    }

    // ---- D fragment = (output channel 4 kq + r of the block, pixel m): bias, leaky-relu, one 16-byte store per block
    const int oy = PWC_S2_TILE_ROWS * ty + row;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        const int ox = PWC_S2_TILE_COLS * tx + hf * 16 + m;
        if (oy < a.Ho && ox < a.Wo) {
            float* yp = a.y + ((size_t)(n * a.Ho + oy) * a.Wo + ox) * a.y_cs + 4 * kq;
#pragma unroll
            for (int j = 0; j < NBW; ++j) {
                const int cb = cb0 + j;
                if (cb < nb) {
                    f32x4 v = __builtin_elementwise_fma(xx[hf][j], f32x4{1.f / 2048.f, 1.f / 2048.f, 1.f / 2048.f, 1.f / 2048.f}, hh[hf][j]);
                    v += *reinterpret_cast<const f32x4*>(a.bias + cb * 16 + 4 * kq);
                    if (a.apply_act) v = pwc_lrelu4(v, a.slope);
                    *reinterpret_cast<f32x4*>(yp + cb * 16) = v;
                }
            }
        }
    }
}

template <int NBW>
static int s2_launch(const S2Args& a, hipStream_t s) {
    const long wgs = (long)a.N * a.nty * a.ntx;
    if (wgs >= (1L << 31)) return PWC_ERANGE;
    const int cc = a.Cin_phys < S2_CC ? a.Cin_phys : S2_CC;
    pwc_allow_dynamic_lds<&conv3x3_s2_kernel<NBW>>(S2_NPX * S2_CC * 4);
    hipLaunchKernelGGL((conv3x3_s2_kernel<NBW>), dim3((unsigned)wgs), dim3(512), (size_t)S2_NPX * cc * 4, s, a);
    return pwc_launch_status();
}

bool pwc_conv3x3_s2_tile_admits(int N, int H, int W, int x_cs, int Cin_phys, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin_phys <= 0 || Cout <= 0 || x_cs < Cin_phys) return false;
    if (Cin_phys % 32 || Cout % 16 || Cout > 128) return false;
    return pwc_fits_2g(N, H, W, x_cs) && (long)Cout * 9 * (Cin_phys / 32) * 128 < (1L << 31);
}

long pwc_conv3x3_s2_tile_count(int N, int H, int W) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    return (long)N * ((Ho + PWC_S2_TILE_ROWS - 1) / PWC_S2_TILE_ROWS) * ((Wo + PWC_S2_TILE_COLS - 1) / PWC_S2_TILE_COLS);
}

// The callers (sk_run, h2_run) have checked pointers, strides and alignment by their own rules; the shape by _admits.
int pwc_conv3x3_s2_tile_launch(const float* x, int x_cs, const float* packed_w, const float* bias, float* y, int y_cs, int N, int H,
                               int W, int Cin_phys, int Cout, int apply_act, float slope, pwc_stream_t stream) {
    if (!pwc_conv3x3_s2_tile_admits(N, H, W, x_cs, Cin_phys, Cout)) return PWC_EUNSUPPORTED;
    S2Args a;
    a.x = x; a.wp = packed_w; a.bias = bias; a.y = y; a.x_cs = x_cs; a.y_cs = y_cs;
    a.N = N; a.H = H; a.W = W;
    pwc_same_pad(H, 2, 1, &a.Ho, &a.pad_t);
    pwc_same_pad(W, 2, 1, &a.Wo, &a.pad_l);
    a.Cin_phys = Cin_phys; a.Cout = Cout; a.apply_act = apply_act; a.slope = slope;
    a.ntx = (a.Wo + PWC_S2_TILE_COLS - 1) / PWC_S2_TILE_COLS;
    a.nty = (a.Ho + PWC_S2_TILE_ROWS - 1) / PWC_S2_TILE_ROWS;
    a.cg = Cin_phys / 32; a.nsteps = 9 * a.cg;
    hipStream_t s = (hipStream_t)stream;
    switch ((Cout / 16 + 1) / 2) {
        case 1: return s2_launch<1>(a, s);
        case 2: return s2_launch<2>(a, s);
        case 3: return s2_launch<3>(a, s);
        default: return s2_launch<4>(a, s);
    }
}

#ifdef PWC_HARNESS
// libpwc_hip_harness.so only: 0 = the entry points' own routing, 1 = the strided tile kernel wherever the shape admits it,
// -1 = never (A/B runs of a model forward).
static int s2_tile_mode = 0;
extern "C" int pwc_debug_conv3x3_s2_tile(int mode) { s2_tile_mode = mode; return 0; }
int pwc_conv3x3_s2_tile_debug_mode() { return s2_tile_mode; }
#endif
