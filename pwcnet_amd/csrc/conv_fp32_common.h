// conv_fp32_common.h -- what the fp32-matrix-pipe convolutions share (conv3x3_mfma.hip, conv3x3_wino.hip, conv3x3_wino4.hip):
// the chunk swizzle of their 64-byte LDS rows, the weight packer, the reduce kernel of the tap split and of the channel split,
// the entry points' argument check and the packable subtraction of the Winograd transforms.
#pragma once
#include "pwc_common.h"

// 16-byte chunk c of a 64-byte row sits at slot c ^ pwc_swz4(row) = c ^ {0,3,2,1}[(row >> 2) & 3]: conflict-free for the four
// 16-lane groups a ds_read_b128 of one MFMA fragment (row = lane & 15, chunk = lane >> 4) is serviced in.
__host__ __device__ __forceinline__ int pwc_swz4(int row) { return (4 - ((row >> 2) & 3)) & 3; }

// -1.0f in an SGPR the optimiser cannot see through: p - q is written fma(q, -1, p) so that it
// can become one v_pk_fma_f32 per two floats (a vector fsub is scalarised by the backend: there
// is v_pk_add_f32 but no packed subtract).  The VALU instructions of the transforms share the
// issue port with the MFMAs and their time ADDS to the MFMA time (measured: removing the 128
// scalar transform instructions of a stage saved 10 % of the kernel).
// (Inline-asm v_pk_add_f32 with neg modifiers was tried: fully packed, same speed, but every
// VALU write an MFMA reads next needs 2 wait states that the hazard recogniser only inserts
// for instructions it can see -- results were wrong until the s_nop moved into the asm.)
__device__ __forceinline__ f32x4 pwc_minus_one4() {
    float m;
    asm volatile("s_mov_b32 %0, 0xbf800000" : "=s"(m));
    return f32x4{m, m, m, m};
}
__device__ __forceinline__ f32x4 pwc_sub4(f32x4 p, f32x4 q, f32x4 minus_one) { return __builtin_elementwise_fma(q, minus_one, p); }

// ---------------------------------------------------------------- weight packing
// packed[position][c16][Cout_pad][16]: element (j*4+e) of row `co` holds value(position, cin_map[c16*16 + (j ^ pwc_swz4(co))*4 + e], co)
// (0 for padding channels), i.e. the 16-byte chunk index is pre-swizzled so that the LDS image is a linear copy.  cin_map: the
// physical -> logical input channel map (null: identity).  `value` is what a family stores: a tap of w_hwio (conv3x3_mfma.hip)
// or an element of G g G^T (the Winograd kernels).
template <class Value>
__global__ void conv_fp32_pack_kernel(const float* __restrict__ w, const int32_t* __restrict__ cin_map, int positions, int Cin,
                                      int Cin_phys, int Cout, int Cout_pad, float* __restrict__ packed) {
    const size_t total = (size_t)positions * Cin_phys * Cout_pad;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int e16 = (int)(idx & 15);
        size_t r = idx >> 4;
        const int co = (int)(r % Cout_pad);
        r /= Cout_pad;
        const int c16 = (int)(r % (Cin_phys >> 4));
        const int pos = (int)(r / (Cin_phys >> 4));
        const int j = (e16 >> 2) ^ pwc_swz4(co), e = e16 & 3;
        const int cphys = c16 * 16 + j * 4 + e;
        const int clog = cin_map ? cin_map[cphys] : (cphys < Cin ? cphys : -1);
        packed[idx] = (clog >= 0 && clog < Cin && co < Cout) ? Value::at(w, pos, clog, co, Cin, Cout) : 0.f;
    }
}

static inline size_t conv_fp32_packed_floats(int positions, int Cin_phys, int Cout) {
    if (Cin_phys <= 0 || Cout <= 0) return 0;
    return (size_t)positions * Cin_phys * ((Cout + 15) & ~15);
}

template <class Value>
static inline int conv_fp32_pack(int positions, const float* w_hwio, const int32_t* cin_map, int Cin, int Cin_phys, int Cout,
                                 float* packed, pwc_stream_t stream) {
    if (!w_hwio || !packed || Cin <= 0 || Cout <= 0 || Cin_phys < Cin) return PWC_EINVAL;
    if (Cin_phys % 16) return PWC_EALIGN;
    const size_t total = conv_fp32_packed_floats(positions, Cin_phys, Cout);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(conv_fp32_pack_kernel<Value>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w_hwio, cin_map, positions,
                       Cin, Cin_phys, Cout, (Cout + 15) & ~15, packed);
    return pwc_launch_status();
}

// ---------------------------------------------------------------- split reduce
// y[pix][co] = act(bias[co] + sum_z ws[z][pix][co]) over the M pixels of the tap split's (conv3x3_mfma.hip) or the channel
// split's (conv3x3_wino.hip) raw partial sums; z summed in a fixed order, so the result is deterministic.
template <int T = 256>
__global__ __launch_bounds__(T) void conv_fp32_split_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ bias,
                                                                   float* __restrict__ y, int y_cs, int y_vec4, long M, int Cout,
                                                                   int Cout_pad, int nsplit, int apply_act, float slope) {
    const int c4n = Cout >> 2;
    const long total = M * c4n;
    for (long idx = (long)blockIdx.x * T + threadIdx.x; idx < total; idx += (long)gridDim.x * T) {
        const int c4 = (int)(idx % c4n);
        const long pix = idx / c4n;
        f32x4 v = *reinterpret_cast<const f32x4*>(bias + c4 * 4);
        for (int z = 0; z < nsplit; ++z) v += *reinterpret_cast<const f32x4*>(ws + ((size_t)z * M + pix) * Cout_pad + c4 * 4);
        if (apply_act) v = pwc_lrelu4(v, slope);
        float* dst = y + (size_t)pix * y_cs + c4 * 4;
        if (y_vec4) *reinterpret_cast<f32x4*>(dst) = v;
        else { dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3]; }
    }
}

static inline bool conv_fp32_y_vec4(const float* y, int y_cs) { return (y_cs & 3) == 0 && pwc_aligned16(y); }

// max_blocks: each call site keeps the grid cap it was measured with
static inline void conv_fp32_split_reduce(const float* ws, const float* bias, float* y, int y_cs, long M, int Cout, int nsplit,
                                          int apply_act, float slope, long max_blocks, hipStream_t stream) {
    long blocks = (M * (Cout >> 2) + 255) / 256;
    if (blocks > max_blocks) blocks = max_blocks;
    hipLaunchKernelGGL(conv_fp32_split_reduce_kernel<256>, dim3((unsigned)blocks), dim3(256), 0, stream, ws, bias, y, y_cs,
                       conv_fp32_y_vec4(y, y_cs) ? 1 : 0, M, Cout, (Cout + 15) & ~15, nsplit, apply_act, slope);
}

// ---------------------------------------------------------------- argument check
// The rules the three entry points share, in the order they report (pwc_conv_io_check): a dilation below 1 is PWC_EINVAL like
// a bad size, channel counts that are no multiples of 16 are PWC_EUNSUPPORTED.  y_aligned: F(4x4) stores 16 bytes at a time;
// the other two fall back to scalar stores (conv_fp32_y_vec4).  The PWC_ERANGE rules stay with each family.
static inline int conv_fp32_io_check(const float* x, int x_cs, const float* packed, const float* bias, const float* y, int y_cs,
                                     int N, int H, int W, int Cin_phys, int Cout, int dilation, bool y_aligned) {
    if (dilation < 1) return PWC_EINVAL;
    return pwc_conv_io_check(x, x_cs, Cin_phys, y, y_cs, Cout, packed, bias, N, H, W, !(Cin_phys % 16 || Cout % 16), y_aligned);
}
