// pwc_common.h -- shared device/host helpers for libpwc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pwc_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 pwc_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 pwc_f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 pwc_f16x2 __attribute__((ext_vector_type(2)));

#define PWC_WAVE 64

static inline int pwc_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PWC_OK : (int)e;
}

// "Set the dynamic-LDS ceiling of this kernel once per device", in front of a launch.  hipFuncAttributeMaxDynamicSharedMemorySize
// is a PER-DEVICE attribute: one flag per kernel and device (a process that uses the library on a second GPU must set it there
// too).  Idempotent, benign if raced.  The template is instantiated per kernel POINTER, not per kernel type -- the
// instantiations of a kernel template share a type.
template <auto Kernel>
static inline void pwc_allow_dynamic_lds(int bytes) {
    static unsigned long long done[4] = {0, 0, 0, 0};
    int d = 0;
    if (hipGetDevice(&d) == hipSuccess && d >= 0 && d < 256) {                  // (unknown device: just set it again)
        const unsigned long long bit = 1ull << (d & 63);
        if (done[d >> 6] & bit) return;
        done[d >> 6] |= bit;
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// Compute units of the current device, asked once per device (256 where the runtime cannot say): the grid of the persistent kernels.
static inline int pwc_cu_count() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cus[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

// The flat grid of the one-lane-per-item kernels: workgroups of 256 lanes over `items`, at most 4096 (grid-stride beyond).
static inline dim3 pwc_flat_grid(long items) {
    const long blocks = (items + 255) / 256;
    return dim3((unsigned)(blocks > 4096 ? 4096 : blocks));
}

// Whether p is off the boundary of mask + 1 bytes.
static inline bool pwc_off(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
static inline bool pwc_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The argument checks the conv entry points share (F16 and fp32 matrix pipe), in the order they report: null pointers and non-positive
// sizes (PWC_EINVAL), the family's own shape rule (`supported` false: PWC_EUNSUPPORTED), a channel stride below the channel
// count (PWC_EINVAL), channel strides that are not whole 16-byte chunks and pointers off a 16-byte boundary (PWC_EALIGN).
// y_aligned false: the kernel falls back to scalar stores, y and y_cs need no alignment.
// What a family checks besides -- stride and dilation, further operands, the 32-bit range of ITS buffer resources -- stays with
// it, in front of or behind this call as the code it reports has to win or lose.
static inline int pwc_conv_io_check(const void* x, int x_cs, int Cin_phys, const void* y, int y_cs, int Cout, const void* packed_w,
                                    const void* bias, int N, int H, int W, bool supported, bool y_aligned = true) {
    if (!x || !packed_w || !bias || !y) return PWC_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || Cin_phys <= 0 || Cout <= 0) return PWC_EINVAL;
    if (!supported) return PWC_EUNSUPPORTED;
    if (x_cs < Cin_phys || y_cs < Cout) return PWC_EINVAL;
    if ((x_cs & 3) || !pwc_aligned16(x) || !pwc_aligned16(packed_w) || !pwc_aligned16(bias)) return PWC_EALIGN;
    if (y_aligned && ((y_cs & 3) || !pwc_aligned16(y))) return PWC_EALIGN;
    return PWC_OK;
}
// The out-of-range byte offset of the kernels whose buffer resources cover one image of less than PWC_OOB bytes: a load from it
// returns zeros (the SAME padding), a store to it is dropped.
constexpr unsigned PWC_OOB = 0x7FFF0000u;
// A whole tensor behind ONE buffer resource with 32-bit byte offsets (an out-of-range offset, 2^31, is how a lane asks for
// zeros): n x h x w records of cs floats must end below 2^31 bytes.
static inline bool pwc_fits_2g(long n, long h, long w, long cs) { return n * h * w * cs * 4 < (1L << 31); }

// TF 'SAME' padding of one axis for a 3-tap kernel (see include/pwc_hip.h, conv).
static inline void pwc_same_pad(int in, int stride, int dil, int* out, int* before) {
    int o = (in + stride - 1) / stride;
    int total = (o - 1) * stride + 2 * dil + 1 - in;
    if (total < 0) total = 0;
    *out = o;
    *before = total / 2;
}

// a * b rounded to fp32 and NOT contractible into a following add/sub (hipcc fuses `a * b - c` into
// one fma otherwise -- __fmul_rn does not stop that): the reference computes such products as ops of
// their own (resize coordinate in = i * scale, flow * scale), floor / fraction come from the ROUNDED value
__device__ __forceinline__ float pwc_mul_rounded(float a, float b) {
    float r = a * b;
    asm volatile("" : "+v"(r));
    return r;
}

// ---- the corner table of the bilinear warp (bilinear_warp, reference modules.py:107-137), for pixel (gy, gx) of an
// H x W image and its displacement (fx, fy) = flow * scale, BOTH already rounded products (pwc_mul_rounded: model.py:109 is an
// op of its own).  The weights come from the UN-clipped floors, the four corner coordinates are clipped independently -- at the
// image edge two corners may be the same pixel while their weights still differ.  The forward warps (warp_kernel, the fused
// gathers of cost_volume.hip, cost_volume_mfma.hip, cost_volume_h2.hip) take their corners from here; what a site does with them
// -- byte or float offsets, out-of-image pixels, the 1/C of the mean -- is its own.  Two kernels spell the same operations out
// because their device code changed through this function: the table block of cost_volume_blk_kernel and warp_grad_kernel.
struct PwcCorners {
    int y0, y1, x0, x1;               // clipped rows / columns of the corners (y0, x0), (y0, x1), (y1, x0), (y1, x1)
    f32x4 w;                          // the corners' weights, in that order
};
__device__ __forceinline__ PwcCorners pwc_bilinear_corners(int gy, int gx, float fx, float fy, int H, int W) {
    const float fx0 = floorf(fx), fy0 = floorf(fy);
    const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
    const float hl = (float)(H - 1), wl = (float)(W - 1);
    PwcCorners k;
    k.y0 = (int)fminf(fmaxf((float)gy + fy0, 0.f), hl);
    k.y1 = (int)fminf(fmaxf((float)gy + fy1, 0.f), hl);
    k.x0 = (int)fminf(fmaxf((float)gx + fx0, 0.f), wl);
    k.x1 = (int)fminf(fmaxf((float)gx + fx1, 0.f), wl);
    k.w = f32x4{(fy1 - fy) * (fx1 - fx), (fy1 - fy) * (fx - fx0), (fy - fy0) * (fx1 - fx), (fy - fy0) * (fx - fx0)};
    return k;
}
// modules.py:132-135: c00*x00 + c01*x01 + c10*x10 + c11*x11, summed left to right (one multiply, three fused multiply-adds)
__device__ __forceinline__ f32x4 pwc_blend_corners(f32x4 w, f32x4 x00, f32x4 x01, f32x4 x10, f32x4 x11) {
    f32x4 v = w[0] * x00;
    v = __builtin_elementwise_fma(f32x4{w[1], w[1], w[1], w[1]}, x01, v);
    v = __builtin_elementwise_fma(f32x4{w[2], w[2], w[2], w[2]}, x10, v);
    v = __builtin_elementwise_fma(f32x4{w[3], w[3], w[3], w[3]}, x11, v);
    return v;
}

// ---- the bilinear corner table in doubles (the flow consumers, the label-free losses) of a position (sx, sy) INSIDE an H x W
// image -- the caller's own inside test is what keeps the four reads in the image: the corners (y0, x0), (y0, x1), (y1, x0),
// (y1, x1) as pixel offsets within the image, x1 and y1 clipped to the last column and row, and the weights along x and y from the
// floors.  The inside test and the blend stay with each site.
struct PwcBilinearF64 {
    size_t o00, o01, o10, o11;
    double wx0, wx1, wy0, wy1;
};
__device__ __forceinline__ PwcBilinearF64 pwc_bilinear_f64(double sx, double sy, int H, int W) {
    const double fx0 = floor(sx), fy0 = floor(sy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    PwcBilinearF64 k;
    k.wx1 = sx - fx0; k.wy1 = sy - fy0; k.wx0 = 1.0 - k.wx1; k.wy0 = 1.0 - k.wy1;
    k.o00 = (size_t)y0 * W + x0; k.o01 = (size_t)y0 * W + x1; k.o10 = (size_t)y1 * W + x0; k.o11 = (size_t)y1 * W + x1;
    return k;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() carries a fence over global memory as well, which
// hipcc lowers to `s_waitcnt vmcnt(0)` in front of the s_barrier: every LDS-DMA piece (buffer_load ... lds) and every
// store in flight is drained at each barrier, and a software pipeline that waits for its pieces with counted
// `s_waitcnt vmcnt(n)` is silently serialised (found in round 3 in the ISA of conv3x3_wino_kernel: all three barriers
// of a stage were preceded by vmcnt(0)).  A wave must have waited for its OWN pieces of a region (s_waitcnt vmcnt)
// before this barrier publishes the region to the other waves.
// (Second finding, late in round 3: a workgroup-scope fence on the "local" address space is lowered to vmcnt(0) too -- the
// backend counts buffer_load ... lds as LDS writes -- so this barrier drains the LDS-DMA pipeline just the same and the
// counted waits in front of it only matter for what they guarantee, not for overlap.  PWC_FENCE_BARRIER=0 spells the barrier
// out instead (`s_waitcnt lgkmcnt(0); s_barrier` with a "memory" clobber): the counted waits then really leave fetches in
// flight across barriers -- checked in the ISA, results identical on every harness shape -- and the fetch/LDS skeleton of the
// F(4x4) kernel drops from 154 to 134 us, but the complete kernels do not move (F(4x4) 252 against 247 us, F(2x2) 296
// against 290 us): fetch time adds to MFMA time on gfx950 whether or not it is in flight early.  The fence
// form stays the default.)
#ifndef PWC_FENCE_BARRIER
#define PWC_FENCE_BARRIER 1
#endif
// The spelled-out form: this wave's LDS operations are complete, then the barrier -- fetches and stores in flight stay in flight.
__device__ __forceinline__ void pwc_lds_barrier_raw() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void pwc_lds_barrier() {
#if PWC_FENCE_BARRIER
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
#else
    pwc_lds_barrier_raw();
#endif
}

// s_waitcnt vmcnt(n) only (gfx9 encoding: vmcnt [3:0] + [15:14], expcnt [6:4], lgkmcnt [11:8]): the counted wait of the
// software pipelines over buffer_load ... lds pieces
#define PWC_WAIT_VM(n) __builtin_amdgcn_s_waitcnt(((n) & 15) | (((n) >> 4) << 14) | (7 << 4) | (15 << 8))

__device__ __forceinline__ float pwc_lrelu(float v, float slope) {
    // tf.nn.leaky_relu(x, alpha) = max(alpha*x, x)
    return fmaxf(v, slope * v);
}
// ... of four values.  Two spellings of the same values, because each kernel's device code changed through the other one: the
// MFMA, direct and reduce kernels multiply per element (four v_mul_f32 that the scheduler places between the stores), the
// Winograd epilogues multiply the vector (two v_pk_mul_f32: their VALU time adds to the MFMA time, see conv3x3_wino.hip).
__device__ __forceinline__ f32x4 pwc_lrelu4(f32x4 v, float slope) {
    return f32x4{pwc_lrelu(v[0], slope), pwc_lrelu(v[1], slope), pwc_lrelu(v[2], slope), pwc_lrelu(v[3], slope)};
}
__device__ __forceinline__ f32x4 pwc_lrelu4_packed(f32x4 v, float slope) {
    const f32x4 sv = v * slope;
    return f32x4{fmaxf(v[0], sv[0]), fmaxf(v[1], sv[1]), fmaxf(v[2], sv[2]), fmaxf(v[3], sv[3])};
}

// Bijective XCD-aware remap of a linear workgroup id (MI355X: 8 XCDs, block b is
// dispatched to XCD b % 8).  After the remap, the blocks that land on one XCD own a
// contiguous range of logical tile ids, so neighbouring tiles share that XCD's L2.
__device__ __forceinline__ int pwc_xcd_remap(int b, int nblocks) {
    const int q = nblocks >> 3, r = nblocks & 7;
    const int xcd = b & 7, k = b >> 3;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + k;
}

// ---- the two-term fp16 operand split of the F16-matrix-pipe kernels (conv3x3_h2.hip, conv3x3_c16pair.hip,
// cost_volume_mfma.hip):  x = h + 2^-11 m',  h = fp16(x),  m' = fp16((x - h) 2^11)  (x - h is exact in fp32; the scaling keeps
// m' out of fp16's subnormals).  Two values in four vector instructions: v_cvt_pk_f16_f32, v_pk_mul_f32 (x 2^11 of both) and
// one mixed-precision FMA per value that reads the fp16 half in place and writes its half of the pair -- the same values as
//   h = (_Float16)x;  m' = (_Float16)fmaf((float)h, -2048.f, x * 2048.f);
// which the compiler turns into seven.  |x| >= 65520 rounds h to inf (m' is then -inf / NaN): the range condition of these
// kernels; [65504, 65520) still rounds h to 65504 with a finite m' (< 2^15) and stays exact (tests/test_gpu_forward_f64.py,
// tests/test_gpu_f16_pipe_f64.py).
__device__ __forceinline__ void pwc_split2(const float x0, const float x1, unsigned& h_pair, unsigned& m_pair) {
    const f32x2 xs = {x0, x1};
    const pwc_f16x2 h2 = __builtin_convertvector(xs, pwc_f16x2);
    const f32x2 xm = xs * 2048.f;
    const unsigned hp = __builtin_bit_cast(unsigned, h2);
    const float neg = -2048.f;
    unsigned mp;
    asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(mp) : "v"(hp), "s"(neg), "v"(xm[0]));
    asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(mp) : "v"(hp), "s"(neg), "v"(xm[1]));
    h_pair = hp; m_pair = mp;
}
__device__ __forceinline__ void pwc_split4(const f32x4 x, pwc_f16x4& h, pwc_f16x4& m) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    u32x2 hp, mp;
    unsigned a, b;
    pwc_split2(x[0], x[1], a, b); hp[0] = a; mp[0] = b;
    pwc_split2(x[2], x[3], a, b); hp[1] = a; mp[1] = b;
    h = __builtin_bit_cast(pwc_f16x4, hp);
    m = __builtin_bit_cast(pwc_f16x4, mp);
}
__device__ __forceinline__ void pwc_split4(const float x0, const float x1, const float x2, const float x3, pwc_f16x4& h, pwc_f16x4& m) {
    pwc_split4(f32x4{x0, x1, x2, x3}, h, m);
}
// One value, for the weight pack kernels.  fma(h, -2^11, x 2^11) and (x - h) 2^11 are the same bits for every finite
// |x| < 65520: x - h, h 2^11 and x 2^11 are all exact in fp32 there, so either spelling rounds the same number to fp16 once.
__device__ __forceinline__ void pwc_split1(const float x, _Float16& h, _Float16& m) {
    h = (_Float16)x;
    m = (_Float16)__builtin_fmaf((float)h, -2048.f, x * 2048.f);
}

// ---- packed weights of the kernels that keep all 32 output channels as the row operand of one 32 x 32 x 16 instruction
// (conv3x3_t32.hip, conv3x3_w32.hip): packed[tap][j][hm][lane][e] (fp16) = weight of output channel lane & 31, tap, physical
// input channel 16 j + 8 (lane >> 5) + e, h halves then m' halves; cin_map as in pwc_conv3x3_pack_f32.
template <int COUT = 32>
__global__ void conv3x3_c32_pack_kernel(const float* __restrict__ w, const int32_t* __restrict__ cin_map, int Cin, int Cin_phys,
                                        _Float16* __restrict__ packed) {
    static_assert(COUT == 32, "the row operand of v_mfma_f32_32x32x16_f16");
    const int j16 = Cin_phys >> 4;
    const int total = 9 * j16 * 512;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int e = idx & 7, lane = (idx >> 3) & 63;
        const int r = idx >> 9;
        const int j = r % j16, tap = r / j16;
        const int cphys = j * 16 + (lane >> 5) * 8 + e, co = lane & (COUT - 1);
        const int clog = cin_map ? cin_map[cphys] : (cphys < Cin ? cphys : -1);
        float v = 0.f;
        if (clog >= 0 && clog < Cin) v = w[((size_t)tap * Cin + clog) * COUT + co];
        _Float16* dst = packed + (size_t)r * 1024 + lane * 8 + e;
        pwc_split1(v, dst[0], dst[512]);
    }
}

// ---- the strided tile kernel (conv3x3_s2.hip) behind pwc_conv3x3_sk_f32 and pwc_conv3x3_h2_stride2_f32: stride 2, dilation 1,
// 'SAME', weights in the pwc_conv3x3_sk_pack_f32 layout.  _admits: the shapes it handles (C_in % 32, C_out % 16, C_out <= 128, the
// tensor behind one buffer resource); _count: its workgroups (tiles of 4 x 32 output pixels); _launch: the callers have checked
// pointers, channel strides and alignment by their own rules.
#define PWC_S2_TILE_ROWS 4
#define PWC_S2_TILE_COLS 32
bool pwc_conv3x3_s2_tile_admits(int N, int H, int W, int x_cs, int Cin_phys, int Cout);
long pwc_conv3x3_s2_tile_count(int N, int H, int W);
int pwc_conv3x3_s2_tile_launch(const float* x, int x_cs, const float* packed_w, const float* bias, float* y, int y_cs, int N, int H,
                               int W, int Cin_phys, int Cout, int apply_act, float slope, pwc_stream_t stream);
#ifdef PWC_HARNESS
int pwc_conv3x3_s2_tile_debug_mode();
#endif
