/*
 * pwc_hip.h -- C ABI of libpwc_hip.so: the MI355X (gfx950) PWC-Net inference ops.
 *
 * The reference (daigo0927/pwcnet) has no FFI layer: its op-level API is the Python
 * of model.py / modules.py running stock TensorFlow-1.8 primitives.  Each entry point
 * below replaces the TF sub-graph of one reference callable (file:line cited per
 * function); pwcnet_amd/modules.py binds them with ctypes and re-exposes the
 * reference's class names and call signatures.  INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions (all functions):
 *   - tensors are NHWC float32 in device (HBM) memory, caller-owned; nothing is
 *     allocated, freed or synchronised inside the library;
 *   - a tensor argument is (pointer to its first channel, channel stride `*_cs` in
 *     floats): pixel p, channel c lives at ptr[p * cs + c].  cs == C is a dense
 *     tensor; cs > C addresses a channel slice of a wider tensor, which is how
 *     tf.concat (modules.py:264,270,305) is made free;
 *   - work is enqueued on `stream` (a hipStream_t; NULL = the default stream) and the
 *     call returns immediately;
 *   - return value: PWC_OK (0), a negative PWC_E* argument error, or a positive
 *     hipError_t from the launch.  No exceptions, no global mutable state: the
 *     functions are re-entrant and thread-safe on distinct streams.  What a launch
 *     does is decided by its arguments alone (tile variants are explicit `_variant_`
 *     entry points); the library exports NO process-wide setting.  The ablation /
 *     tile-pinning knobs the A/B scripts under scripts/ use (pwc_debug_*) exist only
 *     in libpwc_hip_harness.so, a second build of the same sources with -DPWC_HARNESS
 *     (pwcnet_amd/_lib.py, PWC_HARNESS=1) that no product path and no test loads.
 */
#ifndef PWC_HIP_H
#define PWC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pwc_stream_t; /* hipStream_t */

enum {
    PWC_OK = 0,
    PWC_EINVAL = -1,   /* null pointer / non-positive size */
    PWC_EALIGN = -2,   /* pointer or channel stride not aligned as the kernel needs */
    PWC_ERANGE = -3,   /* size exceeds what the kernel indexes (see each function) */
    PWC_EUNSUPPORTED = -4
};

/* Library version (major*10000 + minor*100 + patch). */
int pwc_version(void);
/* Text for a return code of this library (negative codes) or of HIP (positive). */
const char* pwc_error_string(int code);

/* ---- a1: CostVolumeLayer.__call__ + get_cost/pad2d/crop2d, modules.py:158-204 ----
 * out[n,y,x,(v+R)*(2R+1)+(h+R)] =
 *     lrelu_slope( (1/C) * sum_c f0[n,y,x,c] * f1w[n,y+v,x+h,c] ),  0 outside the image;
 * v = vertical shift (outer loop, modules.py:197), h = horizontal (inner, :198).
 * Needs C % 4 == 0, f0/f1w 16-byte aligned with cs % 4 == 0; search_range in [1,4]. */
int pwc_cost_volume_f32(const float* f0, int f0_cs, const float* f1w, int f1w_cs,
                        float* out, int out_cs, int N, int H, int W, int C,
                        int search_range, float slope, pwc_stream_t stream);
/* 1 if pwc_cost_volume_f32 runs its rolling-window kernel for this geometry (C = 32, search_range 4,
 * 16-byte aligned operands, out_cs % 4 == 0, at least 4096 pixels per image), 0 for the tile kernel.
 * Same results either way; exported so that profilers can name the launch. */
int pwc_cost_volume_uses_rolling_kernel(int H, int W, int C, int search_range, int f0_cs, int f1_cs,
                                        int out_cs);

/* ---- a2: WarpingLayer(warp_type='bilinear') = bilinear_warp, modules.py:99-137 ----
 * out[n,y,x,:] = sum_{i,j} w_ij * x[n, clip(y+floor(fy)+i), clip(x+floor(fx)+j), :]
 * with (fx,fy) = flow_scale * flow[n,y,x,0:2]; flow_scale restates the caller's
 * `flows_up*self.scales[l]` (model.py:109).  Needs C % 4 == 0 and 16-byte alignment of
 * x/out with cs % 4 == 0. */
int pwc_warp_bilinear_f32(const float* x, int x_cs, const float* flow, int flow_cs,
                          float flow_scale, float* out, int out_cs,
                          int N, int H, int W, int C, pwc_stream_t stream);

/* ---- a3: WarpingLayer(warp_type='nearest') = nearest_warp, modules.py:83-97 ----
 * flow truncated toward zero (tf.cast int32, :85), added to the grid, clipped. */
int pwc_warp_nearest_f32(const float* x, int x_cs, const float* flow, int flow_cs,
                         float flow_scale, float* out, int out_cs,
                         int N, int H, int W, int C, pwc_stream_t stream);

/* ---- a2/a3 + the f0 part of tf.concat (modules.py:264) in one launch ----
 * pwc_warp_bilinear_f32 (bilinear != 0) or pwc_warp_nearest_f32 (bilinear == 0), and in the same
 * launch a copy of copy_C channels of every pixel of copy_src into copy_dst (copy_C == 0: none).
 * copy_C % 4 == 0, copy strides % 4 == 0, 16-byte aligned. */
int pwc_warp_copy_f32(int bilinear, const float* x, int x_cs, const float* flow, int flow_cs,
                      float flow_scale, float* out, int out_cs, int N, int H, int W, int C,
                      const float* copy_src, int copy_src_cs, float* copy_dst, int copy_dst_cs,
                      int copy_C, pwc_stream_t stream);

/* ---- a2+a1 (+ the f0 part of tf.concat, modules.py:264) for the COARSE pyramid levels ----
 * One launch for model.py:105-112 on small feature maps (7x16 ... 28x64 pixels per image), where
 * separate warp / cost-volume / copy launches are latency-bound: out as pwc_cost_volume_f32 of
 * (f0, warp(f1, flow_scale*flow)); flow == NULL: no warp (pyramid level 0, model.py:105-106);
 * f0_copy != NULL: f0's C channels are also copied to f0_copy (channel stride f0_copy_cs).
 * search_range must be 4 (PWC_EUNSUPPORTED otherwise); alignment rules of pwc_cost_volume_f32. */
int pwc_cost_volume_coarse_f32(const float* f0, int f0_cs, const float* f1, int f1_cs,
                               const float* flow, int flow_cs, float flow_scale,
                               float* out, int out_cs, float* f0_copy, int f0_copy_cs,
                               int N, int H, int W, int C, int search_range, float slope,
                               pwc_stream_t stream);

/* ---- a2+a1 fused: model.py:109-112 (warp then cost volume) without materialising
 * the warped feature map.  f1 is the UN-warped second feature map.  Same result as
 * pwc_warp_bilinear_f32 followed by pwc_cost_volume_f32.  Runs the matrix-pipe kernel of
 * pwc_warp_cost_volume_concat_f32 where that one is supported, the tile kernel with a gathering
 * loader otherwise. */
int pwc_warp_cost_volume_f32(const float* f0, int f0_cs, const float* f1, int f1_cs,
                             const float* flow, int flow_cs, float flow_scale,
                             float* out, int out_cs, int N, int H, int W, int C,
                             int search_range, float slope, pwc_stream_t stream);

/* ---- a2+a1 + the `features_0` part of tf.concat (modules.py:264) in ONE launch, correlation on the matrix
 * pipe (csrc/cost_volume_mfma.hip) -- model.py:105-112 for a pyramid level:
 *   out      = pwc_cost_volume_f32(f0, bilinear_warp(f1, flow_scale * flow))     (flow == NULL: f1 as is)
 *   f0_copy  = f0                                                                (f0_copy == NULL: no copy)
 * without ever writing the warped map.  out_pad_writable != 0 declares channels 81..83 of every `out` record
 * padding that the callee may overwrite with zeros (the estimator buffers of pwcnet_amd/model.py: segments start
 * on multiples of 4 channels) -- the record then leaves as 21 full 16-byte stores.
 * Supported: search_range 4, C in {32, 64, 96}, 16-byte aligned f0 / f1 / out / f0_copy with channel strides
 * % 4 == 0, flow 4-byte aligned, per-image extents below 2^31 bytes; anything else returns PWC_EUNSUPPORTED /
 * PWC_EALIGN and the caller uses the separate entry points.  pwc_warp_cost_volume_concat_supported tells in
 * advance (pointers taken as aligned). */
int pwc_warp_cost_volume_concat_f32(const float* f0, int f0_cs, const float* f1, int f1_cs,
                                    const float* flow, int flow_cs, float flow_scale,
                                    float* out, int out_cs, int out_pad_writable,
                                    float* f0_copy, int f0_copy_cs,
                                    int N, int H, int W, int C, int search_range, float slope,
                                    pwc_stream_t stream);
int pwc_warp_cost_volume_concat_supported(int H, int W, int C, int search_range, int f0_cs, int f1_cs,
                                          int flow_cs, int out_cs, int f0_copy_cs);
/* Round 5: the same launch with the correlation on the F16 matrix pipe: every operand (f0, and the warped f1 after the
 * fp32 bilinear blend of modules.py:132-135) is used as the two-term fp16 split x = h + 2^-11 m' of pwc_conv3x3_h2_f32,
 * three v_mfma_f32_16x16x32_f16 per (4x4-pixel block pair, 32 channels), fp32 accumulation -- 27 matrix instructions per
 * block where the fp32 form has 72 twice as long, and none of them stalls the vector instructions of its SIMD.  Error
 * against float64: not larger than the fp32 form's, and per output element within 16 x 2^-24 of the sum of absolute products
 * (16 + 4 behind a warp; tests/test_gpu_f16_pipe_f64.py).  RANGE: features below 65520 in magnitude ([65504, 65520) still splits
 * exactly; from 65520 on: NaN on the outputs that read the feature, never a finite wrong number; see PWC_STATUS_NONFINITE).  Same support set as the fp32 form.  Round 6: out_pad_writable = 2 (flow != NULL) puts
 * the pixel's flow (x, y), as read, into channels 81, 82 of its record and zero into channel 83: the record is then
 * [cv | flows_up_prev | 0] of the estimator's input (see pwc_conv3x3_h2_ex3_f32). */
int pwc_warp_cost_volume_concat_h2_f32(const float* f0, int f0_cs, const float* f1, int f1_cs,
                                       const float* flow, int flow_cs, float flow_scale,
                                       float* out, int out_cs, int out_pad_writable,
                                       float* f0_copy, int f0_copy_cs,
                                       int N, int H, int W, int C, int search_range, float slope,
                                       pwc_stream_t stream);
/* Round 5: the same operation for the SMALL pyramid levels -- C in {96, 128, 192} (7 x 16 ... 28 x 64 pixels at 448 x 1024) --
 * on the F16 matrix pipe (csrc/cost_volume_blk.hip): one 4 x 4-pixel block of f0 per workgroup, its 12 x 12-pixel window
 * of f1 (all channels, the four bilinear corners) requested at once -- or, where a launch has fewer blocks than the device has
 * CUs, one of the window's three block rows per workgroup -- so a launch is one chain flow -> corners -> blend -> matrix
 * instructions -> stores instead of a channel-stage loop of memory round trips (pwc_cost_volume_coarse_f32) or a walk over
 * block rows (the _h2 form: faster from about 8192 pixels per launch on, where this form's nine-fold re-gather of f1 costs
 * more than the walk's prologue).  Also takes C = 64 (small batches).  Arithmetic and range as
 * pwc_warp_cost_volume_concat_h2_f32.  Alignment requirements as pwc_warp_cost_volume_concat_f32;
 * pwc_warp_cost_volume_concat_blk_supported tells in advance. */
int pwc_warp_cost_volume_concat_blk_f32(const float* f0, int f0_cs, const float* f1, int f1_cs,
                                       const float* flow, int flow_cs, float flow_scale,
                                       float* out, int out_cs, int out_pad_writable,
                                       float* f0_copy, int f0_copy_cs,
                                       int N, int H, int W, int C, int search_range, float slope,
                                       pwc_stream_t stream);
int pwc_warp_cost_volume_concat_blk_supported(int H, int W, int C, int search_range, int f0_cs, int f1_cs,
                                              int flow_cs, int out_cs, int f0_copy_cs);

/* ---- a4/a5/a6: tf.layers.Conv2D(Cout,(3,3),(s,s),'same',dilation_rate=d) [+
 * tf.nn.leaky_relu(slope)] -- modules.py:62-67,267-268,274,306-324 ----
 *
 * Weight packing for the fp32-MFMA implicit-GEMM kernel.  `w_hwio` is the TF variable
 * (3,3,Cin,Cout).  `cin_map` (length Cin_phys, device int32, may be NULL = identity on
 * the first Cin entries, padding after) gives for every PHYSICAL input channel of the
 * activation buffer the logical TF channel it holds, or -1 for a padding channel
 * (its weights are packed as zero).  Cin_phys % 16 == 0.  The packed buffer holds
 * pwc_conv3x3_packed_floats(Cin_phys, Cout) floats. */
size_t pwc_conv3x3_packed_floats(int Cin_phys, int Cout);
int pwc_conv3x3_pack_f32(const float* w_hwio, const int32_t* cin_map, int Cin, int Cin_phys,
                         int Cout, float* packed, pwc_stream_t stream);

/* y[n,oy,ox,co] = act(bias[co] + sum_{ty,tx,ci} x[n,oy*s-pt+ty*d,ox*s-pl+tx*d,ci] * w[ty,tx,ci,co])
 * with TF 'SAME' padding (pad_total = max((out-1)*s + 2d+1 - in, 0), pad_before =
 * pad_total/2: stride 2 on an even size pads bottom/right only).  apply_act=0 gives
 * the activation-less flow heads.  Output is (N,ceil(H/s),ceil(W/s),Cout) at channel
 * stride y_cs.
 * Launch plan: `tile` = -1 lets the library choose (large M: big tiles for the full
 * rounds of workgroups + a smaller-tile tail launch; small M: the 9 taps are split over
 * 3 or 9 workgroup groups whose partial sums go through `workspace` and are summed in a
 * fixed order by a reduce kernel -- deterministic).  tile >= 0 forces one tile
 * configuration; `split` = 0 (library decides), 1 (never), 3 or 9.  `workspace` is
 * caller-owned scratch of `workspace_floats` floats (pwc_conv3x3_workspace_floats gives
 * the worst case); NULL disables the tap split.
 * Needs Cout % 16 == 0, x 16-byte aligned, x_cs % 4 == 0, x_cs >= Cin_phys, and every
 * padding channel of x finite (they meet zero weights). */
int pwc_conv3x3_f32(const float* x, int x_cs, const float* packed, const float* bias,
                    float* y, int y_cs, int N, int H, int W, int Cin_phys, int Cout,
                    int stride, int dilation, int apply_act, float slope, int tile, int split,
                    float* workspace, size_t workspace_floats, pwc_stream_t stream);
size_t pwc_conv3x3_workspace_floats(int M, int Cout);

/* Introspection: the plan pwc_conv3x3_f32(tile = -1) uses for M output pixels:
 * plan4 = {main tile id, tail tile id or -1, pixels covered by the main launch, tap split};
 * pwc_conv3x3_tile_shape gives a tile id's workgroup tile BM x BN. */
int pwc_conv3x3_plan(int M, int Cout, int Cin_phys, int* plan4);
/* 1 when pwc_conv3x3_f32(tile = -1, split = 0) routes this shape to the resident-weights /
 * halo-patch kernel (stride 1, dilation 1, Cin_phys == Cout in {16, 32}, M >= 65536). */
int pwc_conv3x3_uses_halo_kernel(int M, int Cin_phys, int Cout, int stride, int dilation);
int pwc_conv3x3_tile_shape(int tile, int* bm, int* bn);

/* Winograd F(2x2,3x3) form of the same convolution for stride 1 and Cout % 16 == 0:
 * 2.25x fewer multiplies (16 per 2x2 outputs instead of 36), fp32 result within ~1e-6
 * relative of the direct sum.  A dilation-d convolution is run as d*d ordinary ones on the
 * pixel sub-lattices (y mod d, x mod d).  pwc_conv3x3_wino_workgroups gives the number of
 * 16x16-pixel x 32-channel workgroups a launch would have (the caller's profitability test:
 * small or sparsely filled launches are faster on pwc_conv3x3_f32).  `packed_u` holds the transformed weights
 * U = G g G^T produced by pwc_conv3x3_wino_pack_f32 (same cin_map semantics as
 * pwc_conv3x3_pack_f32; pwc_conv3x3_wino_packed_floats floats).  Other requirements as
 * pwc_conv3x3_f32. */
size_t pwc_conv3x3_wino_packed_floats(int Cin_phys, int Cout);
int pwc_conv3x3_wino_pack_f32(const float* w_hwio, const int32_t* cin_map, int Cin, int Cin_phys,
                              int Cout, float* packed_u, pwc_stream_t stream);
int pwc_conv3x3_wino_f32(const float* x, int x_cs, const float* packed_u, const float* bias,
                         float* y, int y_cs, int N, int H, int W, int Cin_phys, int Cout,
                         int dilation, int apply_act, float slope, pwc_stream_t stream);
long pwc_conv3x3_wino_workgroups(int N, int H, int W, int Cout, int dilation);
/* Winograd F(4x4,3x3) form of the same convolution (csrc/conv3x3_wino4.hip): 36 multiplies per 4x4 outputs instead
 * of 64, for the big full-resolution layers (modules.py:267-268 `optflow_4/conv2d..conv2d_2`, modules.py:308-316
 * `context/conv2d_1..conv2d_3`).  fp32 throughout; its rounding error is ~10x that of F(2x2) per layer (2e-6 of the
 * activation scale) and leaves the end-to-end flow error where a direct fp32 convolution puts it (profiles/
 * r03_f4x4_numerics.txt).  packed_u comes from pwc_conv3x3_wino4_pack_f32 ([36][Cin_phys/16][Cout_pad][16] floats).
 * Needs Cout % 16 == 0, Cin_phys % 16 == 0, y 16-byte aligned with y_cs % 4 == 0.  pwc_conv3x3_wino4_supported: 1
 * where it is the faster kernel for the shape (48 <= Cin_phys <= 256, Cout >= 32, at least 256 workgroups of 16 x 32
 * pixels x 16 couts, sub-lattices of at least 14 x 28 pixels), 0 otherwise. */
size_t pwc_conv3x3_wino4_packed_floats(int Cin_phys, int Cout);
int pwc_conv3x3_wino4_pack_f32(const float* w_hwio, const int32_t* cin_map, int Cin, int Cin_phys,
                               int Cout, float* packed_u, pwc_stream_t stream);
int pwc_conv3x3_wino4_f32(const float* x, int x_cs, const float* packed_u, const float* bias,
                          float* y, int y_cs, int N, int H, int W, int Cin_phys, int Cout,
                          int dilation, int apply_act, float slope, pwc_stream_t stream);
int pwc_conv3x3_wino4_supported(int N, int H, int W, int Cin_phys, int Cout, int dilation);
/* The same convolution DIRECTLY (no Winograd transform) on the F16 matrix pipe with exact-to-22-bit operand splits
 * (csrc/conv3x3_h2.hip; reference modules.py:266-268 `optflow_l/conv2d*`, modules.py:306-323 `context/conv2d*`,
 * modules.py:221-236 `fp_extractor/conv2d*` where they are stride 1).  fp32 in, fp32 out, fp32 accumulation.  Every
 * operand is used as x = h + 2^-11 m' with h = fp16(x), m' = fp16((x - h) 2^11); of the four cross products the three
 * above 2^-22 are formed (uh vh, uh vm', um' vh; v_mfma_f32_32x32x16_f16) in two fp32 accumulators.  Measured error
 * against a float64 convolution: 0.1x that of pwc_conv3x3_wino4_f32 and 0.7x that of pwc_conv3x3_wino_f32 on every
 * layer shape (profiles/r04_exp_h2.txt), 0.4x that of a v_mfma_f32_16x16x4_f32 chain (profiles/
 * r04_exp_f16x2_numerics.txt).  RANGE: inputs and weights below 65520 in magnitude (fp16's largest finite value is 65504;
 * up to 65520 h rounds to it and the split stays exact); 65520 and beyond makes the outputs that depend on it NaN (inf - inf
 * in the split), never a silently wrong number.  LOWER END: the split is exact to 22 bits for |x| >= 2^-14 (6e-5); below that h and m' reach fp16's subnormals and
 * the operand carries an ABSOLUTE error of up to 1.5e-11 (3e-4 relative at |x| = 1e-7) -- harmless for activations and
 * weights that are summed with terms of ordinary size, not for a tensor that is small as a whole: the training path keeps its
 * data gradients on the fp32 kernels for that reason (pwcnet_amd/train.py, Trainer(f16x2_dgrad=False)).  packed_w comes from pwc_conv3x3_h2_pack_f32 (split weights, pwc_conv3x3_h2_packed_floats floats; same
 * cin_map semantics as pwc_conv3x3_pack_f32).  Needs Cout % 32 == 0, Cout <= 512, Cin_phys % 16 == 0, x and y 16-byte aligned with
 * x_cs % 4 == 0 and y_cs % 4 == 0.  pwc_conv3x3_h2_supported: 1 where it is the fastest kernel of this library for the
 * shape (Cin_phys >= 32, sub-lattices of at least 7 x 24 pixels -- narrower ones of an even dilation are taken two at a time
 * where Cout % 64 == 0 --, at least 192 tiles -- or at least 64 with a channel loop
 * long enough for the workspace form below to spread it over the CUs), 0 otherwise; the entry point
 * itself accepts every shape that meets the requirements above. */
size_t pwc_conv3x3_h2_packed_floats(int Cin_phys, int Cout);
int pwc_conv3x3_h2_pack_f32(const float* w_hwio, const int32_t* cin_map, int Cin, int Cin_phys,
                            int Cout, float* packed_w, pwc_stream_t stream);
int pwc_conv3x3_h2_f32(const float* x, int x_cs, const float* packed_w, const float* bias,
                       float* y, int y_cs, int N, int H, int W, int Cin_phys, int Cout,
                       int dilation, int apply_act, float slope, float* workspace, size_t workspace_floats,
                       pwc_stream_t stream);
/* `workspace` (caller-owned, 16-byte aligned, pwc_conv3x3_h2_workspace_floats floats, every byte 0xFF before the first
 * launch that uses the buffer -- every launch leaves it so -- and not shared by launches that may run concurrently)
 * turns a launch into one workgroup per CU, each computing an equal share of the launch's (tile, 16-channel stage)
 * sequence, wherever that is the faster form (more tiles than CUs: no partly filled last round, one prologue per workgroup
 * instead of one per tile; far fewer tiles than CUs and a long channel loop: every CU gets a part of it).  A tile cut into
 * pieces is finished by the workgroup holding its first piece, which adds the others' published fp32 sums to its own in the
 * order of their stages (finished sums, fixed order: the result does not depend on timing, launches repeat bitwise) --
 * within fp32 rounding of the uncut sum.  workspace = NULL (or pwc_conv3x3_h2_workspace_floats = 0): one workgroup per
 * tile. */
size_t pwc_conv3x3_h2_workspace_floats(int N, int H, int W, int Cin_phys, int Cout, int dilation);
int pwc_conv3x3_h2_supported(int N, int H, int W, int Cin_phys, int Cout, int dilation);
/* Round 5.  Status words: `status` points at TWO caller-owned uint32 in device memory (8-byte aligned; the caller zeroes
 * them, launches only OR bits into status[0] / atomic-max status[1]; NULL: no report).
 *   status[0] & PWC_STATUS_NONFINITE        pwc_resize_bilinear_status_f32 wrote a value that is not finite.  The F16-pipe
 *                                           kernels (pwc_conv3x3_h2*, pwc_conv3x3_c16pair*, pwc_warp_cost_volume_concat_h2_f32)
 *                                           turn an operand at or beyond 65520 in magnitude into NaN outputs (inf - inf in the
 *                                           split; the band 65504-65519 still splits exactly: planted operands of 65503, 65519 and
 *                                           +-65520 are tested against float64 on every one of these kernels,
 *                                           tests/test_gpu_forward_f64.py and tests/test_gpu_f16_pipe_f64.py).  An INTERMEDIATE of
 *                                           pwc_conv3x3_c16pair_f32 / pwc_conv3x3_c3c16pair_f32 that reaches 65520 from in-range inputs
 *                                           does the same to every output behind it (tested).  NaN survives every later layer of the network, so the model's LAST launch
 *                                           sees it: repeat the forward on the fp32 kernels (the reference, plain fp32, has no
 *                                           such limit).  Watching the operands inside the kernels instead was measured at 2-3 %
 *                                           of every launch (profiles/r05_timeline_range_tracking_cost.txt).
 *   status[0] & PWC_STATUS_STREAMK_TIMEOUT  a workgroup of the workspace form of pwc_conv3x3_h2* gave up waiting for a published
 *                                           partial sum (cannot happen short of a fault); its outputs are NaN and the workspace
 *                                           may hold stale sums: refill it with 0xFF bytes before its next use
 *   status[1]                               pwc_absmax_f32: bits of the largest |value| seen (a non-negative float orders like
 *                                           its bit pattern) -- the debugging aid behind PWCDCNet(track_max=True)
 * pwc_conv3x3_h2_ex_f32 = pwc_conv3x3_h2_f32 with the status words and with the input channels given as TWO tensors over
 * the same pixels: physical channels [0, Cin_a_phys) are channels [0, Cin_a_phys) of x (Cin_a_phys % 16 == 0), channels
 * [Cin_a_phys, Cin_phys) are channels [0, Cin_phys - Cin_a_phys) of x2 (channel stride x2_cs, 16-byte aligned).  This is
 * how `tf.concat([cv, features_0, flows_up_prev, features_up_prev])` (reference modules.py:261-264) costs nothing for
 * features_0: the estimator's first layer reads it from the pyramid tensor.  x2 = NULL: all channels from x. */
#define PWC_STATUS_NONFINITE 1u
#define PWC_STATUS_STREAMK_TIMEOUT 2u
int pwc_conv3x3_h2_ex_f32(const float* x, int x_cs, int Cin_a_phys, const float* x2, int x2_cs,
                          const float* packed_w, const float* bias, float* y, int y_cs, int N, int H, int W,
                          int Cin_phys, int Cout, int dilation, int apply_act, float slope, float* workspace,
                          size_t workspace_floats, uint32_t* status, pwc_stream_t stream);
/* Round 6: the input channels as THREE tensors over the same pixels (dilation 1): physical channels [0, Cin_a_phys) from x, the
 * next Cin_b_phys from x2, the remaining Cin_phys - Cin_a_phys - Cin_b_phys from x3 (Cin_a_phys, Cin_b_phys % 16 == 0; x2, x3
 * 16-byte aligned, strides % 4 == 0).  An operand's channel stride may be up to 12 channels SHORT of its 16-channel stage count
 * (x_cs = 84 with Cin_a_phys = 96): its last stage then reads the first channels of the NEXT pixel's record (zeros behind an
 * image's last pixel), which must hold finite values, and the caller packs zero weights for those channels (cin_map = -1).
 * With it `tf.concat([cv, features_0, flows_up_prev, features_up_prev])` (reference modules.py:261-264) is three tensors that
 * their producers write DENSELY: [cv 81 | flows_up_prev 2 | 0] in 336-byte records (pwc_warp_cost_volume_concat_h2_f32 with
 * out_pad_writable = 2), features_0 in the pyramid tensor, features_up_prev as a 32-channel tensor -- no producer writes a slice
 * of a wider record.  The logical channel order of the concat lives in the packed weights. */
int pwc_conv3x3_h2_ex3_f32(const float* x, int x_cs, int Cin_a_phys, const float* x2, int x2_cs, int Cin_b_phys,
                           const float* x3, int x3_cs, const float* packed_w, const float* bias, float* y, int y_cs,
                           int N, int H, int W, int Cin_phys, int Cout, int apply_act, float slope, float* workspace,
                           size_t workspace_floats, uint32_t* status, pwc_stream_t stream);
/* TWO chained 3x3 stride-1 'SAME' convolutions of 16 channels each (16 -> 16 -> 16) with a leaky-relu of slope `slope`
 * behind each, in one launch (csrc/conv3x3_c16pair.hip; reference modules.py:62-67, the `fp_extractor/conv2d_1`,
 * `conv2d_2` pair of pyramid level 1): the intermediate stays in LDS instead of making a round trip through memory.
 * Arithmetic as pwc_conv3x3_h2_f32 (fp32 in / out / accumulation, exact-to-22-bit fp16 operand pairs, three products;
 * the intermediate is rounded to fp32 exactly as a tensor in memory would be).  RANGE: inputs, weights AND the intermediate
 * below 65520 in magnitude; from 65520 on the outputs that read the value are NaN, never a finite wrong number
 * (tests/test_gpu_f16_pipe_f64.py: per output element against float64, also for pwc_conv3x3_c3c16pair_f32).  packed comes from
 * pwc_conv3x3_c16pair_pack_f32 (both HWIO (3,3,16,16) kernels; pwc_conv3x3_c16pair_packed_floats floats).  x, y: NHWC
 * with channel strides x_cs, y_cs >= 16 (multiples of 4), 16-byte aligned.  _supported: 1 where the fused launch is
 * the faster way to run the pair (at least one 16 x 32-pixel tile per CU). */
size_t pwc_conv3x3_c16pair_packed_floats(void);
int pwc_conv3x3_c16pair_pack_f32(const float* w1_hwio, const float* w2_hwio, float* packed, pwc_stream_t stream);
int pwc_conv3x3_c16pair_f32(const float* x, int x_cs, const float* packed, const float* bias1, const float* bias2,
                            float* y, int y_cs, int N, int H, int W, float slope, pwc_stream_t stream);
int pwc_conv3x3_c16pair_supported(int N, int H, int W);
/* The same launch with the stride-2 'SAME' convolution of the RAW images in front (3 -> 16 -> 16 -> 16, leaky-relu behind
 * each; reference modules.py:57-67, `fp_extractor/conv2d`, `conv2d_1`, `conv2d_2`: all of pyramid level 1): a workgroup
 * fetches the 41 x 73-pixel raw patch of its 16 x 32-pixel output tile and neither intermediate leaves the CU.  The first
 * convolution runs on the same split arithmetic (27 of a 32-deep matrix instruction).  The images are two batches that
 * share the weights (the two frames of a pair): N_a images at x_a, N_b at x_b (x_b = NULL with N_b = 0), NHWC with
 * EXACTLY 3 channels at channel stride 3, H0 x W0 with W0 % 4 == 0 (PWC_EUNSUPPORTED otherwise), 16-byte aligned; y:
 * (N_a + N_b) x ceil(H0 / 2) x W0 / 2 x 16 at channel stride y_cs.  packed: pwc_conv3x3_c3c16pair_pack_f32 of the HWIO
 * (3,3,3,16), (3,3,16,16), (3,3,16,16) kernels (pwc_conv3x3_c3c16pair_packed_floats floats).  _supported: W0 % 4 == 0
 * and the level-1 image is one pwc_conv3x3_c16pair_supported names. */
size_t pwc_conv3x3_c3c16pair_packed_floats(void);
int pwc_conv3x3_c3c16pair_pack_f32(const float* w0_hwio, const float* w1_hwio, const float* w2_hwio, float* packed,
                                   pwc_stream_t stream);
int pwc_conv3x3_c3c16pair_f32(const float* x_a, int N_a, const float* x_b, int N_b, const float* packed,
                              const float* bias0, const float* bias1, const float* bias2, float* y, int y_cs,
                              int H0, int W0, float slope, pwc_stream_t stream);
int pwc_conv3x3_c3c16pair_supported(int N, int H0, int W0);
/* Stride 2 ('SAME', dilation 1, EVEN H and W; the extractor's down-sampling layers, reference modules.py:57-60) through the
 * same kernel (round 5).  With the input seen as its four parity planes x_ab[y', x'] = x[2 y' + a, 2 x' + b] the strided
 * convolution is a stride-1 one with taps at 0 / +1 on each plane: a channel stage of the kernel is (16 channels, parity), fetched
 * from the pixels of its plane, and four of a stage's nine tap slots carry matrix instructions -- 16 Cin products per output
 * (a strided convolution needs 9 Cin; round 4's "stride-1 launch storing every second sum" executed 36 Cin and lost to the fp32
 * kernel).  y is (N, H / 2, W / 2) at channel stride y_cs.  packed_w: pwc_conv3x3_h2_stride2_pack_f32 (same arguments as
 * pwc_conv3x3_h2_pack_f32: cin_map over the input's Cin_phys physical channels; pwc_conv3x3_h2_stride2_packed_floats floats:
 * the parity-plane image and, for Cin_phys % 32 == 0 and Cout % 16 == 0, behind it the pwc_conv3x3_sk_pack_f32 image that the
 * strided tile kernel of csrc/conv3x3_s2.hip reads -- the entry point runs 32-channel inputs with Cout <= 128 on that kernel);
 * workspace: pwc_conv3x3_h2_stride2_workspace_floats (0: none), rules of pwc_conv3x3_h2_f32; status: the caller's status words
 * (or NULL), as pwc_conv3x3_h2_ex_f32's (PWC_STATUS_STREAMK_TIMEOUT).  Odd sizes: PWC_EUNSUPPORTED
 * (pwc_conv3x3_f32 takes them).  _supported: 1 where it is the faster kernel: inputs of up to 32 channels whose output is a
 * shape pwc_conv3x3_h2_supported takes at 4 Cin_phys channels (measured: 16 -> 32 and 32 -> 64 of the extractor; from 64 input
 * channels on the per-stage fixed cost of 4 x as many stages outweighs the matrix pipe's rate). */
size_t pwc_conv3x3_h2_stride2_packed_floats(int Cin_phys, int Cout);
int pwc_conv3x3_h2_stride2_pack_f32(const float* w_hwio, const int32_t* cin_map, int Cin, int Cin_phys,
                                    int Cout, float* packed_w, pwc_stream_t stream);
size_t pwc_conv3x3_h2_stride2_workspace_floats(int N, int H, int W, int Cin_phys, int Cout);
int pwc_conv3x3_h2_stride2_f32(const float* x, int x_cs, const float* packed_w, const float* bias,
                               float* y, int y_cs, int N, int H, int W, int Cin_phys, int Cout,
                               int apply_act, float slope, float* workspace, size_t workspace_floats,
                               uint32_t* status, pwc_stream_t stream);
int pwc_conv3x3_h2_stride2_supported(int N, int H, int W, int Cin_phys, int Cout);

/* Round 5: 3x3 convolution for SMALL launches (csrc/conv3x3_sk.hip) -- the 7 x 16 and 14 x 32 pyramid levels of a batch of
 * 8, every level of a single pair -- on the F16 matrix pipe, arithmetic and RANGE of pwc_conv3x3_h2_f32 (two-term fp16
 * operand splits, fp32 accumulation; |x|, |w| < 65520).  Same operation as pwc_conv3x3_f32 (TF 'SAME' padding, stride 1 | 2,
 * any dilation, + bias, + leaky_relu when apply_act): the K dimension (9 taps x Cin_phys) of a 16-pixel x 16-channel tile is
 * dealt to the eight waves of ONE workgroup, every wave requests all its operands at once, the eight partial sums are added
 * in wave order (launches repeat bitwise) -- one dispatch where the tiled kernels need a tap / channel split over workgroups
 * plus a reduce launch to fill the device.  Needs Cin_phys % 32 == 0, Cout % 16 == 0, x / y / packed_w / bias 16-byte
 * aligned, x_cs % 4 == 0, y_cs % 4 == 0, N*H*W*x_cs*4 < 2^31.  packed_w: pwc_conv3x3_sk_pack_f32 (the split halves in
 * fragment order, pwc_conv3x3_sk_packed_floats floats; cin_map as in pwc_conv3x3_pack_f32).  pwc_conv3x3_sk_supported: 1
 * where it is the fastest kernel of this library for the shape (the form that stages the workgroup's input patch in the
 * LDS: stride 1, no dilation, 96 ... 288 input channels, up to 2.4e8 multiply-adds -- output pixels x Cin_phys x Cout -- and 8 K
 * output pixels; stride 2, 64 ... 128 input channels, up to 2e8 multiply-adds; otherwise up to 1e8 multiply-adds and 4096
 * output pixels, beyond that pixel count stride-2 and thin layers only), else 0.
 * pwc_conv3x3_sk_variant_f32: the same convolution with the workgroup tile and form GIVEN -- tile in {11, 21, 22} (fragments from
 * global memory), {31, 41, 42} (patch in the LDS) -- for tests and tuning (every tile gives the same result on every shape it
 * admits; PWC_EUNSUPPORTED where it does not: x2 tiles need Cout % 32 == 0, 3x / 4x no dilation and at most 288 (stride 2: 128)
 * input channels; tile 50: the strided tile kernel of csrc/conv3x3_s2.hip -- stride 2, no dilation, Cout <= 128 -- which
 * pwc_conv3x3_sk_f32 itself launches for stride-2 layers of 192 or more 4 x 32-pixel output tiles).  The tile is an argument of
 * the call: the library keeps no process-wide setting. */
size_t pwc_conv3x3_sk_packed_floats(int Cin_phys, int Cout);
int pwc_conv3x3_sk_pack_f32(const float* w_hwio, const int32_t* cin_map, int Cin, int Cin_phys, int Cout,
                            float* packed_w, pwc_stream_t stream);
int pwc_conv3x3_sk_f32(const float* x, int x_cs, const float* packed_w, const float* bias, float* y, int y_cs,
                       int N, int H, int W, int Cin_phys, int Cout, int stride, int dilation, int apply_act,
                       float slope, pwc_stream_t stream);
int pwc_conv3x3_sk_supported(int N, int H, int W, int Cin_phys, int Cout, int stride, int dilation);
int pwc_conv3x3_sk_variant_f32(const float* x, int x_cs, const float* packed_w, const float* bias, float* y, int y_cs,
                               int N, int H, int W, int Cin_phys, int Cout, int stride, int dilation, int apply_act,
                               float slope, int tile, pwc_stream_t stream);

/* Round 5: the same convolution for THIN inputs to 32 output channels (csrc/conv3x3_t32.hip) -- Cin_phys 16 (stride 1 | 2) or
 * 32 (stride 1), Cout 32, no dilation: the feature extractor's full-resolution layers (reference modules.py:58-71,
 * fp_extractor/conv2d_3 ... conv2d_5).  Weights STATIONARY: a wave keeps the split halves of the whole weight tensor in
 * registers (9 or 18 K steps of a 32 x 32 x 16 matrix instruction whose row operand is all 32 output channels) and only pixel
 * fragments move: a workgroup walks over tiles of 8 rows x 32 pixels, the next tile's input patch arrives by LDS-DMA while the
 * four waves compute the current one; one barrier per tile.  Arithmetic, RANGE and alignment requirements of
 * pwc_conv3x3_sk_f32.  packed_w: pwc_conv3x3_t32_pack_f32 (pwc_conv3x3_t32_packed_floats floats; cin_map as in
 * pwc_conv3x3_pack_f32).  pwc_conv3x3_t32_supported: 1 where it is the fastest kernel of this library for the shape (a
 * supported shape with at least 256 tiles), else 0. */
size_t pwc_conv3x3_t32_packed_floats(int Cin_phys);
int pwc_conv3x3_t32_pack_f32(const float* w_hwio, const int32_t* cin_map, int Cin, int Cin_phys, float* packed_w,
                             pwc_stream_t stream);
int pwc_conv3x3_t32_f32(const float* x, int x_cs, const float* packed_w, const float* bias, float* y, int y_cs,
                        int N, int H, int W, int Cin_phys, int Cout, int stride, int apply_act, float slope,
                        pwc_stream_t stream);
int pwc_conv3x3_t32_supported(int N, int H, int W, int Cin_phys, int Cout, int stride);
/* Round 6: the same convolution for 32 OUTPUT channels from 32 or 64 input channels, stride 1, no dilation (csrc/conv3x3_w32.hip)
 * -- fp_extractor/conv2d_4, conv2d_5 (reference modules.py:58-71), optflow_l/conv2d_4 (modules.py:266-268: the 64 -> 32 layer of
 * every estimator) and context/conv2d_5 (modules.py:321-322).  The whole split weight tensor stays in the LDS for the life of a
 * persistent workgroup (36 / 72 KB), all 32 output channels are the row operand of one 32 x 32 x 16 matrix instruction, the input
 * patch of a tile (8 / 4 rows x 32 columns) is requested into registers under the previous tile's K loop and split once: no
 * per-stage staging (pwc_conv3x3_h2_f32 runs these layers at half the rate of its 128-cout layers).  64 input channels: the K
 * loop is dealt to two wave groups whose finished sums are added in a fixed order (launches repeat bitwise).  Arithmetic, RANGE
 * and alignment requirements of pwc_conv3x3_sk_f32; N*H*W*x_cs*4 and N*H*W*y_cs*4 < 2^31.  packed_w: pwc_conv3x3_w32_pack_f32
 * (pwc_conv3x3_w32_packed_floats floats; cin_map as in pwc_conv3x3_pack_f32).  pwc_conv3x3_w32_supported: 1 where it is the
 * fastest kernel of this library for the shape (a supported shape with at least 256 tiles), else 0. */
size_t pwc_conv3x3_w32_packed_floats(int Cin_phys);
int pwc_conv3x3_w32_pack_f32(const float* w_hwio, const int32_t* cin_map, int Cin, int Cin_phys, float* packed_w,
                             pwc_stream_t stream);
int pwc_conv3x3_w32_f32(const float* x, int x_cs, const float* packed_w, const float* bias, float* y, int y_cs,
                        int N, int H, int W, int Cin_phys, int Cout, int apply_act, float slope, pwc_stream_t stream);
int pwc_conv3x3_w32_supported(int N, int H, int W, int Cin_phys, int Cout, int stride, int dilation);
/* Tile variants of the kernel above (workgroup = couts x rows x 32 columns): 1 = 128 x 8, 2 = 64 x 16, 3 = 96 x 8,
 * 4 = 32 x 16, 5 = 64 x 8.  pwc_conv3x3_h2_plan: the one pwc_conv3x3_h2_f32 launches for a shape (fewest estimated
 * rounds of 256 workgroups x matrix instructions per tap; 0 = the shape is not accepted).  pwc_conv3x3_h2_variant_f32:
 * the same convolution with the variant given (Cout must be a multiple of its couts) -- for tests and tuning. */
int pwc_conv3x3_h2_plan(int N, int H, int W, int Cin_phys, int Cout, int dilation);
int pwc_conv3x3_h2_variant_f32(const float* x, int x_cs, const float* packed_w, const float* bias,
                               float* y, int y_cs, int N, int H, int W, int Cin_phys, int Cout,
                               int dilation, int apply_act, float slope, int variant, float* workspace,
                               size_t workspace_floats, pwc_stream_t stream);
/* The same convolution with the input-channel stages dealt to `csplit` workgroups per tile (launches that would leave
 * most of the GPU's workgroup slots empty: the 14x32 / 28x64 pyramid levels).  Partial outputs go to `workspace`
 * (pwc_conv3x3_wino_split_workspace_floats floats, 16-byte aligned) and are summed in a fixed order, with the bias and the
 * activation, by a second kernel: deterministic, within fp32 rounding of pwc_conv3x3_wino_f32.
 * pwc_conv3x3_wino_split_plan gives the csplit to use for a shape (1 = do not split; then no workspace is needed). */
int pwc_conv3x3_wino_split_plan(int N, int H, int W, int Cin_phys, int Cout, int dilation);
size_t pwc_conv3x3_wino_split_workspace_floats(int N, int H, int W, int Cout, int csplit);
int pwc_conv3x3_wino_split_f32(const float* x, int x_cs, const float* packed_u, const float* bias,
                               float* y, int y_cs, int N, int H, int W, int Cin_phys, int Cout,
                               int dilation, int apply_act, float slope, int csplit, float* workspace,
                               size_t workspace_floats, pwc_stream_t stream);

/* Same convolution straight from the HWIO variable, any Cin/Cout, plus the optional
 * residual add of modules.py:275-277 (`flows += flows_up_prev`) and modules.py:326
 * (`flows + x`): y = act(conv) + residual.  Used for Cin = 3 (first extractor layer),
 * Cout = 2 (flow heads) and as the in-library cross-check of the MFMA kernel. */
int pwc_conv3x3_direct_f32(const float* x, int x_cs, const float* w_hwio, const float* bias,
                           float* y, int y_cs, const float* residual, int res_cs,
                           int N, int H, int W, int Cin, int Cout, int stride, int dilation,
                           int apply_act, float slope, pwc_stream_t stream);

/* ---- a7: tf.image.resize_bilinear (TF 1.8 legacy: src = dst*in/out, no half-pixel,
 * no align-corners), modules.py:283-284 and model.py:127; y = resize(x) * mul. */
int pwc_resize_bilinear_f32(const float* x, int x_cs, float* y, int y_cs,
                            int N, int H, int W, int C, int OH, int OW, float mul,
                            pwc_stream_t stream);
/* The same launch; additionally status[0] |= PWC_STATUS_NONFINITE if any value it writes is not finite (status: two
 * caller-owned uint32, see pwc_conv3x3_h2_ex_f32; NULL = pwc_resize_bilinear_f32).  The model's last launch -- the x4
 * upsampling of model.py:127 -- runs through this entry: one compare per output of a launch that waits for memory. */
int pwc_resize_bilinear_status_f32(const float* x, int x_cs, float* y, int y_cs,
                                   int N, int H, int W, int C, int OH, int OW, float mul,
                                   uint32_t* status, pwc_stream_t stream);
/* status[1] = max(status[1], bits of max |x[p, 0:C]|) over npix pixels (channel stride x_cs); NaN entries are skipped.
 * Debugging aid (PWCDCNet(track_max=True) runs it on every conv input): how far a network's activations are from the
 * 65504 of the F16-pipe kernels. */
int pwc_absmax_f32(const float* x, int x_cs, long npix, int C, uint32_t* status, pwc_stream_t stream);

/* Two resizes of one geometry in one launch (modules.py:283-284: flows_up and features_up of the
 * same level): xa/ya carry 2 channels (8-byte aligned, even channel strides), xb/yb CB channels
 * (CB % 4 == 0, 16-byte aligned).  Same arithmetic as pwc_resize_bilinear_f32 with mul = 1. */
int pwc_resize_bilinear_pair_f32(const float* xa, int xa_cs, float* ya, int ya_cs,
                                 const float* xb, int xb_cs, float* yb, int yb_cs,
                                 int N, int H, int W, int CB, int OH, int OW, pwc_stream_t stream);

/* ---- stream placement probe (no reference counterpart: the reference times repeated sess.run calls, test.py:48-53, and
 * must not depend on the process's stream history).  pwc_device_spin keeps `stream` busy for about `ticks` cycles of the
 * device clock counter without touching memory; pwc_device_touch adds 1 to p[0].  pwcnet_amd/model.py brackets the pair
 * with timing events to learn whether two HIP streams share a hardware queue; never part of a forward. */
int pwc_device_spin(long long ticks, pwc_stream_t stream);
int pwc_device_touch(float* p, pwc_stream_t stream);

/* ---- tf.concat helper (modules.py:264,305): dst[p, 0:C] = src[p, 0:C] for npix pixels. */
int pwc_copy_channels_f32(const float* src, int src_cs, float* dst, int dst_cs,
                          long npix, int C, pwc_stream_t stream);

/* ---- losses (forward): reference losses.py:4-13 (L1loss, L2loss, EPE) and the per-level term of
 * multiscale_loss / multirobust_loss (losses.py:15-48) ----
 * out_sums[n] = sum over the H x W pixels of image n of
 *     || pred[n,y,x,0:2] - gt[n, floor(y*GH/H), floor(x*GW/W), 0:2] / gt_div ||_ord ,  ord = 1 or 2;
 * the nearest-neighbour downsampling of the ground truth (tf.image.resize_nearest_neighbor,
 * losses.py:27,43) is folded into the read (GH = H, GW = W for none).  Deterministic (fixed-order
 * partial sums in `workspace`, at least pwc_flow_norm_workspace_floats(N,H,W) floats). */
size_t pwc_flow_norm_workspace_floats(int N, int H, int W);
int pwc_flow_norm_sums_f32(const float* pred, int pred_cs, const float* gt, int gt_cs,
                           int N, int H, int W, int GH, int GW, float gt_div, int ord,
                           float* workspace, size_t workspace_floats, float* out_sums,
                           pwc_stream_t stream);

/* ==== f4: training path (reference train.py:66-92: tf.gradients of the forward + tf.train.AdamOptimizer) ====
 * Gradient tensors have the layout of the activation they belong to.  `accumulate` != 0: the kernel adds
 * into its output (an activation with several consumers collects its gradient from all of them). */

/* tf.nn.leaky_relu gradient, in place: dy[p,c] *= (y[p,c] > 0 ? 1 : slope), y = the activation's OUTPUT. */
int pwc_lrelu_grad_f32(const float* y, int y_cs, float* dy, int dy_cs, long npix, int C, float slope,
                       pwc_stream_t stream);
/* dst[p,0:C] = (accumulate ? dst : 0) + alpha * src[p,0:C] (channel-slice add / scaled copy). */
int pwc_add_f32(const float* src, int src_cs, float* dst, int dst_cs, long npix, int C, float alpha,
                int accumulate, pwc_stream_t stream);
/* out[c] (+)= sum over pixels of dy[p,c]: bias gradient of tf.layers.Conv2D.  Deterministic. */
size_t pwc_channel_sums_workspace_floats(long npix, int C);
int pwc_channel_sums_f32(const float* dy, int dy_cs, long npix, int C, float* workspace,
                         size_t workspace_floats, float* out, int accumulate, pwc_stream_t stream);
/* The two above in ONE pass over dy: dy *= (y > 0 ? 1 : slope) in place, out[c] (+)= sum_p dy[p,c]. */
int pwc_lrelu_grad_channel_sums_f32(const float* y, int y_cs, float* dy, int dy_cs, long npix, int C, float slope,
                                    float* workspace, size_t workspace_floats, float* out, int accumulate,
                                    pwc_stream_t stream);
/* Transpose of pwc_resize_bilinear_f32 (tf.image.resize_bilinear legacy, modules.py:283-284) for integer
 * factors OH/H = OW/W in 1..4: dx (+)= mul * R^T dy.  Gather form, deterministic. */
int pwc_resize_bilinear_grad_f32(const float* dy, int dy_cs, float* dx, int dx_cs, int N, int H, int W, int C,
                                 int OH, int OW, float mul, int accumulate, pwc_stream_t stream);
/* Gradient of pwc_warp_bilinear_f32 (bilinear_warp, modules.py:99-137; floor / clip carry no gradient):
 * dx += scatter of the corner weights (fp32 atomics; dx may be null), dflow (+)= flow_scale * d/d(flow*scale). */
int pwc_warp_bilinear_grad_f32(const float* x, int x_cs, const float* flow, int flow_cs, float flow_scale,
                               const float* dy, int dy_cs, float* dx, int dx_cs, float* dflow, int dflow_cs,
                               int dflow_accumulate, int N, int H, int W, int C, pwc_stream_t stream);
/* The same gradient with a bit-reproducible scatter: the corner contributions to dx are added as 64-bit fixed-point
 * integers (2^-36 steps) in `workspace` (pwc_warp_bilinear_grad_workspace_bytes bytes, 8-byte aligned; zeroed by the
 * call) and converted once -- integer sums do not depend on the order of the atomics.  dx == NULL: no workspace needed.
 * Range: contributions below 1.5e-11 vanish, sums are exact up to +-1.3e8; an upstream gradient that is not finite or
 * reaches 2^26 raises a poison word behind the sums and EVERY element of dx becomes NaN (a diverging step stays visible;
 * the fp32-atomic form keeps relative precision instead). */
size_t pwc_warp_bilinear_grad_workspace_bytes(int N, int H, int W, int C);
int pwc_warp_bilinear_grad_det_f32(const float* x, int x_cs, const float* flow, int flow_cs, float flow_scale,
                                   const float* dy, int dy_cs, float* dx, int dx_cs, float* dflow, int dflow_cs,
                                   int dflow_accumulate, int N, int H, int W, int C, void* workspace,
                                   size_t workspace_bytes, pwc_stream_t stream);
/* Gradient of pwc_cost_volume_f32 (modules.py:158-204) w.r.t. both feature maps, leaky-relu and mean
 * included: cv = the forward output, dcv = its gradient.  df0 / df1w may be null.  search_range 4. */
int pwc_cost_volume_grad_f32(const float* f0, int f0_cs, const float* f1w, int f1w_cs, const float* cv, int cv_cs,
                             const float* dcv, int dcv_cs, float* df0, int df0_cs, float* df1w, int df1w_cs,
                             int accumulate, int N, int H, int W, int C, int search_range, float slope,
                             pwc_stream_t stream);
/* Gradient w.r.t. pred of  scale * sum_p || pred[p] - gt[nearest(p)] / gt_div ||_ord  (losses.py:4-8,20-29). */
int pwc_flow_norm_grad_f32(const float* pred, int pred_cs, const float* gt, int gt_cs, int N, int H, int W,
                           int GH, int GW, float gt_div, int ord, float scale, float* dpred, int dpred_cs,
                           int accumulate, pwc_stream_t stream);
/* tf.train.AdamOptimizer update of a flat parameter buffer (TF 1.8 adam.py; train.py:90) with the gradient
 * of gamma * l2_loss(var) folded in (train.py:75): g = grad_scale * grads + l2_gamma * p; lr_t from the host. */
int pwc_adam_step_f32(float* params, const float* grads, float* m, float* v, long n, float lr_t, float beta1,
                      float beta2, float eps, float l2_gamma, float grad_scale, pwc_stream_t stream);
/* Weight gradient of tf.layers.Conv2D(...,(3,3),(s,s),'same',dilation_rate=d) on the fp32 MFMA units:
 * dw_hwio[ty][tx][ci][co] (+)= sum_pixels x_pad[...] * dy, ci in the variable's LOGICAL order (cin_map maps the
 * physical channels of x, -1 = padding; null = identity).  Deterministic (fixed-order split-k sums). */
size_t pwc_conv3x3_wgrad_workspace_floats(int N, int H, int W, int Cin_phys, int Cout, int stride);
int pwc_conv3x3_wgrad_f32(const float* x, int x_cs, const float* dy, int dy_cs, const int32_t* cin_map, int Cin,
                          int Cin_phys, int Cout, float* dw_hwio, int accumulate, int N, int H, int W, int stride,
                          int dilation, float* workspace, size_t workspace_floats, pwc_stream_t stream);
/* Data gradient of tf.layers.Conv2D(...,(3,3),(2,2),'same') for an input of 1..4 channels (the images of the first
 * extractor conv): dx (+)= d conv / d x . dy, w_hwio = the forward kernel (3,3,Cx,Cy), dx of size H x W (both even),
 * dy of size H/2 x W/2.  One pass over dy, no zero-stuffed map.  Cy % 4 == 0, dy 16-byte aligned with dy_cs % 4 == 0,
 * w_hwio 16-byte aligned (PWC_EALIGN); odd H or W, Cx outside 1..4, Cy % 4 != 0: PWC_EUNSUPPORTED; null pointers,
 * non-positive sizes, channel strides below the channel counts: PWC_EINVAL.  Every check precedes the launch. */
int pwc_conv3x3_dgrad_s2_narrow_f32(const float* dy, int dy_cs, const float* w_hwio, float* dx, int dx_cs, int N, int H,
                                    int W, int Cx, int Cy, int accumulate, pwc_stream_t stream);

/* ==== sparse ground truth: the losses, their gradient and the flow metrics under a validity mask ====
 * `valid` is one byte per pixel of the GROUND TRUTH, uint8_t[N][GH][GW], dense, non-zero = valid; no alignment is asked of
 * it (byte loads).  It is read at the nearest-neighbour index the ground truth is read at -- floor(y * GH / H), the rounded
 * fp32 product, clipped: tf.image.resize_nearest_neighbor applied to the mask.  Invalid pixels are SELECTED out: neither pred
 * nor gt is read there, an invalid pixel adds exactly 0.0f to every sum and exactly 0 to every gradient whatever the two hold
 * (NaN, Inf, the .flo sentinel 1e10).  Every check precedes the launches: null pointers, sizes <= 0, channel strides < 2,
 * gt_div == 0, a workspace that is too small: PWC_EINVAL; ord outside {1, 2}: PWC_EUNSUPPORTED; H * W > 2^31 - 65537 or N > 65535
 * (sums and metrics): PWC_ERANGE. */

/* pwc_flow_norm_sums_f32 over the valid pixels: out_sums[n] as there, out_counts[n] = the number of valid pixels of image n
 * at pred's resolution (exact; an image without valid pixels gives sum 0, count 0).  Deterministic, with the partition and
 * the order of additions of the unmasked call: an all-ones mask returns its bits. */
size_t pwc_flow_norm_masked_workspace_floats(int N, int H, int W);
int pwc_flow_norm_masked_sums_f32(const float* pred, int pred_cs, const float* gt, int gt_cs, const uint8_t* valid,
                                  int N, int H, int W, int GH, int GW, float gt_div, int ord,
                                  float* workspace, size_t workspace_floats, float* out_sums, int32_t* out_counts,
                                  pwc_stream_t stream);
/* pwc_flow_norm_grad_f32 at the valid pixels (an all-ones mask returns its bits); an invalid pixel's two floats are written
 * as 0 (accumulate == 0) or left untouched (accumulate != 0).  Channels outside dpred's two floats are never written. */
int pwc_flow_norm_masked_grad_f32(const float* pred, int pred_cs, const float* gt, int gt_cs, const uint8_t* valid,
                                  int N, int H, int W, int GH, int GW, float gt_div, int ord, float scale,
                                  float* dpred, int dpred_cs, int accumulate, pwc_stream_t stream);
/* Flow metrics of pred against gt, both N x H x W in pixels (flows_final against the ground truth); valid == NULL: every
 * pixel.  With e = ||pred - gt||_2 and g = ||gt||_2 at a valid pixel, out[n][0..11] =
 *   n_valid, sum e, n(e > 3 && e > 0.05 g)  [KITTI's outlier rule, Fl], n(e > 1), n(e > 3), n(e > 5),
 *   n(g < 10), sum e (g < 10), n(10 <= g < 40), sum e (10 <= g < 40), n(g >= 40), sum e (g >= 40).
 * Counts are added as integers (exact); sums are fp32 block partials added in index order in double: two calls give the
 * same bits.  One pass over the data; workspace: at least the floats the workspace function names. */
size_t pwc_flow_metrics_workspace_floats(int N, int H, int W);
int pwc_flow_metrics_f32(const float* pred, int pred_cs, const float* gt, int gt_cs, const uint8_t* valid,
                         int N, int H, int W, float* workspace, size_t workspace_floats, double* out,
                         pwc_stream_t stream);

/* ==== self-supervised losses: the photometric warp term, the edge-aware smoothness of the flow, the soft census term ====
 * Two loss terms that need no ground truth, each as per-image sums (a deterministic two-stage reduction: workgroup partials in
 * `workspace`, added in index order) and as the gradient of those sums with respect to the flow (a gather, one lane per pixel,
 * no atomics: deterministic).  All tensors NHWC fp32, pointer + channel stride; images have C = 1..4 channels and no alignment
 * is asked of anything (scalar loads).  The images are constants: no gradient reaches them.
 *   rho(d) = (d^2 + eps^2)^q  (generalised Charbonnier),  rho'(d) = 2 q d (d^2 + eps^2)^(q - 1).
 * Every check precedes the launches: null pointers other than the optional ones, sizes <= 0, a channel stride below the
 * channel count, eps <= 0, q outside (0, 1], alpha < 0, a workspace that is too small: PWC_EINVAL; C outside 1..4:
 * PWC_EUNSUPPORTED; H * W > 2^31 - 65537 or N > 65535: PWC_ERANGE. */

/* Photometric term.  Pixel p = (n, y, x) samples images_1[n] at (py, px) = (y + flow_scale * flow[p,1], x + flow_scale *
 * flow[p,0]) and CONTRIBUTES iff (valid == NULL or valid[p] != 0, uint8_t[N][H][W]) and 0 <= px <= W - 1 and 0 <= py <= H - 1
 * (a NaN or Inf flow fails the test).  Other pixels are selected out: no image is read for them and, where the mask rules them
 * out, no flow either.  The sample is the bilinear warp's: x0 = floor(px), x1 = min(x0 + 1, W - 1), weight px - x0 on x1, the
 * same in y.  out_sums[n] = sum over the contributing pixels of sum_c rho(images_0[p,c] - sample[c]); out_counts[n] = their
 * number (exact).  The sample point, the weights and the difference are computed in double and the difference is rounded to
 * fp32 once, so that rho' does not magnify a rounding error of the interpolation by 1 / eps. */
size_t pwc_photometric_workspace_floats(int N, int H, int W);
int pwc_photometric_sums_f32(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                             float flow_scale, const uint8_t* valid, int N, int H, int W, int C, float eps, float q,
                             float* workspace, size_t workspace_floats, float* out_sums, int32_t* out_counts,
                             pwc_stream_t stream);
/* dflow[p,0] (+)= dsums[n] * flow_scale * sum_c rho'(d_c) * (-d sample_c / d px), dflow[p,1] likewise along y (floor and clip
 * carry no gradient, as in the warp's own gradient).  dsums: N floats ON THE DEVICE, the upstream gradient of out_sums (no host
 * synchronisation).  A pixel that does not contribute gets 0 (accumulate == 0) or is left untouched (accumulate != 0). */
int pwc_photometric_grad_f32(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                             float flow_scale, const uint8_t* valid, int N, int H, int W, int C, float eps, float q,
                             const float* dsums, float* dflow, int dflow_cs, int accumulate, pwc_stream_t stream);

/* Smoothness term, first order, forward differences: out_sums[n] = sum over the pixels with x < W - 1 of
 * wx(p) * sum_k rho(flow[n,y,x+1,k] - flow[n,y,x,k]), wx(p) = exp(-alpha * mean_c |image[n,y,x+1,c] - image[n,y,x,c]|), plus
 * the same along y for y < H - 1.  image: at the flow's resolution, C channels; NULL: every weight is 1 (C and image_cs are
 * then ignored; a constant image gives the same bits). */
size_t pwc_flow_smoothness_workspace_floats(int N, int H, int W);
int pwc_flow_smoothness_sums_f32(const float* flow, int flow_cs, const float* image, int image_cs, int C, float alpha,
                                 float eps, float q, int N, int H, int W, float* workspace, size_t workspace_floats,
                                 float* out_sums, pwc_stream_t stream);
/* dflow (+)= dsums[n] * d out_sums[n] / d flow: every lane gathers the up to four differences its pixel takes part in (its
 * own along x and y, its left and its upper neighbour's). */
int pwc_flow_smoothness_grad_f32(const float* flow, int flow_cs, const float* image, int image_cs, int C, float alpha,
                                 float eps, float q, int N, int H, int W, const float* dsums, float* dflow, int dflow_cs,
                                 int accumulate, pwc_stream_t stream);
/* Smoothness term, second order (UnFlow's published configurations): the same parameters, checks and workspace
 * (pwc_flow_smoothness_workspace_floats) as the first-order pair.  out_sums[n] = sum over the centres 1 <= x <= W - 2 of
 * wxx(p) * sum_k rho(flow[n,y,x-1,k] - 2 flow[n,y,x,k] + flow[n,y,x+1,k]), wxx(p) = exp(-alpha * mean_c |image[n,y,x+1,c] -
 * image[n,y,x-1,c]|) -- the stride-2 image difference centred on the same pixel -- plus the same along y for 1 <= y <= H - 2.
 * A constant flow AND a constant slope cost nothing beyond rho(0).  W < 3: no x terms, H < 3: no y terms, both: the sum is 0, no
 * error.  image NULL: every weight is 1 (a constant image gives the same bits).  The second difference is formed in double
 * (exact for three fp32 values) and rounded to fp32 once. */
int pwc_flow_smoothness2_sums_f32(const float* flow, int flow_cs, const float* image, int image_cs, int C, float alpha,
                                  float eps, float q, int N, int H, int W, float* workspace, size_t workspace_floats,
                                  float* out_sums, pwc_stream_t stream);
/* dflow (+)= dsums[n] * d out_sums[n] / d flow: every lane gathers the up to six second differences its pixel takes part in --
 * along each axis as the left neighbour, the centre (factor -2) and the right neighbour.  No atomics. */
int pwc_flow_smoothness2_grad_f32(const float* flow, int flow_cs, const float* image, int image_cs, int C, float alpha,
                                  float eps, float q, int N, int H, int W, const float* dsums, float* dflow, int dflow_cs,
                                  int accumulate, pwc_stream_t stream);

/* Soft census (ternary) term: the photometric term on the local intensity ORDER, invariant to additive and largely to
 * multiplicative brightness changes.  Grey planes a(p) = scale * mean_c images_0[p] and b(p) = scale * mean_c (the photometric
 * term's bilinear sample of images_1 at p moved by flow_scale * flow[p]; sample point, weights and blend in double, rounded
 * once); b(p) = 0 with zero derivative where the sample point is out of frame or the flow is not finite.  With the K =
 * (2 radius + 1)^2 - 1 offsets o != 0 of the window,
 *   t0 = a(p+o) - a(p), t1 = b(p+o) - b(p), tau(t) = t / sqrt(c1 + t^2), d = (tau(t0) - tau(t1))^2, h(p) = (1/K) sum_o d / (c2 + d).
 * Pixel p CONTRIBUTES iff it is at least `radius` pixels from every border (no padding), its sample point is in frame, and
 * (valid == NULL or valid[p] != 0).  Unlike the photometric term's, the mask and the in-frame test select CENTRES only: the
 * neighbours of a contributing centre are always read (images_0 at a masked pixel must hold numbers).  out_sums[n] = sum over
 * the contributing pixels of rho(h(p)), out_counts[n] = their number (exact); H <= 2 radius or W <= 2 radius: both 0, no error.
 * Three launches: a per-pixel pass that writes a, b and the in-frame flag to workspace planes, a windowed pass (32 x 8 tiles of
 * centres with a `radius` halo staged in the LDS) that adds its tiles' terms in a fixed tree, and the parts added in index
 * order: two calls give the same bits.  workspace: at least pwc_census_workspace_floats(N, H, W, with_grad) floats, with_grad
 * 0 for the sums and 1 for the gradient.  Checks, in this order: null pointers and sizes <= 0 (PWC_EINVAL); C outside 1..4
 * or radius outside 1..3 (PWC_EUNSUPPORTED); a channel stride below the channel count, eps, scale, c1 or c2 <= 0, q outside
 * (0, 1] (PWC_EINVAL); H * W > 2^31 - 65537 or N > 65535 (PWC_ERANGE); a null or short workspace, null outputs (PWC_EINVAL). */
size_t pwc_census_workspace_floats(int N, int H, int W, int with_grad);
int pwc_census_sums_f32(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                        float flow_scale, const uint8_t* valid, int N, int H, int W, int C, int radius, float scale,
                        float c1, float c2, float eps, float q, float* workspace, size_t workspace_floats,
                        float* out_sums, int32_t* out_counts, pwc_stream_t stream);
/* dflow (+)= the gradient of sum_n dsums[n] * out_sums[n] w.r.t. the flow.  With G(p) = dsums[n] rho'(h(p)) / K where p
 * contributes and 0 elsewhere, and D(t0, t1) = c2 / (c2 + d)^2 * 2 (tau(t1) - tau(t0)) * c1 / (c1 + t1^2)^(3/2):
 *   dL/db(q) = -sum_o (G(q) + G(q+o)) D(t0(q,o), t1(q,o))   over the offsets with q+o inside the image
 * (tau is odd, so q as a centre and q as a neighbour of the centre q+o share one loop), and, where q is in frame,
 *   dflow[q] = flow_scale * scale * dL/db(q) * mean_c (d sample / d x, d sample / d y).
 * A pixel that is out of frame gets 0 (accumulate == 0) or is left untouched (accumulate != 0).  A gather over the same tiles
 * with a, b and G staged: no atomics, two calls give the same bits.  dsums: N floats on the device. */
int pwc_census_grad_f32(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                        float flow_scale, const uint8_t* valid, int N, int H, int W, int C, int radius, float scale,
                        float c1, float c2, float eps, float q, const float* dsums, float* workspace,
                        size_t workspace_floats, float* dflow, int dflow_cs, int accumulate, pwc_stream_t stream);

/* SSIM term: the data term of UFlow / ARFlow (0.15 L1 + 0.85 SSIM).  x(p, c) = images_0[p, c]; y(p, c) = the photometric term's
 * bilinear sample of images_1 at p moved by flow_scale * flow[p] -- its in-frame rule (0 <= px <= W - 1, 0 <= py <= H - 1, a
 * non-finite flow is out of frame), floor, clipped corners and weights; sample point, weights and blend in double, rounded to
 * fp32 once.  Per channel, over the n = (2 radius + 1)^2 pixels of the window of centre p, in double from the fp32 x and y and
 * in the CENTRED form, so that a variance cannot go negative:
 *   mu_x = mean x, mu_y = mean y, s_x = mean (x - mu_x)^2, s_y = mean (y - mu_y)^2, s_xy = mean (x - mu_x)(y - mu_y),
 *   A1 = 2 mu_x mu_y + c1, A2 = 2 s_xy + c2, B1 = mu_x^2 + mu_y^2 + c1, B2 = s_x + s_y + c2,
 *   SSIM = A1 A2 / (B1 B2),   term(p, c) = (1 - SSIM) / 2.
 * No clamp (|SSIM| <= 1 up to rounding), no eps and no q: the term is not passed through rho.  c1 = 0.01^2, c2 = 0.03^2 for
 * images in [0, 1]; radius 1 is the 3 x 3 window of UFlow / ARFlow.  A centre p CONTRIBUTES iff it is at least `radius` pixels
 * from every border (no padding), (valid == NULL or valid[p] != 0), and the sample point of EVERY pixel of its window is in
 * frame.  This differs from the census term: a zero inside an SSIM window would wreck its means and variances, so an
 * out-of-frame or non-finite pixel switches off every window it belongs to; `valid` still selects centres only.
 * out_sums[n] = sum over the contributing centres of sum_c term(p, c), out_counts[n] = their number (exact); H <= 2 radius or
 * W <= 2 radius: both 0, no error.  Launches as for the census term: a per-pixel pass (the C planes of y and the in-frame byte
 * to workspace), a windowed pass over 32 x 8 tiles of centres with a `radius` halo of x, y and the flag staged in the LDS, tile
 * terms added in a fixed tree, the parts in index order: two calls give the same bits.
 * workspace: at least pwc_ssim_workspace_floats(N, H, W, C, with_grad) floats, with_grad 0 for the sums and 1 for the gradient:
 *   2 * N * parts + (with_grad ? 9 : 1) * C * N * H * W + (N * H * W + 3) / 4 + (with_grad ? 1 : 0),
 * parts = min(256, ceil(W / 32) * ceil(H / 8)) -- the part sums and counts, the planes of y (gradient: and of its two
 * derivatives), the in-frame bytes, and (gradient) three planes of doubles per channel behind one float of slack for their
 * alignment.  Checks, in this order: null pointers and sizes <= 0 (PWC_EINVAL); C outside 1..4 or radius outside 1..3
 * (PWC_EUNSUPPORTED); a channel stride below the channel count, c1 or c2 <= 0 or NaN (PWC_EINVAL); H * W > 2^31 - 65537 or N > 65535
 * (PWC_ERANGE); a null or short workspace, null outputs (PWC_EINVAL). */
size_t pwc_ssim_workspace_floats(int N, int H, int W, int C, int with_grad);
int pwc_ssim_sums_f32(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                      float flow_scale, const uint8_t* valid, int N, int H, int W, int C, int radius, float c1, float c2,
                      float* workspace, size_t workspace_floats, float* out_sums, int32_t* out_counts,
                      pwc_stream_t stream);
/* dflow (+)= the gradient of sum_n dsums[n] * out_sums[n] w.r.t. the flow (the images are constants; floor and clip carry no
 * gradient).  With S = SSIM, for a pixel q in the window of centre p:
 *   dS/dy_q = (1/n) [2 mu_x A2 / (B1 B2) + 2 (x_q - mu_x) A1 / (B1 B2) - 2 S mu_y / B1 - 2 S (y_q - mu_y) / B2]
 *           = alpha_p + beta_p x_q + gamma_p y_q,
 * linear in x_q and y_q, so the gather splits: dL/dy(q) = -1/2 dsums[n] (sum_p alpha_p + x_q sum_p beta_p + y_q sum_p gamma_p)
 * over the contributing centres within `radius` of q -- one per-centre pass that writes the three coefficients per channel (as
 * doubles: they cancel), then box sums over the same tiles -- and
 *   dflow[q] = flow_scale * sum_c dL/dy_c(q) * (d sample_c / d px, d sample_c / d py).
 * A q that is out of frame, or has no contributing centre within `radius`, gets exactly 0 (accumulate == 0) or is left
 * untouched (accumulate != 0).  No atomics: two calls give the same bits.  dsums: N floats on the device. */
int pwc_ssim_grad_f32(const float* im0, int im0_cs, const float* im1, int im1_cs, const float* flow, int flow_cs,
                      float flow_scale, const uint8_t* valid, int N, int H, int W, int C, int radius, float c1, float c2,
                      const float* dsums, float* workspace, size_t workspace_floats, float* dflow, int dflow_cs,
                      int accumulate, pwc_stream_t stream);

/* ==== occlusion: forward-backward consistency of two flows (the `valid` masks of the data terms above, and the consistency term) ====
 * flow_a is the flow 0 -> 1, flow_b the flow 1 -> 0, both NHWC fp32 with 2 channels at channel strides a_cs, b_cs >= 2 (scalar
 * loads, no alignment asked).  For direction a, pixel p = (n, y, x): f = flow_scale * flow_a[p], (px, py) = (x + f0, y + f1);
 * the in-frame test 0 <= px <= W - 1, 0 <= py <= H - 1 (a NaN or Inf fails it) and the bilinear sample are the photometric
 * term's (x0 = floor(px), x1 = min(x0 + 1, W - 1), weight px - x0 on x1, the same in y); g = flow_scale * (that sample of
 * flow_b, both channels).  valid_a[p] = 1 iff (valid_a_in == NULL or valid_a_in[p] != 0) and the sample point is in frame and
 *   |f + g|^2 <= alpha1 * (|f|^2 + |g|^2) + alpha2,
 * else 0; evaluated as (right side - left side) >= 0, which is the same decision for finite values, false for a NaN on either
 * side and false where the sampled flow holds an Inf.  Direction b: the same with the roles of the flows and masks swapped.  A
 * pixel its input mask rules out reads neither flow, an out-of-frame pixel no sample (selected, not multiplied).  alpha2 is in
 * px^2 at the flows' resolution after flow_scale (UnFlow: alpha1 0.01, alpha2 0.5).  Sample point, weights, f + g and both
 * sides are computed in double: the decision is a float64 restatement's except at true near-ties.
 * valid_a, valid_b: uint8_t[N][H][W] out; valid_b NULL: only direction a is computed (counts_b must then be NULL too).
 * counts_a, counts_b: int32_t[N] out, the number of 1s per image (exact; workgroup partials added in a fixed tree, then in index
 * order: two calls give the same bits; no atomics); both may be NULL, and then no workspace is needed.  Otherwise workspace: at
 * least pwc_fb_workspace_floats(N, H, W) floats.  One launch for both directions, plus one small launch (a thread per image) per count
 * vector.  Checks, all before any launch: null flows or valid_a, N, H, W <= 0, a channel stride below 2, alpha1 or alpha2
 * negative or NaN, counts_b without valid_b (PWC_EINVAL); H * W > 2^31 - 65537 or N > 65535 (PWC_ERANGE); counts asked with a null or
 * short workspace (PWC_EINVAL). */
size_t pwc_fb_workspace_floats(int N, int H, int W);
int pwc_fb_valid_u8(const float* flow_a, int a_cs, const float* flow_b, int b_cs, float flow_scale,
                    const uint8_t* valid_a_in, const uint8_t* valid_b_in, int N, int H, int W, float alpha1, float alpha2,
                    uint8_t* valid_a, uint8_t* valid_b, int32_t* counts_a, int32_t* counts_b,
                    float* workspace, size_t workspace_floats, pwc_stream_t stream);

/* The consistency term (UnFlow's third): the same two flows, sample and in-frame test as pwc_fb_valid_u8, word for word.  For
 * direction a, e = f + g (double, rounded to fp32 once); pixel p CONTRIBUTES iff (valid_a == NULL or valid_a[p] != 0) and its
 * sample point is in frame (a NaN or Inf flow fails the test; a pixel its mask rules out reads no flow of its own direction):
 *   sums_a[n] = sum over the contributing pixels of rho(e0) + rho(e1),  counts_a[n] = their number (exact),
 * rho as in the self-supervised losses above.  Direction b: the roles swapped.  The masks are usually pwc_fb_valid_u8's outputs.
 * One launch for both directions (workgroup partials in `workspace`, at least pwc_fb_consistency_workspace_floats(N, H, W)
 * floats, added in a fixed tree), then one small launch per direction that adds the parts in index order: two calls give the
 * same bits.  Checks, all before any launch: null flows, N, H, W <= 0, a channel stride below 2, eps <= 0, q outside (0, 1],
 * a null output (PWC_EINVAL); H * W > 2^31 - 65537 or N > 65535 (PWC_ERANGE); a null or short workspace (PWC_EINVAL). */
size_t pwc_fb_consistency_workspace_floats(int N, int H, int W);
int pwc_fb_consistency_sums_f32(const float* flow_a, int a_cs, const float* flow_b, int b_cs, float flow_scale,
                                const uint8_t* valid_a, const uint8_t* valid_b, int N, int H, int W, float eps, float q,
                                float* workspace, size_t workspace_floats, float* sums_a, int32_t* counts_a,
                                float* sums_b, int32_t* counts_b, pwc_stream_t stream);
/* dflow_a, dflow_b (+)= the gradient of sum_n dsums_a[n] sums_a[n] + dsums_b[n] sums_b[n] with respect to flow_a and flow_b.
 * The masks are constants; floor and clip carry no gradient.  A flow collects two parts.  GATHER, from its own direction's
 * contributing pixels (f and the sample position):
 *   dflow_a[p,j] = flow_scale * dsums_a[n] * sum_k rho'(e_k) * (delta_kj + flow_scale * d sample_k / d pos_j).
 * SCATTER, from the other direction's contributing pixels that read one of its four corners:
 *   dflow_a[corner,k] += flow_scale * dsums_b[n] * (corner weight) * rho'(e_k).
 * Several pixels may share a corner, so the scatter adds (corner weight) * rho'(e_k) -- dsums and flow_scale are constant per
 * image and direction and are factored out, exactly -- into 64-bit FIXED-POINT accumulators of 2^-36 steps in `workspace`:
 * integer addition is associative, the result does not depend on the order in which the atomics land, two calls give the same
 * bits.  The call zeroes the accumulators (one per pixel and channel of each flow, and one poison word per flow), one launch
 * over the pixels of both directions scatters, and a finish launch over the pixels of both flows forms the pixel's gather part,
 * converts its accumulators once, multiplies by flow_scale * dsums[n] and stores the sum of the two parts.
 * RANGE of the fixed point: a contribution below 1.5e-11 vanishes; a contribution that is not finite or reaches 2^26, and a
 * non-finite entry of the dsums that scales a flow's scatter part (dsums_b for dflow_a, dsums_a for dflow_b), raise that flow's
 * poison word, and EVERY element of that dflow is then NaN; a cell whose sum reaches 2^61 (|sum| >= 2^25) is NaN.  A diverging
 * step never comes out finite.  (A non-finite dsums reaches its own direction's gather part by plain arithmetic.)
 * accumulate == 0: every pixel of both dflows is written, 0 where neither part reaches; accumulate != 0: the same values are
 * added to what is there.  dsums_a, dsums_b: N floats on the device, no host synchronisation.  workspace: 8-byte aligned, at
 * least pwc_fb_consistency_grad_workspace_bytes(N, H, W) bytes.  Checks as above, with null dsums or dflows and a dflow channel
 * stride below 2 in place of the null outputs, and a misaligned workspace with the short one (PWC_EINVAL). */
size_t pwc_fb_consistency_grad_workspace_bytes(int N, int H, int W);
int pwc_fb_consistency_grad_f32(const float* flow_a, int a_cs, const float* flow_b, int b_cs, float flow_scale,
                                const uint8_t* valid_a, const uint8_t* valid_b, int N, int H, int W, float eps, float q,
                                const float* dsums_a, const float* dsums_b, void* workspace, size_t workspace_bytes,
                                float* dflow_a, int dflow_a_cs, float* dflow_b, int dflow_b_cs, int accumulate,
                                pwc_stream_t stream);

/* ==== forward splatting: the pixels of a frame moved to where the flow sends them (a scatter; range-map occlusion) ====
 * x: N x H x W records of x_cs >= C floats, C of them used (C == 0: x may be NULL, only the coverage is computed); flow: NHWC fp32
 * with 2 channels at channel stride flow_cs >= 2; w: N x H x W floats, the weight of each SOURCE pixel, or NULL (1); valid:
 * N x H x W bytes, the source mask, or NULL (every pixel).  Scalar loads, no alignment asked of them.
 * Source pixel p = (n, y, x) has the target point px = x + flow_scale * flow[p,0], py = y + flow_scale * flow[p,1], formed in
 * double (flow_scale is a float: the product is exact).  It CONTRIBUTES iff its mask passes and px > -1, px < W, py > -1, py < H
 * (a NaN or Inf fails the test).  x0 = floor(px), wx = px - x0, likewise y; corner (y0 + dy, x0 + dx), dx, dy in {0, 1}, carries
 * b = (dx ? wx : 1 - wx) * (dy ? wy : 1 - wy) in double, and EACH corner receives b * w * x[p,c] on its own iff it lies inside the
 * frame: a point half a pixel outside still splats onto the border (UFlow's range map, softmax splatting).  Nothing is clamped.
 *   out[t,c] = sum of b * w * x[p,c] over the contributions that reach t;  coverage[t] = sum of b * w  (the splatted w).
 * normalize != 0: out[t,c] = that sum / coverage's sum, formed in double and rounded once, where the coverage's sum is > 0, and 0
 * elsewhere (average splatting; w = exp(alpha z): softmax splatting).  coverage is written either way; with w NULL it is the
 * RANGE MAP of the flow (the number of source pixels that land on t, bilinearly).
 * Several sources share a target, so the sums are 64-bit FIXED-POINT integers of 2^-36 steps in `workspace` -- N * H * W * C
 * numerators, N * H * W denominators, one poison word -- added by integer atomics: the order in which they land cannot change a
 * bit, two calls give the same bits.  Three steps on the stream: the accumulators are zeroed, one launch over the source pixels
 * scatters, one launch over the target pixels converts every accumulator once ((double)v * 2^-36).  RANGE: a contribution below
 * 2^-37 vanishes; one that is not finite or reaches 2^26 raises the poison word, and EVERY element of out and coverage is then
 * NaN (a flag, no fault); an element whose sum reaches 2^61 is NaN.  No host synchronisation, no process-wide state.
 * workspace: 8-byte aligned, at least pwc_splat_workspace_bytes(N, H, W, C) = 8 * (N * H * W * (C + 1) + 1) bytes (0 for sizes
 * that are refused).  It holds the accumulators after the call: pwc_splat_grad_f32 reads them when normalize != 0.
 * Checks, all before any launch, in this order: a null flow, N, H, W <= 0, C < 0, a null x with C > 0 (PWC_EINVAL); C > 64
 * (PWC_EUNSUPPORTED); flow_cs < 2, x_cs < C (PWC_EINVAL); H * W > 2^31 - 65537 or N > 65535 (PWC_ERANGE); a null coverage, with C > 0
 * a null out or out_cs < C (PWC_EINVAL); a null workspace (PWC_EINVAL), one off an 8-byte boundary (PWC_EALIGN), a short one
 * (PWC_EINVAL). */
size_t pwc_splat_workspace_bytes(int N, int H, int W, int C);
int pwc_splat_f32(const float* x, int x_cs, const float* flow, int flow_cs, float flow_scale, const float* w,
                  const uint8_t* valid, int N, int H, int W, int C, int normalize, void* workspace, size_t workspace_bytes,
                  float* out, int out_cs, float* coverage, pwc_stream_t stream);
/* dx, dw, dflow (+)= the gradient of sum g_out * out + sum g_cov * coverage with respect to x, w and flow; any of the three may
 * be NULL (not all), g_out and g_cov may be NULL (zeros).  The transpose of the scatter is a GATHER: no atomics, no fixed point.
 * Each contributing source pixel re-derives its corners and weights and forms over its in-frame corners k
 *   S_c = sum_k b_k g[k,c],   dx[p,c] = w S_c,   dw[p] = sum_c x[p,c] S_c + sum_k b_k g_cov[k],
 *   dflow[p,0] = flow_scale * w * (sum_c x[p,c] sum_k (db_k/dpx) g[k,c] + sum_k (db_k/dpx) g_cov[k]),  db/dpx = -+(1 - wy), -+wy,
 *   dflow[p,1] likewise with db/dpy = -+(1 - wx), -+wx,
 * each value in double, rounded once; floor carries no gradient.  A pixel that does not contribute gets exact zeros
 * (accumulate == 0) or is left alone (accumulate != 0); accumulate adds exactly what a plain call writes.
 * normalize != 0: g[k,c] above is g_out[k,c] / den_k and g_cov[k] is joined by -sum_c out[k,c] g_out[k,c] / den_k, both 0 where
 * den_k is not positive -- with den and out = num / den read in double from `workspace`, which must hold what pwc_splat_f32 left
 * there for the same inputs; a poisoned forward makes every gradient element NaN.  normalize == 0: workspace is not read.
 * Checks as pwc_splat_f32's first four; then all three outputs NULL, g_cs < C with g_out, dx_cs < C with dx, dflow_cs < 2 with
 * dflow (PWC_EINVAL); with normalize the workspace as above.  One launch. */
int pwc_splat_grad_f32(const float* x, int x_cs, const float* flow, int flow_cs, float flow_scale, const float* w,
                       const uint8_t* valid, int N, int H, int W, int C, int normalize, const float* g_out, int g_cs,
                       const float* g_cov, const void* workspace, size_t workspace_bytes, float* dx, int dx_cs, float* dw,
                       float* dflow, int dflow_cs, int accumulate, pwc_stream_t stream);

/* ---- frames of any size: fit them to the network's geometry, refit the flow to the frames' grid ----
 * The network takes frames whose height and width are multiples of 64.  These two launches sit in front of and behind a forward on
 * plain dense tensors; the forward itself is not involved.
 * Resize arithmetic of one axis (`in` source samples, `out` output samples, output index d), half-pixel centres:
 *   src = ((2 d + 1) in - out) / (2 out)   one double division of exact integers, clamped to [0, in - 1],
 *   i0 = floor(src), f = src - i0, i1 = min(i0 + 1, in - 1);
 * the value is (1 - fy) ((1 - fx) a + fx b) + fy ((1 - fx) c + fx d) in double, every operation rounded on its own, over the
 * corners a = (y0, x0), b = (y0, x1), c = (y1, x0), d = (y1, x1); it is rounded to float32 once.  An axis with in == out has
 * every weight exactly 0: the resize is a copy along it.
 *
 * Frames -> network geometry.  x: N x H x W x 3 dense, uint8_t (x_is_u8 != 0; value v enters as the float32 nearest v / 255) or
 * float32.  y: N x OH x OW x 3 dense float32, OH >= H, OW >= W.  PWC_FIT_RESIZE: the bilinear above, per axis from (H, W) to
 * (OH, OW).  PWC_FIT_PAD: y[oy, ox] = x[min(oy, H - 1), min(ox, W - 1)] (the last row and column repeated).
 * Checks, before any launch: a null pointer, N, H, W <= 0, OH < H, OW < W, an unknown mode (PWC_EINVAL); y off a 16-byte
 * boundary or a float32 x off a 4-byte one (PWC_EALIGN); N * OH * OW >= 2^31 (PWC_ERANGE).  One launch. */
#define PWC_FIT_RESIZE 0
#define PWC_FIT_PAD 1
int pwc_fit_frames_f32(const void* x, int x_is_u8, float* y, int N, int H, int W, int OH, int OW, int mode, pwc_stream_t stream);

/* Flow at network geometry -> flow on the frames' grid.  f: N x FH x FW x 2 dense float32.  y: N x H x W x 2 dense float32.
 * PWC_FIT_RESIZE: the same bilinear from (FH, FW) to (H, W); the double value of u is multiplied by the double quotient W / FW,
 * that of v by H / FH, and the product is rounded to float32 once.  PWC_FIT_PAD: y = f[:, :H, :W].
 * Checks, before any launch: a null pointer, a non-positive size, an unknown mode, PWC_FIT_PAD with FH < H or FW < W
 * (PWC_EINVAL); f or y off an 8-byte boundary (PWC_EALIGN); N * H * W or N * FH * FW >= 2^31 (PWC_ERANGE).  One launch. */
int pwc_refit_flow_f32(const float* f, float* y, int N, int FH, int FW, int H, int W, int mode, pwc_stream_t stream);

/* ---- training augmentation: affine crop of both frames, colour jitter, the flow transformed exactly ----
 * One launch prepares a training batch from whole frames: an OH x OW window of each of the N pairs, resampled through one affine
 * map per frame, jittered in colour, with the ground-truth flow carried into the augmented pair's geometry.
 * im0, im1: N x H x W x 3 dense, uint8_t (im_is_u8 != 0; value v enters as the float32 nearest v / 255) or float32.
 * flow: N x H x W x 2 dense float32 or NULL (then out_flow and out_valid are not written and may be NULL).  valid: N x H x W
 * bytes, non-zero = labelled, or NULL (every pixel labelled).  out0, out1: N x OH x OW x 3, out_flow: N x OH x OW x 2, all float32;
 * out_valid: N x OH x OW bytes (0 / 1).
 * params: N records of 32 doubles IN DEVICE MEMORY, pixel centres at integer indices:
 *    0 ..  5  M0 = (a b c; d e f): output pixel (x, y) -> frame-0 position q0 = (a x + b y + c, d x + e y + f)
 *    6 .. 11  M1, the same map into frame 1
 *   12 .. 17  I1, the inverse of M1, computed by the caller in double (the kernel inverts nothing)
 *   18 .. 23  frame 0 photometric: gain r, g, b; gamma; contrast; brightness
 *   24 .. 29  frame 1 photometric
 *   30 .. 31  zero
 * All arithmetic is double, every operation rounded on its own (no fused multiply-add), each output rounded to float32 once.
 * Frames: q is clamped to [0, W - 1] x [0, H - 1] (replicate); x0 = floor(qx), fx = qx - x0, x1 = min(x0 + 1, W - 1), likewise y;
 *   value = (1 - fy) ((1 - fx) a + fx b) + fy ((1 - fx) c + fx d) over the corners a = (y0, x0), b = (y0, x1), c = (y1, x0),
 *   d = (y1, x1); then, unless the frame's photometric record is exactly (1, 1, 1, 1, 1, 0), per channel c
 *   clamp((pow(clamp(value * gain_c, 0, 1), gamma) - 0.5) * contrast + 0.5 + brightness, 0, 1)  (gamma == 1: no pow).
 *   Identity geometry with integer c, f and the identity record: the plain crop, bit for bit.
 * Flow: (u, v) = the input flow sampled at the UN-clamped q0 -- the same bilinear, or with flow_nearest != 0 the single tap
 *   (floor(qx + 0.5), floor(qy + 0.5)); q1 = q0 + (u, v) is where the content sits in frame 1, p1 = I1 q1 where it sits in the
 *   augmented frame 1, out_flow(p) = p1 - p.  Zoom, rotation, mirror and a relative transform of frame 1 are all this formula.
 * Validity: out_valid(p) = 1 iff q0 lies in [0, W - 1] x [0, H - 1] and every tap used for the flow is labelled: the single tap
 *   in nearest mode, the four corners in bilinear mode -- a corner whose weight is exactly zero (fx == 0 or fy == 0) is not a
 *   tap: it is not read.  Where out_valid is 0, out_flow is 0, 0: an unlabelled value (the 1e10 of .flo files) is never
 *   blended into an output.
 * Checks, before any launch: a null im0, im1, params, out0 or out1, a flow with a null out_flow or out_valid, a size <= 0
 * (PWC_EINVAL); float32 frames, out0 or out1 off a 4-byte boundary, params, flow or out_flow off an 8-byte one (PWC_EALIGN);
 * N * H * W or N * OH * OW >= 2^31, N > 65535, OH > 16 * 65535 (PWC_ERANGE).  One launch; no workspace, no atomics, no random numbers. */
int pwc_augment_pairs_f32(const void* im0, const void* im1, int im_is_u8, const float* flow, const unsigned char* valid,
                          const double* params, float* out0, float* out1, float* out_flow, unsigned char* out_valid,
                          int N, int H, int W, int OH, int OW, int flow_nearest, pwc_stream_t stream);

/* ---- frame and mask pyramids: every level of a multi-scale loss from one launch ----
 * The label-free data terms take `flow_scale` = 20 / 2^level and frames "the caller has downsampled"; these two launches are that
 * caller.  factors: n_levels (1 .. 6) DISTINCT values out of 2, 4, 8, 16, 32, 64, in any order; outs[i] belongs to factors[i].
 * H and W must be multiples of the largest factor given (not of 64).
 *
 * Frames.  x: N x H x W x C dense, C = 1 .. 4, uint8_t (x_is_u8 != 0; value v enters as the float32 nearest v / 255, as in
 * the fit entry points above) or float32.  outs[i]: N x H/f x W/f x C dense float32, f = factors[i]:
 *   outs[i][n, y, x, c] = (sum of x[n, f y .. f y + f - 1, f x .. f x + f - 1, c], in double) / f^2, rounded to float32 once.
 * The order of a cell's sum is fixed by the cell: the cells of the smallest factor f0 are summed rows top to bottom, pixels left
 * to right; every larger cell is ((a + b) + c) + d over the 2 x 2 cells of half its size, a, b the upper pair.  It does not
 * depend on N, on the other images, or on how the launch is cut into workgroups: two calls give the same bits, an image gives
 * the same bits alone and in a batch.  For uint8 frames every sum is exact (each summand is a multiple of 2^-31 and a sum is at
 * most 4096: 43 bits), so the result is the correctly rounded mean whatever the order.  Every input element is read from memory
 * once; coarser levels are built inside the workgroup from the finer sums (registers, then LDS in doubles); no atomics, no
 * workspace, no status word.  A NaN or Inf makes the cells that contain it non-finite by plain arithmetic, and nothing else.
 * The loads are 16 bytes wide where x, the row pitch W * C * (1 or 4) and the piece a lane loads are multiples of 16 bytes,
 * else 4 bytes, else single bytes: the host decides, no alignment is asked of uint8 frames.
 * Checks, before any launch, in this order: a null x or outs, N, H, W <= 0 (PWC_EINVAL); C outside 1 .. 4 (PWC_EUNSUPPORTED); a
 * null factors, n_levels outside 1 .. 6 (PWC_EINVAL); a factor that is not one of the six (PWC_EUNSUPPORTED); a factor given
 * twice, H or W not a multiple of the largest factor, a null outs[i] (PWC_EINVAL); a float32 x or an outs[i] off a 4-byte
 * boundary (PWC_EALIGN); N * H * W * C >= 2^31 (PWC_ERANGE).  One launch. */
int pwc_frame_pyramid_f32(const void* x, int x_is_u8, int N, int H, int W, int C, const int* factors, float* const* outs,
                          int n_levels, pwc_stream_t stream);

/* Masks.  valid: N x H x W bytes, non-zero = valid (the masks of the loss entry points above).  For factors[i] = f the launch
 * counts, in integers, the non-zero bytes of every f x f block; outs[i]: N x H/f x W/f bytes, 1 where the count is at least
 * need[i] and 0 elsewhere (need[i] = f^2: a min-pool, need[i] = 1: a max-pool); counts: NULL, or n_levels pointers each of
 * which is NULL or N x H/f x W/f int32 that receives the counts.  The same kernel and tiles as the frames, with C = 1.
 * Checks, in this order: a null valid, outs or need, N, H, W <= 0 (PWC_EINVAL); the factors as above; H or W not a multiple of
 * the largest factor, a null outs[i], need[i] outside 1 .. f^2 (PWC_EINVAL); a counts[i] off a 4-byte boundary (PWC_EALIGN);
 * N * H * W >= 2^31 (PWC_ERANGE).  One launch. */
int pwc_mask_pyramid_u8(const unsigned char* valid, int N, int H, int W, const int* factors, const int* need,
                        unsigned char* const* outs, int* const* counts, int n_levels, pwc_stream_t stream);

/* ==== feature normalisation: one layer norm over the two feature maps of a pair, in front of the cost volume ====
 * (pwc_featnorm.hip; semantics, bounds and launch plan in DESIGN.md.)  f0, f1: N x H x W records of f0_cs / f1_cs floats, C
 * used -- the halves of a stacked 2N tensor, or one tensor and itself shifted by a frame.  For pair n, over the M = 2 H W C
 * values of f0[n] and f1[n]:
 *   mean = sum x / M,  var = sum (x - mean)^2 / M (biased),  rstd = 1 / sqrt(var + eps),
 *   y = float32(((double)x - mean) * rstd),  stats[n] = {mean, rstd} (doubles).
 * Every quantity is a double, every output is rounded once.  The variance comes from ONE pass over sums shifted by the pair's
 * first value K = f0[n][0] (d = x - K: mean = K + sum d / M, var = sum d^2 / M - (sum d / M)^2, clamped at 0): the cancellation
 * is (|mean - K| rstd)^2 ulps of a double, not (|mean| rstd)^2, and a constant pair has var == 0 exactly.
 * The sums are cut by pwc_feature_norm_parts(H, W, C) -- never by N -- and added in a fixed order: two calls give the same
 * bits, a pair gives the same bits alone and in a batch, with 16-byte accesses (C % 4 == 0, strides % 4 == 0, pointers on 16-byte
 * boundaries) and without.  A NaN or Inf makes its own pair non-finite and no other.  No atomics, no host synchronisation.
 * Launches: one where parts == 1 (H W C <= 4096: a workgroup per pair sums and applies), else two.
 * workspace: pwc_feature_norm_workspace_bytes(N, H, W, C) = 16 * N * parts bytes, 0 where parts == 1 (then it may be NULL);
 * 8-byte aligned.  The gradient needs the same amount; it may be the same memory.
 * Checks, before any launch, in this order: null f0, f1, y0, y1 or stats, N, H, W, C <= 0 (PWC_EINVAL); a channel stride below
 * C, eps negative or NaN (PWC_EINVAL); a float pointer off a 4-byte boundary (PWC_EALIGN); H * W * C >= 2^31 or N > 65535
 * (PWC_ERANGE); stats off an 8-byte boundary (PWC_EALIGN); where the workspace is needed a null one (PWC_EINVAL), one off an
 * 8-byte boundary (PWC_EALIGN), a short one (PWC_EINVAL). */
size_t pwc_feature_norm_workspace_bytes(int N, int H, int W, int C);
int pwc_feature_norm_parts(int H, int W, int C);   /* 0 for sizes the entry points refuse */
int pwc_feature_norm_f32(const float* f0, int f0_cs, const float* f1, int f1_cs, int N, int H, int W, int C, double eps,
                         void* workspace, size_t workspace_bytes, float* y0, int y0_cs, float* y1, int y1_cs, double* stats,
                         pwc_stream_t stream);
/* Its gradient.  g0, g1: upstream gradients of y0, y1; stats: what the forward wrote.  With xh = ((double)x - mean) * rstd
 * recomputed from x (never read from the rounded y), a = sum g / M, b = sum g xh / M over the pair:
 *   d = float32(rstd * (g - a - xh * b)), written, or (accumulate) added to what d0 / d1 hold (d + v, one rounding).
 * The sums as above (same parts, same order).  d0 / d1 must not overlap the inputs.  Checks as above, with g0, g1, d0, d1 in
 * place of y0, y1 and no eps.  One launch where parts == 1, else two. */
int pwc_feature_norm_grad_f32(const float* f0, int f0_cs, const float* f1, int f1_cs, const float* g0, int g0_cs,
                              const float* g1, int g1_cs, const double* stats, int N, int H, int W, int C, void* workspace,
                              size_t workspace_bytes, float* d0, int d0_cs, float* d1, int d1_cs, int accumulate,
                              pwc_stream_t stream);

/* ==== flow distillation: a student flow against a teacher flow read through a window (self-supervision) ====
 * (pwc_distill.hip; semantics, bounds and launch plan in DESIGN.md.)  student: N x h x w records of s_cs >= 2 floats, teacher:
 * N x H x W records of t_cs >= 2 floats, 2 used of each; 0 <= y0, y0 + h <= H, 0 <= x0, x0 + w <= W.  The teacher and
 * teacher_valid are read IN PLACE through the window: student pixel p = (y, x) pairs with teacher pixel P = (y + y0, x + x0).
 * teacher_valid: N x H x W bytes or NULL (every pixel); exclude: N x h x w bytes or NULL (none).  Pixel p CONTRIBUTES iff
 * teacher_valid is non-zero at P, exclude is zero at p, both teacher components at P are finite with |.| <= 1e9 (the .flo
 * sentinel rule) and both student components at p are finite.
 *   sums[n] = sum over the contributing p of rho(student[p,0] - teacher[P,0]) + rho(student[p,1] - teacher[P,1]),
 *   rho(d) = (d^2 + eps^2)^q,  counts[n] = the number of contributing p (exact).
 * Every pixel's value is a double, the sums are taken in double -- cut into parts by (h, w) alone, never by N, and added in a
 * fixed order -- and rounded to float32 once: two calls give the same bits, an image gives the same bits alone and in a batch,
 * with 8-byte accesses (even channel strides, pointers on 8-byte boundaries) and without.  A pixel that does not contribute adds
 * exactly 0; a mask that rules it out keeps its flows from being read.  No atomics, no host synchronisation.  Two launches.
 * workspace: pwc_flow_distill_workspace_bytes(N, h, w) = 12 * N * parts bytes (0 for sizes that are refused), 8-byte aligned.
 * Checks, before any launch, in this order: a null student or teacher, N, h, w, H, W < 1, a channel stride below 2, a window
 * that is not inside the teacher, eps not positive, q outside (0, 1] (PWC_EINVAL); h * w or H * W > 2^31 - 65537, N > 65535
 * (PWC_ERANGE); a flow off a 4-byte boundary (PWC_EALIGN); a null sums, counts or workspace (PWC_EINVAL), a workspace off an
 * 8-byte boundary (PWC_EALIGN), a short one (PWC_EINVAL). */
size_t pwc_flow_distill_workspace_bytes(int N, int h, int w);
int pwc_flow_distill_sums_f32(const float* student, int s_cs, const float* teacher, int t_cs, int N, int h, int w, int H, int W,
                              int y0, int x0, const uint8_t* teacher_valid, const uint8_t* exclude, double eps, double q,
                              float* sums, int32_t* counts, void* workspace, size_t workspace_bytes, pwc_stream_t stream);
/* dstudent (+)= the gradient of sum_n dsums[n] sums[n] with respect to the student; the teacher is a constant.  A contributing
 * pixel gets float32(dsums[n] * 2 q d (d^2 + eps^2)^(q - 1)) per component, formed in double and rounded once; any other pixel
 * gets 0 (accumulate == 0) or is left alone (accumulate != 0); accumulate adds exactly what a plain call writes.  A gather:
 * one lane per student pixel, no scatter, no atomics, no workspace.  dsums: N floats on the device.  dstudent: N x h x w
 * records of ds_cs >= 2 floats; it must not overlap the inputs.  Checks as above up to the flows' alignment, then a null dsums
 * or dstudent, ds_cs < 2 (PWC_EINVAL), dsums or dstudent off a 4-byte boundary (PWC_EALIGN).  One launch. */
int pwc_flow_distill_grad_f32(const float* student, int s_cs, const float* teacher, int t_cs, int N, int h, int w, int H, int W,
                              int y0, int x0, const uint8_t* teacher_valid, const uint8_t* exclude, double eps, double q,
                              const float* dsums, float* dstudent, int ds_cs, int accumulate, pwc_stream_t stream);

/* ==== flow composition: the flow a -> c from the flows a -> b and b -> c (long-range flow from consecutive pairs) ====
 * (pwc_compose.hip; semantics, bounds and launch plan in DESIGN.md.)  flow_ab, flow_bc, flow_ac: N x H x W records of ab_cs,
 * bc_cs, ac_cs >= 2 floats, 2 used of each; valid_ab, valid_bc: N x H x W bytes or NULL (every pixel); valid_ac: N x H x W bytes.
 * For pixel p = (n, y, x), f = flow_ab[p], q = (x + f0, y + f1) in double, x0 = floor(qx), x1 = min(x0 + 1, W - 1),
 * wx = qx - x0, likewise in y (pwc_fb_valid_u8's sample):
 *   flow_ac[p,k] = float32(f_k + S_k),  S_k = the sum over the four corners c of b_c flow_bc[c,k],
 *   b_c = (wx | 1 - wx)(wy | 1 - wy), everything in double, rounded once.
 * p is VALID iff valid_ab is non-zero at p, both f components are finite with |.| <= 1e9 (the .flo sentinel rule),
 * 0 <= qx <= W - 1 and 0 <= qy <= H - 1, and at EACH of the four clamped corners valid_bc is non-zero and both flow_bc
 * components are finite with |.| <= 1e9 -- whatever the corner's weight.  valid_ac[p] = 1 / 0 is that decision; an invalid
 * pixel's flow_ac is exactly (1e10f, 1e10f), the .flo sentinel.  Selection is by branch: a pixel valid_ab rules out reads no
 * flow, one whose f fails reads no corner, a NaN in a place the rule excludes reaches no output.  A gather, no workspace; with
 * 8-byte accesses (even channel strides, pointers on 8-byte boundaries) and without, the bits are the same.  flow_ac must not
 * overlap the inputs.  Checks, before the launch, in this order: a null flow_ab, flow_bc, flow_ac or valid_ac, N, H, W < 1, a
 * channel stride below 2 (PWC_EINVAL); H * W > 2^31 - 65537, N > 65535 (PWC_ERANGE); a flow off a 4-byte boundary (PWC_EALIGN).
 * One launch. */
int pwc_flow_compose_f32(const float* flow_ab, int ab_cs, const float* flow_bc, int bc_cs, const uint8_t* valid_ab,
                         const uint8_t* valid_bc, int N, int H, int W, float* flow_ac, int ac_cs, uint8_t* valid_ac,
                         pwc_stream_t stream);
/* (dflow_ab, dflow_bc) (+)= the gradient of the sum over the VALID p and k of g[p,k] flow_ac[p,k] with respect to both flows;
 * the masks are constants, floor and clamp carry no gradient, g at an invalid pixel is not read.  g: N x H x W records of
 * g_cs >= 2 floats.
 *   dflow_ab[p,j] = float32(g[p,j] + sum_k g[p,k] dS_k/dq_j) at a valid p (a gather, in double, rounded once),
 *     dS_k/dqx = (1 - wy)(B[y0,x1] - B[y0,x0]) + wy (B[y1,x1] - B[y1,x0]), B = flow_bc[.,k] -- 0 where the clamp made x1 = x0 --
 *     likewise in y; an invalid p gets 0 (accumulate == 0) or is left alone;
 *   dflow_bc[c,k] = the sum over the valid p and their corners c of b_c g[p,k] (a scatter).
 * The scatter's sums are 64-bit fixed-point integers added by integer atomics, with a step RELATIVE to the image: a first
 * launch forms m_n = max |g[p,k]| over the valid pixels of image n (order independent, on the device), contributions are
 * multiplied by the exact power of two 2^-e_n, m_n <= 2^e_n < 2 m_n, and rounded to 2^-36; the finish converts each accumulator
 * once and multiplies by 2^e_n.  So: two calls give the same bits, an image gives the same bits alone and in a batch, g times
 * a power of two gives the gradients times that power of two (short of underflow), m_n == 0 gives exact zeros, and each
 * contribution is off by at most 2^-37 2^e_n < 2^-36 m_n.  A non-finite g at a valid pixel of image n makes every element of
 * dflow_bc[n] NaN (whatever accumulate holds; other images are untouched) and reaches dflow_ab by plain arithmetic; a cell
 * whose sum reaches 2^25 2^e_n is NaN.  accumulate adds exactly what a plain call writes.  dflow_ab, dflow_bc: N x H x W
 * records of dab_cs, dbc_cs >= 2 floats; they must not overlap the inputs or each other.
 * workspace: pwc_flow_compose_grad_workspace_bytes(N, H, W) = 8 * (2 N H W + N) bytes (0 for sizes that are refused), 8-byte
 * aligned.  Checks, before any launch, in this order: a null flow_ab, flow_bc, g, dflow_ab or dflow_bc, N, H, W < 1, a channel
 * stride below 2 (PWC_EINVAL); H * W > 2^31 - 65537, N > 65535 (PWC_ERANGE); a flow or gradient off a 4-byte boundary (PWC_EALIGN); a
 * null workspace (PWC_EINVAL), one off an 8-byte boundary (PWC_EALIGN), a short one (PWC_EINVAL).  A memset and three
 * launches: per-image maximum, scatter (with the gather into dflow_ab), finish. */
size_t pwc_flow_compose_grad_workspace_bytes(int N, int H, int W);
int pwc_flow_compose_grad_f32(const float* flow_ab, int ab_cs, const float* flow_bc, int bc_cs, const uint8_t* valid_ab,
                              const uint8_t* valid_bc, int N, int H, int W, const float* g, int g_cs, void* workspace,
                              size_t workspace_bytes, float* dflow_ab, int dab_cs, float* dflow_bc, int dbc_cs, int accumulate,
                              pwc_stream_t stream);

/* ==== flow visualisation: Middlebury colour coding, frame tiles and KITTI's log-scale error map as RGB bytes ====
 * (pwc_flowvis.hip; semantics, bounds and bytes in DESIGN.md 16.)  Every value is formed in double from the float32 inputs, as
 * the sequence of IEEE operations flow_io.flow_to_color performs: no fused multiply-add, correctly rounded division and square
 * root; atan2 is the only operation that may differ from numpy's.  A flow's scale is ONE float32 product per component, applied
 * first; a pixel is KNOWN iff both products are finite with |.| <= 1e9 (the .flo sentinel rule, flow_io.flow_valid).
 *
 * max_rad[n] = the largest sqrt(u u + v v) over the pixels of image n that are known and, where valid is given, non-zero in
 * it; 0 where there is none.  flow: N x H x W records of flow_cs >= 2 floats, 2 used; valid: N x H x W bytes or NULL;
 * max_rad: N doubles, zeroed by the call itself.  A workgroup's maximum is added with one 64-bit integer atomic max on the bits
 * (non-negative doubles order as their bits do): two calls give the same bits, an image gives the same bits alone and in a
 * batch, and the value equals numpy's bit for bit.  Checks, before the memset, in this order: a null flow or max_rad, N, H,
 * W < 1, flow_cs < 2 (PWC_EINVAL); H * W > 2^31 - 65537, N > 65535 (PWC_ERANGE); flow off a 4-byte or max_rad off an 8-byte boundary
 * (PWC_EALIGN).  A memset and one launch. */
int pwc_flow_max_radius_f64(const float* flow, int flow_cs, const uint8_t* valid, int N, int H, int W, float flow_scale,
                            double* max_rad, pwc_stream_t stream);
/* A tile of an output picture: what fills the columns [x0, x0 + tile_w) of every row of every image.  Output pixel (n, y, x)
 * reads source pixel (n, y * src_h / out_h, (x - x0) * src_w / tile_w) (integer divisions: nearest neighbour with
 * infer_continuous.pyramid_montage's integers; a source of the output's height and tile_w = src_w is read one to one).
 *   PWC_VIS_FLOW       src: N x src_h x src_w records of src_cs >= 2 floats.  flow_io.flow_to_color with max_rad[n] as the
 *                      radius: (u, v) = the scaled flow, (0, 0) where it is unknown or valid (N x src_h x src_w bytes, or NULL)
 *                      is zero; scale = max_rad + DBL_EPSILON; u / scale, v / scale, rad / scale;
 *                      fk = (atan2(-v, -u) / pi + 1) / 2 * 54, k0 = floor(fk), k1 = (k0 + 1) % 55, f = fk - k0,
 *                      col = (1 - f) * wheel[k0] / 255 + f * wheel[k1] / 255; col = 1 - rad * (1 - col) where rad <= 1,
 *                      col * 0.75 elsewhere; the byte is floor(255 * col).  max_rad: N doubles on the device, each finite
 *                      and >= 0 (anything else gives unspecified colours, nothing is read out of bounds).
 *   PWC_VIS_FRAME_U8   src: N x src_h x src_w x 3 bytes, copied.
 *   PWC_VIS_FRAME_F32  src: N x src_h x src_w x 3 floats; the byte is rint(255 * x) in double, clamped to 0 .. 255, 0 for a NaN.
 *   PWC_VIS_ERROR      src: the predicted flow, gt: the ground truth (records of gt_cs >= 2 floats), neither scaled.
 *                      d = src - gt, d_err = |d|, d_mag = |gt|, n_err = min(d_err / 3.0, (d_err / d_mag) / 0.05), d_err / 3.0
 *                      where d_mag == 0; the colour of the bin lo <= n_err < hi with the edges 0, 1/16, 1/8, 1/4, 1/2, 1, 2, 4,
 *                      8, 16, inf: (49,54,149) (69,117,180) (116,173,209) (171,217,233) (224,243,248) (254,224,144) (253,174,97)
 *                      (244,109,67) (215,48,39) (165,0,38).  A pixel whose gt is unknown or zero in valid is (0,0,0); one with a
 *                      known gt and an unknown prediction gets the last bin.  No transcendental: exact. */
enum { PWC_VIS_FLOW = 0, PWC_VIS_FRAME_U8 = 1, PWC_VIS_FRAME_F32 = 2, PWC_VIS_ERROR = 3 };
#define PWC_VIS_MAX_TILES 8
typedef struct pwc_vis_tile {
    const void* src;
    const float* gt;          /* PWC_VIS_ERROR */
    const uint8_t* valid;     /* PWC_VIS_FLOW, PWC_VIS_ERROR: or NULL */
    const double* max_rad;    /* PWC_VIS_FLOW */
    int kind, src_cs, gt_cs, src_h, src_w, x0, tile_w;
    float flow_scale;         /* PWC_VIS_FLOW */
} pwc_vis_tile;
/* out: N x out_h x out_w x 3 bytes (RGB), every pixel written: from the first of the 1 .. 8 tiles whose columns hold it, (0,0,0)
 * where none does.  One launch on `stream` writes the whole batch; the table is copied into the kernel's arguments.  A lane
 * writes four consecutive pixels of the flat (N, out_h, out_w) index as three dwords wherever out is on a 4-byte boundary, the
 * tail (and every pixel of an output off that boundary) byte by byte; the bytes are the same.  Two calls give the same bytes, an
 * image gives the same bytes alone and in a batch.  out must not overlap a source.  Checks, before the launch, in this order: a
 * null tiles or out, ntiles outside 1 .. 8, N, out_h, out_w < 1, per tile a null src, src_h, src_w, tile_w < 1, columns outside
 * [0, out_w], an unknown kind, a missing max_rad / gt, a channel stride below 2 (PWC_EINVAL); out_h * out_w or a tile's
 * src_h * src_w > 2^31 - 65537, N > 65535 (PWC_ERANGE); a float source off a 4-byte, max_rad off an 8-byte boundary (PWC_EALIGN). */
int pwc_flow_vis_tiles_u8(const pwc_vis_tile* tiles, int ntiles, int N, int out_h, int out_w, uint8_t* out, pwc_stream_t stream);
/* wheel: 55 x 3 bytes, the colour wheel PWC_VIS_FLOW reads (flow_io.color_wheel(); a host copy, no launch). */
int pwc_flow_vis_wheel_u8(uint8_t* wheel);

/* ==== point tracking: query points carried through the consecutive flows of a sequence ====
 * (pwc_track.hip; semantics and launch plan in DESIGN.md 17.)  flows_fw: T x H x W records of fw_cs >= 2 floats, 2 used, the
 * flows t -> t + 1 of T + 1 frames of one size, in pixels; flows_bw: the flows t + 1 -> t in the same layout at bw_cs, or NULL;
 * valids_fw, valids_bw: T x H x W bytes or NULL (every pixel; valids_bw is not read without flows_bw).  points: P x 2 floats
 * (x, y), the flow's channel order, in frame pixels with the pixel centre at the integer; start: P int32 or NULL (all 0);
 * status_in: P bytes or NULL.  Outputs, TIME-MAJOR: tracks (T + 1) x P x 2 floats, status (T + 1) x P bytes, every element
 * written; slice t is contiguous and the last slice of one call is the state that feeds the next.
 *
 * ONE STEP carries a point in state (x, y) float32 with status s across the step flow F, checked against G where given; every
 * operation is an IEEE double + - x, a floor or a comparison in exactly this order, no fused multiply-add:
 *   s is terminal -- LEFT, UNKNOWN, OCCLUDED where stop_on_occlusion != 0 (and any byte that is no status code): position and
 *   status repeat.  Otherwise qx = (double)x, qy = (double)y and
 *   A  not (0 <= qx <= W - 1 and 0 <= qy <= H - 1) (a NaN fails)                            -> LEFT, position kept
 *      x0 = floor(qx), x1 = min(x0 + 1, W - 1), wx = qx - x0, likewise in y (the sample of the forward-backward check above)
 *   B  one of the corners (y0,x0) (y0,x1) (y1,x0) (y1,x1) is zero in F's mask, or holds a component that is not finite or
 *      exceeds 1e9 in magnitude (the .flo sentinel rule) -- all four whatever their weight  -> UNKNOWN, position kept
 *      S_k = ((1 - wy) ((1 - wx) F00_k + wx F01_k)) + (wy ((1 - wx) F10_k + wx F11_k)), k = 0, 1;  rx = qx + S_0, ry = qy + S_1
 *   C  not (0 <= rx <= W - 1 and 0 <= ry <= H - 1)                                          -> LEFT, position kept
 *   D  (G given) b = the sample of G at (rx, ry) by the same rule; a bad corner             -> UNKNOWN, position kept
 *      d_k = S_k + b_k;  bound = a1 ((S_0 S_0 + S_1 S_1) + (b_0 b_0 + b_1 b_1)) + a2, a1 = (double)alpha1, a2 = (double)alpha2;
 *      margin = bound - (d_0 d_0 + d_1 d_1);  not (margin >= 0)                             -> OCCLUDED, position (float)rx, (float)ry
 *      else VISIBLE, position ((float)rx, (float)ry): rounded once.
 * Selection is by branch: a point that fails A reads no flow, one that fails B no check flow, the flow of a masked corner is
 * not loaded.  With stop_on_occlusion == 0 an OCCLUDED point keeps stepping from where it is and may become VISIBLE again.
 *
 * A TRACK.  Point p with s0 = start[p], 0 <= s0 <= T, is VISIBLE at slice s0 at points[p] (LEFT where the query fails A) and
 * steps up to slice T with F = flows_fw[t], G = flows_bw[t] and their masks.  direction PWC_TRACK_BOTH (needs flows_bw): it
 * also steps from s0 down to slice 0, the step t -> t - 1 with F = flows_bw[t - 1], G = flows_fw[t - 1] and the masks swapped
 * likewise; PWC_TRACK_FORWARD: the slices below s0 are UNSEEN at the query position.  start[p] outside 0 .. T: every slice is
 * UNSEEN at the query position.  Where status_in is given and status_in[p] != UNSEEN, start[p] is ignored: the point enters
 * slice 0 in that state at points[p] (the streaming form).  One call over T flows equals, bit for bit, a call over the first
 * T1 followed by a call over the rest that is fed slice T1 (PWC_TRACK_FORWARD).
 *
 * One launch: a lane per point, 256-lane workgroups, at most 4096 of them (grid-stride beyond); no workspace, no atomics.  A
 * record is one 8-byte access where every float pointer is on an 8-byte boundary and both channel strides are even, else two
 * 4-byte ones; the bits are the same.  Checks, before the launch, in this order: a null flows_fw, points, tracks or status, T,
 * H, W, P < 1, a channel stride below 2, an unknown direction, PWC_TRACK_BOTH without flows_bw, with flows_bw an alpha that is
 * negative or NaN (PWC_EINVAL); H or W > 2^24 (beyond it rounding rx <= W - 1 to float32 could leave the frame), H * W >= 2^31,
 * T > 65535 (PWC_ERANGE); a float pointer or start off a 4-byte boundary (PWC_EALIGN). */
enum { PWC_TRACK_UNSEEN = 0, PWC_TRACK_VISIBLE = 1, PWC_TRACK_LEFT = 2, PWC_TRACK_OCCLUDED = 3, PWC_TRACK_UNKNOWN = 4 };
enum { PWC_TRACK_FORWARD = 0, PWC_TRACK_BOTH = 1 };
int pwc_track_points_f32(const float* flows_fw, int fw_cs, const float* flows_bw, int bw_cs, const uint8_t* valids_fw,
                         const uint8_t* valids_bw, int T, int H, int W, const float* points, const int32_t* start,
                         const uint8_t* status_in, int P, int direction, float alpha1, float alpha2, int stop_on_occlusion,
                         float* tracks, uint8_t* status, pwc_stream_t stream);

/* ==== frame interpolation: the frames between two frames, splatted along the two flows between them ====
 * (pwc_interp.hip; semantics, budget and launch plan in DESIGN.md 19.)  frames_0, frames_1: N x H x W x 3, both PWC_INTERP_U8
 * (records of 3 bytes, cs 3; a byte v is read as (double)v / 255.0) or both PWC_INTERP_F32 (records of cs >= 3 floats, 3 used,
 * widened; values in [0, 1] are what the budget below assumes).  flows_fw (0 -> 1), flows_bw (1 -> 0): N x H x W records of
 * fw_cs, bw_cs >= 2 floats, 2 used, in pixels.  valid_fw, valid_bw: N x H x W bytes or NULL (every pixel); weights_fw, weights_bw:
 * N x H x W floats or NULL, the weight of each SOURCE pixel.  times: M doubles on the HOST, 1 <= M <= 16, each in [0, 1], copied
 * into the kernels' arguments.  Outputs: frames_t N x M x H x W x 3 in the frames' dtype, dense; source N x M x H x W bytes; every
 * element written.  Every operation is an IEEE double operation in the order given here, no fused multiply-add; exp is the only
 * one whose result may differ from a restatement's (tests/interp_ref.py).
 *
 * SCATTER, per direction k (0: frame 0 along flows_fw, 1: frame 1 along flows_bw) and source pixel p = (n, y, x) with flow f:
 *   skipped where its mask is zero, or a component of f is not finite or exceeds 1e9 in magnitude (the .flo sentinel rule; a
 *   masked pixel's flow is not loaded).  Its weight w, formed ONCE:
 *     weights_k given: w = weights_k[p]; negative, NaN or Inf: skipped; >= 2^26: the poison word is raised, skipped.
 *     else q = (x + f_0, y + f_1); in frame iff 0 <= qx <= W - 1 and 0 <= qy <= H - 1; x0 = floor(qx), x1 = min(x0 + 1, W - 1),
 *       wx1 = qx - x0, wx0 = 1 - wx1, likewise in y; o_c = wy0 (wx0 O00_c + wx1 O01_c) + wy1 (wx0 O10_c + wx1 O11_c) of the OTHER
 *       frame (the forward-backward check's sample); e = ((|own_0 - o_0| + |own_1 - o_1|) + |own_2 - o_2|) / 3;
 *       w = exp(-min((double)alpha e, 10)); q out of frame: w = exp(-10).
 *   For each time t_m: s = t_m (k = 0) or 1 - t_m (k = 1); (px, py) = (x + s f_0, y + s f_1); contributes iff px > -1, px < W,
 *   py > -1, py < H (a NaN fails); x0 = floor(px), wx = px - x0, likewise y; each corner (y0 + dy, x0 + dx) inside the frame, with
 *   b = (dx ? wx : 1 - wx) (dy ? wy : 1 - wy), receives by 64-bit integer atomics llrint(v 2^36), v = (b w) colour_c (c = 0, 1, 2),
 *   b w, b.  A contribution that rounds to no step is not sent; one that is not finite or reaches 2^26 (float frames far out of
 *   [0, 1]) raises the poison word.
 * RESOLVE, per output pixel (n, m, y, x): per direction range_k = (the b sum) 2^-36, covered_k iff range_k >= (double)min_range
 *   and den_k > 0 (the b w sum), c_k = num_k / den_k (the integers as doubles).  source = covered_0 + 2 covered_1.  The value is
 *   (1 - t) c_0 + t c_1 (source 3), c_0 (1), c_1 (2), (1 - t) frames_0[n, y, x] + t frames_1[n, y, x] (0, a hole).  float frames:
 *   rounded once; bytes: rint(255 v), ties to even, clamped to [0, 255], 0 for a NaN.  With the poison word set every element is
 *   NaN (floats) or 0 (bytes) and every source code 0; a cell whose sum reached 2^61 makes its own pixel so.
 *
 * workspace: pwc_interp_workspace_bytes(N, M, H, W) = 8 (N M H W 10 + 1) bytes, 8-byte aligned, 0 for sizes the call refuses:
 * planes [n][m][k][5][H W] and the poison word.  A time's planes meet no other time's, an image's no other image's: a call cut
 * along N or along M gives the whole call's bits, and two calls give the same bits.  Three steps on `stream`: a memset, one
 * scatter launch (grid (min(ceil(N H W / 256), 4096), 2) workgroups of 256 lanes, grid-stride beyond the cap), one resolve
 * launch (a lane per four output pixels, min(ceil(N M H W / 1024), 4096) workgroups, grid-stride beyond); bytes leave as three
 * dwords per lane where frames_t is on a 4-byte boundary, floats as three 16-byte stores where it is on a 16-byte one, else one by
 * one -- the values are the same.  No host synchronisation, no process-wide state.  Checks, before the memset, in this order: a
 * null frames, flows, times, workspace or output pointer, N, H, W < 1, M outside 1 .. 16, dtypes that differ or are unknown, a
 * time outside [0, 1] or NaN, a negative or NaN alpha or min_range, a flow stride below 2, a float frame stride below 3, a byte
 * frame stride other than 3 (PWC_EINVAL); H * W >= 2^31 or a workspace size beyond size_t (PWC_ERANGE); a float pointer off a
 * 4-byte or the workspace off an 8-byte boundary (PWC_EALIGN); a workspace that is too small (PWC_EINVAL). */
enum { PWC_INTERP_U8 = 0, PWC_INTERP_F32 = 1 };
#define PWC_INTERP_MAX_TIMES 16
size_t pwc_interp_workspace_bytes(int N, int M, int H, int W);
int pwc_interp_frames(const void* frames_0, int dtype_0, int cs_0, const void* frames_1, int dtype_1, int cs_1,
                      const float* flows_fw, int fw_cs, const float* flows_bw, int bw_cs, const uint8_t* valid_fw,
                      const uint8_t* valid_bw, const float* weights_fw, const float* weights_bw, int N, int H, int W,
                      const double* times, int M, float alpha, float min_range, void* workspace, size_t workspace_bytes,
                      void* frames_t, uint8_t* source, pwc_stream_t stream);

/* ==== dominant motion: the parametric motion that explains most of a flow field, what it leaves, frames warped by it ====
 * (pwc_motion.hip; semantics, launch plan and what the tests resolve in DESIGN.md 20.)  flows: N x H x W records of flow_cs >= 2
 * floats, 2 used, in pixels; valid: N x H x W bytes or NULL (every pixel).  A pixel is KNOWN where its mask is non-zero and both
 * components are finite and at most 1e9 in magnitude (the .flo sentinel rule); a masked pixel's flow is not loaded.  Every value is
 * an IEEE double + - x /, a floor, a rint or a comparison in the order given here, no fused multiply-add and no library function:
 * tests/motion_ref.py restates all three entry points in numpy bit for bit.
 *
 * FIT.  Coordinates are normalised, xh = (x - cx) / s, yh = (y - cy) / s with cx = (W - 1) / 2, cy = (H - 1) / 2, s = max(H, W) / 2;
 * the model flow is (a0 + a1 xh) + a2 yh, (b0 + b1 xh) + b2 yh.  PWC_MOTION_TRANSLATION: a1 = a2 = b1 = b2 = 0;
 * PWC_MOTION_SIMILARITY: a1 = b2 = alpha, b1 = -a2 = beta; PWC_MOTION_AFFINE: all six.  iters + 1 passes; in each, per known pixel,
 * w = 1 (pass 0) or 1 / (1 + ((ru ru) + (rv rv)) / (scale scale)) with ru = u - ((a0 + a1 xh) + a2 yh), rv likewise, against the
 * parameters the pass before wrote (the Cauchy weight), and the twelve sums of w, w xh, w yh, (w xh) xh, (w xh) yh, (w yh) yh, w u,
 * (w xh) u, (w yh) u, w v, (w xh) v, (w yh) v plus the integer count.  Order of the sums: the image is cut into parts =
 * min(ceil(H W / 256), 256) parts, lane t of part b adds the pixels b 256 + t, + parts 256, ... in that order starting from 0.0, the
 * 256 lanes of a part add in the tree k = 128 .. 1 (lane t += lane t + k), one lane per image adds the parts in index order
 * starting from 0.0 (the rule of the loss sums, in doubles).  That lane solves the normal equations by L D L^T elimination without
 * pivoting: column j: t_ij = A_ij - l_i0 t_j0 - ... (left to right), d_j = t_jj, l_ij = t_ij / d_j; z_i = r_i - l_i0 z_0 - ...;
 * x_i = z_i / d_i - l_i+1,i x_i+1 - ... (left to right).  Affine: A = [[Sw Sx Sy] [Sx Sxx Sxy] [Sy Sxy Syy]] with the right-hand
 * sides (Su Sxu Syu) and (Sv Sxv Syv).  Similarity, unknowns (a0, b0, alpha, beta): A = [[Sw 0 Sx -Sy] [0 Sw Sy Sx] [Sx Sy Q 0]
 * [-Sy Sx 0 Q]], Q = Sxx + Syy, right-hand side (Su, Sv, Sxu + Syv, Sxv - Syu).  Translation: a0 = Su / Sw, b0 = Sv / Sw.  An image
 * is DEGENERATE where its count is below 1 / 2 / 3 (translation / similarity / affine) or a pivot fails d > 1e-9 Sw (a NaN
 * fails; translation: Sw itself): ok = 0, zero parameters, in that pass and every later one.  Outputs, every element written:
 * matrices N x 3 x 3 doubles, p' = M p for a pixel (x, y, 1): M00 = 1 + a1 / s, M01 = a2 / s, M02 = a0 - ((a1 cx) + (a2 cy)) / s,
 * M10 = b1 / s, M11 = 1 + b2 / s, M12 = b0 - ((b1 cx) + (b2 cy)) / s, then 0 0 1 (the identity where ok = 0); ok N bytes; count N
 * int32 known pixels; weight_sum N doubles, Sw of the last pass.  2 (iters + 1) launches on `stream`: sums on the grid (parts, N),
 * then solve; no atomic, no host synchronisation, no process-wide state; an image's result does not depend on its neighbours in
 * the batch and two calls give the same bits.  workspace: the size the _workspace_bytes function gives (0 for sizes the call
 * refuses), 8-byte aligned.  Checks, in this order: a null flows, workspace or output pointer, N, H, W < 1, iters outside
 * 0 .. 64, scale not > 0 (a NaN fails), flow_cs < 2, an unknown model (PWC_EINVAL); H W > 2^31 - 65537 or N > 65535 (PWC_ERANGE);
 * flows or count off a 4-byte, workspace, matrices or weight_sum off an 8-byte boundary (PWC_EALIGN); a workspace that is too
 * small (PWC_EINVAL).
 *
 * RESIDUAL, one launch, a lane per pixel (4096 workgroups of 256 lanes at most, grid-stride beyond): mu = (((M00 x) + (M01 y)) +
 * M02) - x, mv likewise; ru = u - mu, rv = v - mv; residual = ((float)ru, (float)rv), rounded once; inlier = ((ru ru) + (rv rv))
 * <= threshold threshold.  An unknown pixel, and every pixel of an image whose matrix has a last row other than exactly 0 0 1 or
 * an entry of the first two rows that is not finite, gets 1e10 in both components and inlier 0.  residual: N x H x W x 2 floats,
 * dense; inlier: N x H x W bytes.  Checks: null pointers, sizes < 1, flow_cs < 2, a negative or NaN threshold (PWC_EINVAL); the
 * range as above (PWC_ERANGE); flows or residual off a 4-byte, matrices off an 8-byte boundary (PWC_EALIGN).
 *
 * WARP, one launch, a lane per four output pixels of the flat (N, H, W) index: frames N x H x W x C dense, PWC_MOTION_U8 or
 * PWC_MOTION_F32, 1 <= C <= 4; matrices take an OUTPUT pixel to its source position, sx = ((M00 x) + (M01 y)) + M02, sy likewise.
 * Covered iff the matrix is affine and finite (as above) and 0 <= sx <= W - 1 and 0 <= sy <= H - 1 (a NaN fails); then x0 =
 * floor(sx), x1 = min(x0 + 1, W - 1), wx1 = sx - x0, wx0 = 1 - wx1, likewise in y, and per channel
 * (wy0 ((wx0 c00) + (wx1 c01))) + (wy1 ((wx0 c10) + (wx1 c11))) of the values widened to doubles (a byte v is v); floats are
 * rounded once, bytes are rint (ties to even) clamped to [0, 255].  Not covered: every channel 0, covered 0.  out: N x H x W x C
 * in the frames' dtype, covered: N x H x W bytes; bytes leave as C dwords per lane where out is on a 4-byte boundary, floats as C
 * 16-byte stores where it is on a 16-byte one, else one by one -- the values are the same.  Checks: null pointers, sizes < 1, C
 * outside 1 .. 4, an unknown dtype (PWC_EINVAL); the range as above (PWC_ERANGE); matrices off an 8-byte, float frames or out off a
 * 4-byte boundary (PWC_EALIGN). */
enum { PWC_MOTION_TRANSLATION = 0, PWC_MOTION_SIMILARITY = 1, PWC_MOTION_AFFINE = 2 };
enum { PWC_MOTION_U8 = 0, PWC_MOTION_F32 = 1 };
#define PWC_MOTION_MAX_ITERS 64
size_t pwc_motion_fit_workspace_bytes(int N, int H, int W);
int pwc_motion_fit_f64(const float* flows, int flow_cs, const uint8_t* valid, int N, int H, int W, int model, int iters,
                       double scale, void* workspace, size_t workspace_bytes, double* matrices, uint8_t* ok, int32_t* count,
                       double* weight_sum, pwc_stream_t stream);
int pwc_motion_residual_f32(const float* flows, int flow_cs, const uint8_t* valid, const double* matrices, int N, int H, int W,
                            double threshold, float* residual, uint8_t* inlier, pwc_stream_t stream);
int pwc_warp_affine(const void* frames, int dtype, int C, const double* matrices, int N, int H, int W, void* out, uint8_t* covered,
                    pwc_stream_t stream);

/* ==== moving regions: the connected components of a mask, numbered, with their areas, boxes and mean flows ====
 * (pwc_regions.hip; semantics, launch plan and what the tests resolve in DESIGN.md 21.)  mask: N x H x W bytes; flows: N x H x W
 * records of flow_cs >= 2 floats, 2 used, or NULL.  The result is defined by the input alone, not by the order in which lanes run:
 *
 *   FOREGROUND  a pixel whose mask byte is non-zero (invert != 0: whose mask byte is ZERO) and, where flows is given, whose two
 *               components are finite and at most 1e9 in magnitude (the .flo sentinel rule); the flow of a pixel the mask
 *               excludes is not loaded
 *   CONNECTED   connectivity 4: foreground pixels that share an edge; 8: an edge or a corner.  Never across images.
 *   ROOT        the smallest linear index y W + x of a component;  AREA  its pixel count;  KEPT  area >= min_area
 *   ID          the kept components of an image numbered 1 .. K by ascending ROOT (raster order of their first pixel)
 *   labels      N x H x W int32: the ID, 0 for background and for components that are not kept
 *   count       N int32: K, the true number, also where K > max_regions
 *   TABLE       for ids 1 .. min(K, max_regions), row id - 1; every other row zero; every element written:
 *               area N x R int32;  box N x R x 4 int32: x0 y0 x1 y1, inclusive  (R = max_regions)
 *               sums N x R x 2 int64 (only with flows): the sums of q = (int64) rint(clamp(u, -65536, 65536) * 65536.0), likewise v
 *               mean N x R x 2 doubles (only with flows): ((double)sum_u / 65536.0) / (double)area, likewise v -- these two
 *               divisions, in this order
 *
 * The sums are integers, the same in any order (the 64-bit fixed point of the splat and the composition).  Overflow bound: a
 * pixel adds at most 2^32 in magnitude (65536 * 65536) and an image has at most 2^26 pixels, so a sum stays below 2^58 -- which
 * is why H W > 2^26 is refused.  flows, sums and mean are NULL together or given together.
 * Ten launches on `stream` (nine without flows; the seam launch is left out where the image is one tile): clear the table; label
 * every pwc_regions_tile_h() x pwc_regions_tile_w() tile in the LDS by union-find; join the tiles along their seams with
 * agent-scope atomicMin (every read of the array in that launch is an agent-scope atomic load); flatten every pixel to its root;
 * areas by integer atomics; count, prefix and number the kept roots over min(ceil(H W / 256), 256) CONTIGUOUS chunks of the
 * linear index; labels, boxes and sums by integer atomics; the means.  No loop waits for another lane or workgroup, no host
 * synchronisation, no process-wide state, no floating-point atomic: an image's result does not depend on its neighbours in the
 * batch and two calls give the same bits.  workspace: pwc_regions_workspace_bytes (0 for sizes the call refuses), 8-byte aligned,
 * contents undefined before and after.  Checks, in this order: a null mask, workspace, labels, count, area or box, flows / sums /
 * mean not NULL together, N, H, W < 1, connectivity other than 4 or 8, min_area < 1, max_regions outside 1 .. 65535, flows given
 * with flow_cs < 2 (PWC_EINVAL); H W > 2^26 or N > 65535 (PWC_ERANGE); flows, labels, count, area or box off a 4-byte, workspace,
 * sums or mean off an 8-byte boundary (PWC_EALIGN); a workspace that is too small (PWC_EINVAL). */
int pwc_regions_tile_h(void);
int pwc_regions_tile_w(void);
size_t pwc_regions_workspace_bytes(int N, int H, int W);
int pwc_label_regions(const uint8_t* mask, int invert, const float* flows, int flow_cs, int N, int H, int W, int connectivity,
                      int min_area, int max_regions, void* workspace, size_t workspace_bytes, int32_t* labels, int32_t* count,
                      int32_t* area, int32_t* box, int64_t* sums, double* mean, pwc_stream_t stream);

/* ==== region tracking: which region of image b a region of image a becomes, identities over a sequence ====
 * (pwc_region_links.hip; semantics, launch plan and what the tests resolve in DESIGN.md 22.)  pwc_label_regions' ids are per
 * image; these entry points join the label images of consecutive pairs along the flow between them.  The result is defined by the
 * input alone, not by the order in which lanes run.
 *
 * pwc_link_regions, per image of a batch of N independent (a, b) pairs:
 *   inputs      labels_a, labels_b  N x H x W int32 (pwc_label_regions' ids; any int32 is legal input)
 *               area_a, area_b      N x R int32 (pwc_label_regions' tables), R = max_regions, 1 .. 1024
 *               flows_ab            N x H x W records of flow_cs >= 2 floats, 2 used: frame a -> frame b, pixels
 *               valid_ab            N x H x W bytes or NULL
 *   VOTER       a pixel p = (x, y) with la = labels_a[p] in 1 .. R, valid byte non-zero (where given), and both flow
 *               components finite and <= 1e9 in magnitude (the .flo sentinel rule).
 *               The flow of a pixel that is no voter for the first two reasons is not loaded.
 *   TARGET      qx = rint((double)x + (double)u), qy = rint((double)y + (double)v): one IEEE double addition each, then
 *               rint (ties to even); compared AS DOUBLES with 0 and W-1 / H-1 before any conversion to an integer
 *   VOTE        target out of frame:  left[la-1] += 1
 *               else lb = labels_b[qy, qx];  c = lb if 1 <= lb <= R else 0;  overlap[la-1][c] += 1
 *               (column 0: landed on background, or on a region beyond the table)
 *   best_succ   row a:    the c in 1 .. R with the largest overlap[a][c], ties to the SMALLEST c; 0 if all are zero
 *   best_pred   column b: the a in 1 .. R with the largest overlap[a][b], ties to the SMALLEST a; 0 if all are zero
 *   LINK a->b   best_succ[a] == b  and  best_pred[b] == a  and  overlap >= min_overlap (int, >= 1)
 *               and  (double)overlap >= min_fraction * (double)min(area_a[a-1], area_b[b-1])   (one multiply, one compare)
 *   outputs     succ N x R int32 (b or 0), pred N x R int32 (a or 0), best_succ, best_pred N x R int32,
 *               votes N x R x 4 int32: overlap[a][best_succ[a]] (0 if none), overlap[a][0], left[a], the row's voters
 * All counts are integers added by atomics, the same in any order and at most H W <= 2^26.  A split shows as several b with one
 * best_pred, a merge as several a with one best_succ; in either case only the mutual pair is a link.
 * Five launches on `stream`: clear the N x R x (R + 2) vote table (overlap[a][0 .. R] and left[a] in one row); a lane per pixel
 * votes, the lanes of a wave that hold one key issuing one atomic; a wave per row for best_succ and votes; a workgroup per 64
 * columns for best_pred; a lane per row for succ and pred.  workspace: pwc_region_links_workspace_bytes(N, R) = 4 N R (R + 2)
 * rounded up to 8 (0 for what the call refuses: N outside 1 .. 65535, R outside 1 .. 1024), 8-byte aligned, contents undefined
 * before and after.  Checks, in this order: a null pointer other than valid_ab; N, H, W or max_regions < 1; min_overlap < 1;
 * min_fraction outside [0, 1] or not finite; flow_cs < 2 (PWC_EINVAL); H W > 2^26, N > 65535 or max_regions > 1024 (PWC_ERANGE);
 * a pointer other than valid_ab off a 4-byte, the workspace off an 8-byte boundary (PWC_EALIGN); a workspace that is too small
 * (PWC_EINVAL).
 *
 * pwc_region_identities, over a sequence of S label images:
 *   inputs      pred (S-1) x R (the link s-1 -> s: pwc_link_regions on labels[:-1], labels[1:], flows[:-1]; NULL allowed where
 *               S == 1), count S int32, optionally ids_prev, age_prev, pred_prev R int32 each (the last image of an earlier call
 *               and the link from it to image 0; NULL together or given together), next_id int32 >= 1
 *   image 0     without ids_prev: row r < min(count[0], R) gets next_id + r, age 1.  With it: image 0 is treated like s >= 1.
 *   image s     row b-1 for b = 1 .. min(count[s], R):  p = pred[s-1][b-1];
 *               p in 1 .. R and ids[s-1][p-1] != 0  ->  ids[s][b-1] = ids[s-1][p-1],  age = age of that + 1
 *               else fresh: next_id + (its rank among the fresh rows of image s in ascending b),  age = 1;
 *               then next_id += the number of fresh rows
 *   rows beyond min(count[s], R): 0
 *   outputs     ids S x R int32, age S x R int32, next_id_out 1 int32 (the next_id after image S-1)
 * next_id_in, 1 int32 on the device or NULL: where given, the first fresh id is read from there (an earlier call's next_id_out,
 * so that a sequence fed in pieces needs no copy to the host) and `next_id` is the caller's upper bound of it, used for the range
 * check alone.  One launch of one workgroup; the loop over s is inside the kernel, the previous image's ids and ages are in the
 * LDS, the fresh ranks come from a ballot and a popcount per wave plus the wave totals.  Checks, in this order: a null count,
 * ids, age or next_id_out, a null pred with S > 1, ids_prev / age_prev / pred_prev not NULL together; S or max_regions < 1,
 * next_id < 1 (PWC_EINVAL); max_regions > 1024 or next_id + S R >= 2^31 (PWC_ERANGE); a pointer off a 4-byte boundary
 * (PWC_EALIGN).
 *
 * pwc_relabel_regions: out[s][p] = ids[s][la-1] for la = labels[s][p] in 1 .. R, else 0; S x H x W int32, one launch, a lane per
 * pixel.  Checks: a null pointer; S, H, W or max_regions < 1 (PWC_EINVAL); H W > 2^26, S > 65535 or max_regions > 1024
 * (PWC_ERANGE); a pointer off a 4-byte boundary (PWC_EALIGN).
 * No host synchronisation, no process-wide state, no floating-point atomic, no loop that waits for another lane or workgroup. */
size_t pwc_region_links_workspace_bytes(int N, int max_regions);
int pwc_link_regions(const int32_t* labels_a, const int32_t* labels_b, const int32_t* area_a, const int32_t* area_b,
                     const float* flows_ab, int flow_cs, const uint8_t* valid_ab, int N, int H, int W, int max_regions,
                     int min_overlap, double min_fraction, void* workspace, size_t workspace_bytes, int32_t* succ, int32_t* pred,
                     int32_t* best_succ, int32_t* best_pred, int32_t* votes, pwc_stream_t stream);
int pwc_region_identities(const int32_t* pred, const int32_t* count, const int32_t* ids_prev, const int32_t* age_prev,
                          const int32_t* pred_prev, int next_id, const int32_t* next_id_in, int S, int max_regions, int32_t* ids,
                          int32_t* age, int32_t* next_id_out, pwc_stream_t stream);
int pwc_relabel_regions(const int32_t* labels, const int32_t* ids, int S, int H, int W, int max_regions, int32_t* out,
                        pwc_stream_t stream);

/* ==== flow filter: the image-guided weighted median of a flow field, smoothing and hole filling ====
 * (pwc_flow_filter.hip; launch plan, operation counts, resource figures and what the tests resolve in DESIGN.md 23.)  The
 * weighted median over a window, with weights from spatial distance and colour similarity to the centre pixel and with unknown
 * pixels left out (Sun, Roth, Black, "Secrets of optical flow estimation").  The weights are integers and a median is a
 * selection: the result is a function of the input alone, bit for bit (tests/flow_filter_ref.py restates it in numpy).
 *
 * pwc_flow_filter_f32, per image of a batch of N:
 *   inputs      flows        H x W records of flow_cs >= 2 floats, 2 used
 *               valid        H x W bytes or NULL
 *               guide        H x W x C, C = guide_c in {1, 3}, bytes (PWC_FLOW_FILTER_U8) or floats (PWC_FLOW_FILTER_F32), dense,
 *                            or NULL (color_table is then ignored; guide_dtype and guide_c are still checked)
 *               radius r     1 .. 7
 *               space_table  (2r+1)^2 uint32 in 0 .. 65535, window raster order, ON THE DEVICE
 *               color_table  255 C + 1 uint32 in 0 .. 65535, ON THE DEVICE.  Entries above 65535 are the caller's error (a weight
 *                            is a 32-bit product); pwcnet_amd.filter_flow refuses them on the host.
 *               smooth, fill flags, at least one set;  min_count >= 1;  iters >= 1
 *   KNOWN(q)    the valid byte is non-zero (where a mask is given) and both flow components are finite and <= 1e9 in magnitude
 *               (the .flo sentinel rule, flow_io.flow_valid)
 *   GUIDE BYTE  a float guide value v becomes rint(clamp((double)v * 255.0, 0, 255)), ties to even, a NaN becomes 0; from then
 *               on both guide dtypes are bytes
 *   CANDIDATES  of a centre p: the pixels q INSIDE THE FRAME with |dx|, |dy| <= r and KNOWN(q); nothing is replicated or
 *               mirrored beyond the border.  w_q = space_table[(dy+r)(2r+1) + (dx+r)] * color_table[d],
 *               d = sum_c |guide[q,c] - guide[p,c]|; without a guide d = 0 and the colour table is not read (its factor is 1).
 *               Only candidates with w_q > 0 count: n is their number, T their sum.  Weights and sums are unsigned 64-bit
 *               integers, exact in any order.
 *   MEDIAN      floats are ordered by the key k(x) = bits(x) ^ (bits(x) >> 31 ? 0xFFFFFFFF : 0x80000000), a total order in which
 *               -0 < +0.  Per component, independently: the candidate value with the smallest key K such that
 *               2 * sum_{k(x_q) <= K} w_q >= T (the lower weighted median).  The output carries that candidate's bits.
 *   PIXEL       p KNOWN and smooth:       the medians if n >= 1, else the input bits;   out_valid 1
 *               p KNOWN and not smooth:   the input bits;                               out_valid 1
 *               p not KNOWN, fill and n >= min_count:   the medians;                    out_valid 1
 *               otherwise:                (1e10, 1e10);                                 out_valid 0
 *   PASSES      iters passes, each reading the flow and out_valid of the pass before (a hole wider than r closes from its rim
 *               inwards); guide and tables are the same in every pass.
 *   outputs     out H x W records of out_cs >= 2 floats, 2 written; out_valid H x W bytes
 * One launch per pass on `stream`, no host synchronisation, no process-wide state, no atomics; an image's result depends on that
 * image alone and two calls give the same bits.  workspace: pwc_flow_filter_workspace_bytes(N, H, W, iters) = 8 P + P rounded up
 * to 8, P = N H W, for iters > 1 (one intermediate field; the passes alternate between it and out), 8-byte aligned, contents
 * undefined before and after; NULL is fine where that is 0.
 * Checks, in this order: a null flows, space_table, out or out_valid, a null color_table with a guide; N, H or W < 1; radius
 * outside 1 .. 7; guide_c not 1 or 3 or an unknown guide_dtype (with or without a guide); neither smooth nor fill; min_count or iters < 1;
 * flow_cs or out_cs < 2; out overlapping flows, or out_valid overlapping valid; a workspace that is too small (PWC_EINVAL);
 * H W >= 2^31 or N > 65535 (PWC_ERANGE); flows, out, a table or a float guide off a 4-byte, the workspace off an 8-byte boundary
 * (PWC_EALIGN). */
enum { PWC_FLOW_FILTER_U8 = 0, PWC_FLOW_FILTER_F32 = 1 };
#define PWC_FLOW_FILTER_MAX_RADIUS 7
size_t pwc_flow_filter_workspace_bytes(int N, int H, int W, int iters);   /* 0 for iters == 1 and for sizes the call refuses */
int pwc_flow_filter_f32(const float* flows, int flow_cs, const uint8_t* valid, const void* guide, int guide_dtype, int guide_c,
                        int N, int H, int W, int radius, const uint32_t* space_table, const uint32_t* color_table,
                        int smooth, int fill, int min_count, int iters, void* workspace, size_t workspace_bytes,
                        float* out, int out_cs, uint8_t* out_valid, pwc_stream_t stream);

/* ==== temporal filter: every frame of a clip averaged with its neighbours along the motion ====
 * (pwc_temporal.hip; launch shape, bytes per pixel, resource figures and what is unmeasured in DESIGN.md 24.)  Every pixel of an
 * output frame is the weighted mean of itself and of what its trajectory through the R frames after and the R frames before
 * shows: a neighbour is read where the consecutive flows say the pixel went, weighs by how well its patch matches, and is
 * dropped -- with everything beyond it on that side -- where the walk leaves the frame, meets an unknown flow or fails the
 * forward-backward check.
 *
 * pwc_temporal_filter, one clip per call:
 *   inputs      frames       T x H x W x C, C in {1, 3}, dense, bytes (PWC_TEMPORAL_U8) or floats (PWC_TEMPORAL_F32, values in
 *                            [0, 1] expected, nothing clamped).  GREY LEVEL of a stored value: a = (double)byte, or
 *                            a = 255.0 * (double)v, a NaN reads as 0.
 *               flows_fw     (T - 1) x H x W records of fw_cs >= 2 floats, 2 used: flows_fw[j] is the flow j -> j + 1, in pixels
 *               flows_bw     the same at bw_cs: flows_bw[j] is the flow j + 1 -> j.  Both may be NULL where T == 1.
 *               valids_fw, valids_bw   (T - 1) x H x W bytes or NULL (every pixel)
 *               radius R 1 .. 8; patch P 0 .. 2; sigma > 0 in grey levels; max_distance in grey levels, <= 0: off; fb_check;
 *               alpha1, alpha2 (the forward-backward check's); [i0, i1), the frames of the clip to produce
 *   outputs     filtered (i1 - i0) x H x W x C in the frames' dtype, support (i1 - i0) x H x W bytes in 0 .. 2 R; every element
 *               written; frames i0 .. i1 - 1 in order.
 * Every operation is an IEEE double + - x /, a floor, a rint or a comparison in exactly this order, no fused multiply-add, no
 * library function (tests/temporal_ref.py restates it in numpy bit for bit).  For output frame i and pixel p = (px, py):
 *   acc_c = a_c(p), c = 0 .. C - 1;  wsum = 1;  support = 0.
 *   n = C times the number of offsets o = (ox, oy), |ox|, |oy| <= P, with p + o inside the frame.
 *   For s = +1, then s = -1:  (x, y) = ((float)px, (float)py).  For k = 1 .. R:
 *     f = i + s k outside 0 .. T - 1: this direction ends.
 *     STEP: pwc_track_points_f32's ONE STEP above (A, B, C, D, word for word) of a VISIBLE point at (x, y), with
 *       s = +1:  F = flows_fw[i + k - 1], its mask valids_fw[i + k - 1];  G = flows_bw[i + k - 1], valids_bw[i + k - 1]
 *       s = -1:  F = flows_bw[i - k], valids_bw[i - k];  G = flows_fw[i - k], valids_fw[i - k]
 *       and G not given where fb_check == 0 (step D is then skipped and G's mask is not read).  Any outcome but VISIBLE -- LEFT,
 *       UNKNOWN, OCCLUDED -- ends this direction: frame f and everything beyond it on this side contribute nothing.  Else
 *       (x, y) = ((float)rx, (float)ry), rounded once, inside the frame.
 *     SAMPLES of frame f around q = (x, y):  qx = (double)x, x0 = floor(qx), wx = qx - x0, ux = 1 - wx, likewise in y -- ONE
 *       fractional part for the whole patch.  col(j) = min(max(x0 + j, 0), W - 1), row(j) = min(max(y0 + j, 0), H - 1): the
 *       corner coordinates are clamped to the frame, each on its own (the frame replicated beyond its border).  With g the grey
 *       levels of frame f,
 *         h_c(jx, jy) = (ux g_c[row(jy)][col(jx)]) + (wx g_c[row(jy)][col(jx + 1)])
 *         b_c(o)      = (uy h_c(ox, oy)) + (wy h_c(ox, oy + 1))
 *       b_c(0, 0) is the forward-backward check's sample of frame f at q.
 *     DISTANCE: sum = 0; for oy = -P .. P, for ox = -P .. P with p + o inside the frame, for c = 0 .. C - 1:
 *       df = a_c(p + o) - b_c(o);  sum = sum + (df df).   d2 = sum / (double)n.
 *     WEIGHT: w = 1 / (1 + (d2 / (sigma sigma)));  w = 0 where max_distance > 0 and d2 > (max_distance max_distance).  The walk
 *       goes on either way.
 *     acc_c = acc_c + (w b_c(0, 0));  wsum = wsum + w;  support += 1 where w > 0.
 *   v_c = acc_c / wsum.  Bytes: rint(v_c), ties to even, clamped to [0, 255], 0 for a NaN.  Floats: (float)(v_c / 255.0).
 * T == 1: no flow is read, filtered is the input (a float NaN comes out as 0), support 0.  A piece [i0, i1) of a call over a clip
 * equals, bit for bit, the same frames of a call over any sub-clip that holds frames max(i0 - R, 0) .. min(i1 - 1 + R, T - 1).
 *
 * One launch on `stream`: a lane per output pixel in tiles of 32 x 8, 256-lane workgroups, grid (ceil(W / 32), ceil(H / 8),
 * i1 - i0).  A workgroup stages its tile of frame i with a halo of P pixels in the LDS as grey levels, then every lane walks on its
 * own; the (2P+2)^2 footprint of a neighbour is loaded once, row by row, and all (2P+1)^2 samples are formed from it.  No
 * workspace, no atomics, no host synchronisation, no process-wide state; 64-bit frame and flow offsets; two calls give the same
 * bits.  Checks, before the launch, in this order: a null frames, filtered or support, T, H or W < 1; with T > 1 a null flow or a
 * channel stride below 2; an unknown dtype, C not 1 or 3; radius outside 1 .. 8, patch outside 0 .. 2; sigma (or its square) not
 * positive and finite, a NaN max_distance; with fb_check an alpha that is negative or NaN; i0 < 0, i1 > T or i0 >= i1
 * (PWC_EINVAL); H or W > 2^24, H W >= 2^31, T > 65535, more than 65535 tile rows (PWC_ERANGE); with T > 1 a flow, with float frames
 * frames or filtered, off a 4-byte boundary (PWC_EALIGN). */
enum { PWC_TEMPORAL_U8 = 0, PWC_TEMPORAL_F32 = 1 };
#define PWC_TEMPORAL_MAX_RADIUS 8
#define PWC_TEMPORAL_MAX_PATCH 2
int pwc_temporal_filter(const void* frames, int dtype, int C, const float* flows_fw, int fw_cs, const float* flows_bw, int bw_cs,
                        const uint8_t* valids_fw, const uint8_t* valids_bw, int T, int H, int W, int radius, int patch,
                        double sigma, double max_distance, int fb_check, float alpha1, float alpha2, int i0, int i1,
                        void* filtered, uint8_t* support, pwc_stream_t stream);

/* ==== background plate: the frames of a clip registered on one canvas and voted per pixel; every frame against that plate ====
 * (pwc_plate.hip; the LDS and selection design, launch geometry, resource figures and what is unmeasured in DESIGN.md 25.)
 * Every value is an IEEE double + - x /, a floor, a rint or a comparison in the order given here, no fused multiply-add and no
 * library function: tests/plate_ref.py restates both entry points in numpy bit for bit.  AFFINE AND FINITE, of a 3 x 3 matrix of
 * doubles: WARP's rule above -- the last row exactly 0 0 1 and the six entries of the first two rows finite.
 *
 * pwc_plate_build, one clip per call:
 *   inputs      frames    T x H x W x C dense, PWC_MOTION_U8 or PWC_MOTION_F32, 1 <= C <= 4, 1 <= T <= PWC_PLATE_MAX_FRAMES
 *               matrices  T x 3 x 3 doubles, each taking a CANVAS pixel (x, y, 1) to its position in frame t (pwc_warp_affine's
 *                         convention with the canvas as the output)
 *               use       T bytes or NULL (every frame);  masks  T x H x W bytes or NULL (every pixel)
 *               the canvas size Hc x Wc;  mode PWC_PLATE_MEDIAN or PWC_PLATE_MEAN;  min_count >= 1
 *   SAMPLE      of frame t at canvas pixel (x, y):  sx = ((M00 x) + (M01 y)) + M02, sy = ((M10 x) + (M11 y)) + M12.  PRESENT iff
 *               use[t] is non-zero, the matrix is affine and finite, 0 <= sx <= W - 1 and 0 <= sy <= H - 1 (a NaN fails), the
 *               masks of all four corners below are non-zero and, for float frames, all four corners are finite in every
 *               channel (the frame of a sample that fails an earlier condition is not read).  x0 = floor(sx), x1 = min(x0 + 1,
 *               W - 1), wx1 = sx - x0, wx0 = 1 - wx1, likewise in y; per channel
 *               v = (wy0 ((wx0 c00) + (wx1 c01))) + (wy1 ((wx0 c10) + (wx1 c11))) of the values widened to doubles (a byte b is b).
 *   ROUNDED     r = rint(v), ties to even, clamped to [0, 255] for bytes; r = (float)v, one rounding, for floats.
 *   n           the number of PRESENT samples, 0 .. T.
 *   MEDIAN      per channel, independently: the element of rank (n - 1) / 2 (integer division, 0-based) of the n ROUNDED
 *               samples in ascending order -- the lower median.  Floats are ordered by the flow filter's key
 *               k(x) = bits(x) ^ (bits(x) >> 31 ? 0xFFFFFFFF : 0x80000000), so -0 < +0, and the output is one of the samples' bit
 *               patterns.
 *   MEAN        per channel: s = 0.0; s = s + v for the PRESENT samples in frame order (the doubles, not the rounded values);
 *               s / (double)n, ROUNDED.
 *   outputs     plate Hc x Wc x C in the frames' dtype, count Hc x Wc bytes = n; where n < min_count the plate is 0 in every
 *               channel (count still n).  Every element is written.
 * One launch on `stream`: a lane per canvas pixel in tiles of 32 x 8, 256-lane workgroups, min(tiles, 65536) workgroups,
 * tile-stride beyond.  MEAN keeps its sums in registers.  MEDIAN keeps the ROUNDED samples of a lane in the LDS, T x 256 dwords of
 * dynamic LDS (1 KB per frame, 64 KB at T = 64), slot j of lane l at dword 256 j + l: bytes as one dword per sample (channel c in
 * bits 8 c ..), floats one channel at a time as keys (the corners of the PRESENT samples are gathered again for each further
 * channel).  A lane reads and writes its own slots only: no barrier, no loop that waits for another lane.  Nothing is sorted: the
 * result is built from the top bit down, a round counting the samples below prefix | bit and keeping the bit iff that count is
 * <= (n - 1) / 2 (8 rounds for bytes, all channels in one; 32 for a float channel).  No atomics, no workspace, no scratch, no
 * host synchronisation, no process-wide state; 64-bit frame offsets; two calls give the same bits.
 * Checks, in this order: a null frames, matrices, plate or count; T, H, W, Hc or Wc < 1; T > PWC_PLATE_MAX_FRAMES; C outside
 * 1 .. 4; an unknown dtype or mode; min_count < 1 (PWC_EINVAL); H W or Hc Wc > 2^31 - 65537 (PWC_ERANGE); matrices off an
 * 8-byte, float frames or plate off a 4-byte boundary (PWC_EALIGN).
 *
 * pwc_plate_difference, one launch, a lane per frame pixel of the flat (T, H, W) index (4096 workgroups of 256 lanes at most,
 * grid-stride beyond):
 *   inputs      frames T x H x W x C as above (any T >= 1);  plate Hc x Wc x C in the frames' dtype, count Hc x Wc bytes
 *               (pwc_plate_build's);  matrices T x 3 x 3 doubles, each taking a FRAME pixel (x, y, 1) of frame t to its position
 *               on the canvas;  min_count >= 1;  threshold >= 0
 *   KNOWN       iff the matrix is affine and finite, 0 <= sx <= Wc - 1 and 0 <= sy <= Hc - 1 (sx, sy and the corners as in
 *               SAMPLE, on the canvas), count >= min_count at all four corners and, for floats, the pixel's own channels and
 *               the plate's four corners are finite in every channel.
 *   d           0.0; per channel in order: e = |f - s|, f the frame's value widened to double, s the plate's bilinear double v
 *               (unrounded); d = e where e > d.
 *   outputs     difference T x H x W floats: (float)d, 0 where not KNOWN;  foreground T x H x W bytes: KNOWN and d > threshold
 *               (of the double);  known T x H x W bytes.  Every element is written.
 * Checks, in this order: a null pointer; T, H, W, Hc or Wc < 1; C outside 1 .. 4; an unknown dtype; min_count < 1; a negative or
 * NaN threshold (PWC_EINVAL); H W or Hc Wc > 2^31 - 65537 or T > 65535 (PWC_ERANGE); matrices off an 8-byte, difference, float
 * frames or a float plate off a 4-byte boundary (PWC_EALIGN). */
enum { PWC_PLATE_MEDIAN = 0, PWC_PLATE_MEAN = 1 };
#define PWC_PLATE_MAX_FRAMES 64
int pwc_plate_build(const void* frames, int dtype, int C, const double* matrices, const uint8_t* use, const uint8_t* masks, int T,
                    int H, int W, int Hc, int Wc, int mode, int min_count, void* plate, uint8_t* count, pwc_stream_t stream);
int pwc_plate_difference(const void* frames, int dtype, int C, const void* plate, const uint8_t* count, const double* matrices,
                         int T, int H, int W, int Hc, int Wc, int min_count, double threshold, float* difference,
                         uint8_t* foreground, uint8_t* known, pwc_stream_t stream);

/* ==== projective motion: the homography that explains most of a flow field, and the consumers above with a division per pixel ====
 * (pwc_homography.hip, projective.h, the PROJ instantiations of pwc_motion.hip, the projective branch of pwc_plate.hip; launch
 * plan, bytes and what is unmeasured in DESIGN.md 26.)  Every value is an IEEE double + - x / or a comparison in the order given
 * here, no fused multiply-add and no library function: tests/homography_ref.py restates the fit and the position in numpy bit for
 * bit.  Flows, valid, KNOWN, the partition of the sums, the tree, the part order and the elimination are "dominant motion"'s.
 *
 * POSITION of a pixel (x, y) under a 3 x 3 matrix m0 .. m8 of doubles (projective.h), the one rule of every projective consumer:
 * the matrix is FINITE iff all nine entries are; D = ((m6 x) + (m7 y)) + m8; where D > 0 (a NaN fails) sx = (((m0 x) + (m1 y)) + m2)
 * / D and sy = (((m3 x) + (m4 y)) + m5) / D, elsewhere there is NO POSITION.  For a last row of exactly 0 0 1, D is exactly 1 and
 * sx, sy have the bits of the affine entry points.  A tiny positive D gives a huge or infinite position, which the in-frame
 * comparisons of WARP and SAMPLE reject -- what keeps the corner reads inside the image.
 *
 * FIT (pwc_homography_fit_f64), the reweighted normalised direct linear transform.  xh, yh, cx, cy, s as in dominant motion's FIT;
 * the target is x' = xh + (u / s), y' = yh + (v / s); the unknowns are g0 .. g7 of G = [[g0 g1 g2] [g3 g4 g5] [g6 g7 1]], the
 * identity (g0 = g4 = 1) before pass 0 and wherever an image is DEGENERATE.  iters + 1 passes; in each, per known pixel: w = 1
 * (pass 0); later, against the g of the pass before, D = ((g6 xh) + (g7 yh)) + 1; a pixel with !(D > 0) adds nothing to the sums of
 * that pass (it is still counted); else rx = (((((g0 xh) + (g1 yh)) + g2) / D) - x') s, ry likewise with g3 g4 g5 and y', and
 * w = (1 / (1 + (((rx rx) + (ry ry)) / (scale scale)))) / (D D) -- the Cauchy weight of the geometric residual in pixels times the
 * 1 / D^2 that turns the algebraic error into the geometric one.  With wx = w xh, wy = w yh, b = {w, wx, wy, wx xh, wx yh, wy yh}
 * and q = (x' x') + (y' y') the 23 sums are S[j] += b[j], S[6 + j] += b[j] x', S[12 + j] += b[j] y' (j = 0 .. 5) and S[17 + j] +=
 * b[j] q (j = 1 .. 5), plus the integer count of known pixels.  One lane per image adds the parts and solves, unknowns in the order
 * (g2 g0 g1 g5 g3 g4 g6 g7), the lower triangle
 *   [S0] [S1 S3] [S2 S4 S5] [0 0 0 S0] [0 0 0 S1 S3] [0 0 0 S2 S4 S5] [-S7 -S9 -S10 -S13 -S15 -S16 S20] [-S8 -S10 -S11 -S14 -S16 -S17 S21 S22]
 * with the right-hand side (S6 S7 S8 S12 S13 S14 -S18 -S19), by dominant motion's L D L^T elimination, pivot rule d > 1e-9 S0.
 * DEGENERATE: a count below 4 or a failed pivot; final, as there.  The last pass writes M = T^-1 G T: a_i = (h_i0 / s, h_i1 / s,
 * h_i2 - (((h_i0 cx) + (h_i1 cy)) / s)) for the three rows h_i of G; e0j = (s a_0j) + (cx a_2j), e1j = (s a_1j) + (cy a_2j), e2j =
 * a_2j; m = e / e22, all nine.  ok = 0 and the identity where the image is degenerate, e22 is not > 0, an m is not finite, or
 * ((m6 x) + (m7 y)) + 1 is not > 0 at one of the corners (0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1) -- the horizon would cross
 * the frame.  Outputs, workspace, launches and checks as pwc_motion_fit_f64's, without a model; 23 x 256 doubles and 256 ints of LDS.
 *
 * pwc_motion_residual_projective_f32, pwc_warp_projective, pwc_plate_build_projective, pwc_plate_difference_projective: the entry
 * points of the same names without "_projective" (pwc_warp_affine for the warp), argument for argument and check for check, with
 * "affine and finite" replaced by FINITE and the sums sx, sy replaced by POSITION.  Where there is no position the residual is
 * the sentinel and no inlier, the warp is not covered, the plate has no sample, the difference is not known. */
size_t pwc_homography_fit_workspace_bytes(int N, int H, int W);
int pwc_homography_fit_f64(const float* flows, int flow_cs, const uint8_t* valid, int N, int H, int W, int iters, double scale,
                           void* workspace, size_t workspace_bytes, double* matrices, uint8_t* ok, int32_t* count,
                           double* weight_sum, pwc_stream_t stream);
int pwc_motion_residual_projective_f32(const float* flows, int flow_cs, const uint8_t* valid, const double* matrices, int N, int H,
                                       int W, double threshold, float* residual, uint8_t* inlier, pwc_stream_t stream);
int pwc_warp_projective(const void* frames, int dtype, int C, const double* matrices, int N, int H, int W, void* out,
                        uint8_t* covered, pwc_stream_t stream);
int pwc_plate_build_projective(const void* frames, int dtype, int C, const double* matrices, const uint8_t* use,
                               const uint8_t* masks, int T, int H, int W, int Hc, int Wc, int mode, int min_count, void* plate,
                               uint8_t* count, pwc_stream_t stream);
int pwc_plate_difference_projective(const void* frames, int dtype, int C, const void* plate, const uint8_t* count,
                                    const double* matrices, int T, int H, int W, int Hc, int Wc, int min_count, double threshold,
                                    float* difference, uint8_t* foreground, uint8_t* known, pwc_stream_t stream);

/* ==== epipolar motion: the fundamental matrix that explains most of a flow field, and every pixel's Sampson distance to it ====
 * (pwc_fundamental.hip, motion_jacobi.h; launch plan, bytes and what is unmeasured in DESIGN.md 27.)  A point map -- affine or a
 * homography -- is exact only for a camera that rotates or a scene that is flat; a camera that translates through depth leaves
 * parallax, and the constraint that still holds for everything rigid is p'^T F p = 0.  Every value is an IEEE double + - x / sqrt
 * or a comparison in the order given here, no fused multiply-add; sqrt on doubles (correctly rounded) is the only library call:
 * tests/fundamental_ref.py restates it in numpy bit for bit.  Flows, valid, KNOWN, the partition of the sums, the tree and the
 * part order are "dominant motion"'s; xh, yh, cx, cy, s and the target x' = xh + (u / s), y' = yh + (v / s) are "projective
 * motion"'s: one normalisation T serves both frames.
 *
 * SAMPSON(f, x, y, x', y') for nine doubles f0 .. f8 (row-major F): l0 = ((f0 x) + (f1 y)) + f2, l1 = ((f3 x) + (f4 y)) + f5,
 * l2 = ((f6 x) + (f7 y)) + f8 (l = F p); r = ((x' l0) + (y' l1)) + l2 (= a^T f); m0 = ((f0 x') + (f3 y')) + f6, m1 = ((f1 x') +
 * (f4 y')) + f7 (l' = F^T p'); g = (((l0 l0) + (l1 l1)) + (m0 m0)) + (m1 m1).
 *
 * FIT (pwc_fundamental_fit_f64), the reweighted normalised eight-point fit; iters + 1 passes; in each, per known pixel: w = 1
 * (pass 0); later, against the F^ of the pass before (9 doubles per image in the workspace), r and g = SAMPSON(F^, xh, yh, x', y');
 * a pixel with !(g > 0) adds nothing to the sums of that pass (it is still counted); else d2 = ((r r) / g) (s s), the squared
 * Sampson distance in pixels, and w = (1 / (1 + (d2 / (scale scale)))) / g -- the Cauchy weight over the factor that turns the
 * algebraic error into the geometric one.  The pixel contributes w a a^T with a = (x' xh, x' yh, x', y' xh, y' yh, y', xh, yh, 1);
 * the 45 entries of the triangle are 36 distinct monomials and 36 sums are kept: with wx = w xh, wy = w yh, b = {w, wx, wy, wx xh,
 * wx yh, wy yh} and pa = {x', y', x' x', x' y', y' y'}: S[j] += b[j] and S[6 (m + 1) + j] += b[j] pa[m] (j = 0 .. 5, m = 0 .. 4),
 * plus the integer count of known pixels; ONE tree round over all 36 (36 x 256 doubles and 256 ints of LDS).  One lane per image
 * adds the parts in index order and solves: with a_k = P[pk] Q[qk], P = (1, x', y'), Q = (1, xh, yh), pk = (1 1 1 2 2 2 0 0 0), qk =
 * (1 2 0 1 2 0 1 2 0) and mono(i, j) the place of the product of entries i and j in (1, x, y, x x, x y, y y), entry (k, l) of the
 * symmetric 9 x 9 matrix A is S[6 mono(pk_k, pk_l) + mono(qk_k, qk_l)]; tr = A00 + A11 + ... + A88 left to right.
 * JACOBI (motion_jacobi.h, sizes 9 and 3): V = I; exactly 10 sweeps over (p, q), p < q, in row order; an entry A_pq that is
 * exactly 0 is skipped; else theta = (A_qq - A_pp) / (2 A_pq), t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt((theta theta) + 1)),
 * c = 1 / sqrt((t t) + 1), s = t c; for k other than p, q, from the old values, A_kp <- (c A_kp) - (s A_kq) and A_kq <- (s A_kp) +
 * (c A_kq) (and their mirror images); A_pp <- A_pp - (t A_pq), A_qq <- A_qq + (t A_pq), A_pq <- 0; for every k, V_kp <- (c V_kp) -
 * (s V_kq), V_kq <- (s V_kp) + (c V_kq).  Eigenvalue j is A_jj, its eigenvector column j of V.  (Six sweeps bring the off-diagonal
 * part of the test scene's matrix to 1e-13 of the trace, four do not; 10 is a choice.)
 * F^ is the eigenvector of the smallest eigenvalue e0, ties to the lowest column; e1 is the smallest of the others, ties likewise;
 * eigen = (e0 / tr, e1 / tr).  RANK 2: B_ij = ((F^_0i F^_0j) + (F^_1i F^_1j)) + (F^_2i F^_2j) (= F^^T F^), JACOBI at size 3, v the
 * eigenvector of its smallest eigenvalue (the epipole of the first frame in normalised coordinates); u_i = ((F^_i0 v0) + (F^_i1 v1))
 * + (F^_i2 v2) and F^_ij <- F^_ij - (u_i v_j): the closest rank-2 matrix.
 * DEGENERATE: fewer than 8 known pixels (no decomposition: eigen 0 0), !(e1 > 1e-9 tr) -- the flow is then a homography's, a pure
 * rotation or a flat scene, and F is not determined --, or an entry of F^, v or eigen that is not finite.  Final: a degenerate
 * image's F^ is all zeros in every later pass (every pixel is then left out) and its eigen stays that of the pass that found it.
 * The last pass writes F = T^T F^ T: a_i = (h_i0 / s, h_i1 / s, h_i2 - (((h_i0 cx) + (h_i1 cy)) / s)) for the rows h_i of F^; m_0j =
 * a_0j / s, m_1j = a_1j / s, m_2j = a_2j - (((a_0j cx) + (a_1j cy)) / s); m <- m / sqrt(m0 m0 + m1 m1 + ... + m8 m8) (left to right);
 * the entry of largest magnitude (ties to the lowest index) is made positive by negating all nine.  epipole = ((s v0) + (cx v2),
 * (s v1) + (cy v2), v2): homogeneous, not normalised, F epipole = 0 up to rounding.  ok = 0, matrices all zeros and epipole zeros
 * where the image is degenerate or an entry of m or the epipole is not finite.
 * matrices N x 9 doubles; ok N bytes; count N int32 known pixels; weight_sum N doubles, S[0] of the last pass; eigen N x 2 doubles;
 * epipole N x 3 doubles.  2 (iters + 1) launches on `stream`: sums on the grid (parts, N), then solve; no atomic, no host
 * synchronisation, no process-wide state; an image's result does not depend on its neighbours in the batch and two calls give the
 * same bits.  workspace: pwc_fundamental_fit_workspace_bytes = 8 (N parts 36 + N 9) + 4 N parts rounded up to 8 (0 for sizes the
 * call refuses), 8-byte aligned.  Checks, in pwc_homography_fit_f64's order: a null flows, workspace or output pointer, N, H, W < 1,
 * iters outside 0 .. PWC_MOTION_MAX_ITERS, scale not > 0 (a NaN fails), flow_cs < 2 (PWC_EINVAL); H W > 2^31 - 65537 or N > 65535
 * (PWC_ERANGE); flows or count off a 4-byte, workspace, matrices, weight_sum, eigen or epipole off an 8-byte boundary (PWC_EALIGN);
 * a workspace that is too small (PWC_EINVAL).
 *
 * RESIDUAL (pwc_epipolar_residual_f32), one launch, a lane per pixel (4096 workgroups of 256 lanes at most, grid-stride beyond),
 * in PIXEL coordinates: r, g = SAMPSON(F, x, y, x + u, y + v) with u, v widened to doubles; dd = |r| / sqrt(g), the Sampson distance
 * in pixels; distance = (float)dd, rounded once; inlier = dd <= threshold (of the double).  distance is 1e10 and inlier 0 where the
 * flow is unknown, valid is 0, !(g > 0), or all nine entries of the image's matrix are zero (what FIT writes with ok = 0).
 * distance: N x H x W floats; inlier: N x H x W bytes.  Checks: null pointers, sizes < 1, flow_cs < 2, a negative or NaN threshold
 * (PWC_EINVAL); the range as above (PWC_ERANGE); flows or distance off a 4-byte, matrices off an 8-byte boundary (PWC_EALIGN).
 *
 * What the model cannot see: a point that moves ALONG its epipolar line (a car ahead driving the way the camera drives) satisfies
 * the constraint; and a camera that only rotates leaves F undetermined (ok = 0; eigen shows how close a clip is to that). */
size_t pwc_fundamental_fit_workspace_bytes(int N, int H, int W);
int pwc_fundamental_fit_f64(const float* flows, int flow_cs, const uint8_t* valid, int N, int H, int W, int iters, double scale,
                            void* workspace, size_t workspace_bytes, double* matrices, uint8_t* ok, int32_t* count,
                            double* weight_sum, double* eigen, double* epipole, pwc_stream_t stream);
int pwc_epipolar_residual_f32(const float* flows, int flow_cs, const uint8_t* valid, const double* matrices, int N, int H, int W,
                              double threshold, float* distance, uint8_t* inlier, pwc_stream_t stream);

/* ==== relative pose and depth: how the camera moved between two frames, and how far away every rigid pixel is ====
 * (pwc_pose.hip, two_view.h, motion_jacobi.h; launch plan, bytes and what is unmeasured in DESIGN.md 28.)  With a calibration K =
 * [fx 0 cx; 0 fy cy; 0 0 1], the same for both frames, in pixels of the flow's grid, the fundamental matrix of "epipolar motion"
 * becomes the essential matrix E = K^T F K = [t]x R up to scale, and X' = R X + t takes a point of the first camera's frame to the
 * second's.  |t| is not observable from two views: t has unit length and every depth is in units of that baseline.  Every value is
 * an IEEE double + - x / sqrt or a comparison in the order given here, no fused multiply-add; sqrt on doubles is the only library
 * call: tests/pose_ref.py restates it in numpy bit for bit.  Flows, valid, KNOWN and the partition are "dominant motion"'s;
 * SAMPSON and JACOBI are "epipolar motion"'s.  intrinsics: N x 4 doubles fx fy cx cy; FINE: all four finite, fx > 0 and fy > 0.
 *
 * RAYS of a pixel (x, y) with flow (u, v) widened to doubles: x' = x + u, y' = y + v; d0 = ((x - cx) / fx, (y - cy) / fy, 1),
 * d1 = ((x' - cx) / fx, (y' - cy) / fy, 1).
 * TRIANGULATE(R, t, d0, d1) for a row-major R: a_r = ((R_r0 d0x) + (R_r1 d0y)) + R_r2 (a = R d0); c = d1 x a as c0 = (d1y a2) - a1,
 * c1 = a0 - (d1x a2), c2 = (d1x a1) - (d1y a0); e = d1 x t likewise, e0 = (d1y t2) - t1, e1 = t0 - (d1x t2), e2 = (d1x t1) - (d1y t0);
 * den = ((c0 c0) + (c1 c1)) + (c2 c2); Z0 = (-(((c0 e0) + (c1 e1)) + (c2 e2))) / den; Z1 = (Z0 a2) + t2.  Z0 and Z1 are the depths of
 * the point in the first and the second camera (Z1 d1 = Z0 a + t crossed with d1).  Under -t both are the exact negations.
 *
 * POSE (pwc_camera_pose_f64), three launches.
 * Decompose, a lane per image.  GOOD starts as: not all nine entries of F are zero, and the intrinsics are FINE; an image that is
 * not GOOD skips what follows.  G = F K: G_i0 = F_i0 fx, G_i1 = F_i1 fy, G_i2 = ((F_i0 cx) + (F_i1 cy)) + F_i2; E = K^T G: E_0j =
 * fx G_0j, E_1j = fy G_1j, E_2j = ((cx G_0j) + (cy G_1j)) + G_2j.  B_ij = ((E_0i E_0j) + (E_1i E_1j)) + (E_2i E_2j) (= E^T E), JACOBI
 * at size 3: v3 is the column of the smallest eigenvalue l3 (ties to the lowest column), v1 and v2 the two others in column order
 * with eigenvalues l1, l2.  s1 = sqrt(l1), s2 = sqrt(l2), s3 = l3 > 0 ? sqrt(l3) : 0; GOOD needs s1 > 0 and s2 > 0; singular =
 * (s2 / s1, s3 / s1) -- an essential matrix has (1, 0); s3 is the root of an eigenvalue, so rounding alone leaves about 1e-8 there.
 * u1_i = (((E_i0 v1_0) + (E_i1 v1_1)) + (E_i2 v1_2)) / s1, u2 likewise with v2 and s2; u3 = u1 x u2 as u3_0 = (u1_1 u2_2) -
 * (u1_2 u2_1), u3_1 = (u1_2 u2_0) - (u1_0 u2_2), u3_2 = (u1_0 u2_1) - (u1_1 u2_0), then u3 <- u3 / sqrt(((u3_0 u3_0) + (u3_1 u3_1)) +
 * (u3_2 u3_2)).  c = v1 x v2 in the same form and det = ((c0 v3_0) + (c1 v3_1)) + (c2 v3_2); det < 0 negates v3.  The singular values
 * are forced to (1, 1, 0): R_a = U W V^T, entry (r, c) = ((u2_r v1_c) - (u1_r v2_c)) + (u3_r v3_c); R_b = U W^T V^T, entry (r, c) =
 * ((u1_r v2_c) - (u2_r v1_c)) + (u3_r v3_c); t = u3.  GOOD needs every entry of R_a, R_b, t, E and singular finite.  Candidates, in this
 * order: 0 (R_a, +t), 1 (R_a, -t), 2 (R_b, +t), 3 (R_b, -t).  essential = E and singular as above where GOOD, zeros elsewhere.
 * Vote, grid (parts, N), only for a GOOD image.  A pixel is a voter when it is KNOWN, r, g = SAMPSON(F, x, y, x', y') has g > 0 and
 * (|r| / sqrt(g)) <= threshold -- RESIDUAL's inlier rule.  With RAYS and TRIANGULATE(R_a, t) and TRIANGULATE(R_b, t): candidate 0
 * (2) gets the pixel's vote when den > 0, Z0 > 0 and Z1 > 0; candidate 1 (3) when den > 0, Z0 < 0 and Z1 < 0.  The counts are
 * integers: a lane's registers, a butterfly over the wave, the four waves through the LDS, one integer atomic per count and
 * workgroup -- the same in any order.
 * Select, a lane per image: the winner is the candidate with the most votes, ties to the lowest index.  ok = 1 where the image is
 * GOOD, voters > 0 and 2 votes[winner] > voters (an ambiguous vote is a failure); rotation and translation are the winner's
 * (translation negated for candidates 1 and 3); where ok = 0 both are all zeros.  votes and voters are zeros where not GOOD.
 * rotation N x 9, translation N x 3 doubles; ok N bytes; votes N x 4, voters N int32; singular N x 2, essential N x 9 doubles.
 * workspace: pwc_camera_pose_workspace_bytes = 8 x 22 N (0 for N < 1 or N > 65535), 8-byte aligned.  No host synchronisation, no
 * floating-point atomic; an image's result does not depend on its neighbours in the batch and two calls give the same bits.
 * Checks: a null pointer but valid, N, H, W < 1, flow_cs < 2, a negative or NaN threshold (PWC_EINVAL); H W > 2^31 - 65537 or N >
 * 65535 (PWC_ERANGE); flows, votes or voters off a 4-byte, any double array or the workspace off an 8-byte boundary (PWC_EALIGN);
 * a workspace that is too small (PWC_EINVAL).
 *
 * DEPTH (pwc_triangulate_depth_f32), one launch, a lane per pixel (4096 workgroups of 256 lanes at most, grid-stride beyond),
 * RESIDUAL's flow loads.  An image is OFF where all nine entries of its rotation are zero (what POSE writes with ok = 0) or its
 * intrinsics are not FINE.  Per pixel RAYS and TRIANGULATE(R, t).  Where a2 > 0: ex = x' - ((fx (a0 / a2)) + cx), ey = y' - ((fy
 * (a1 / a2)) + cy), pp = sqrt((ex ex) + (ey ey)): the distance in pixels between where the point is seen and where a point at
 * infinity on the same ray would be; the relative error of the depth is about the flow's error over pp.  known = 1 and depth =
 * (float)Z0, rounded once -- the depth in the FIRST camera in baselines -- where the image is not OFF, the pixel is KNOWN, a2 > 0,
 * den > 0, Z0 > 0, Z1 > 0 and pp >= min_parallax; elsewhere known = 0 and depth = 1e10.  parallax (may be null) = (float)pp where
 * the image is not OFF, the pixel is KNOWN and a2 > 0, else 0.  The epipolar constraint is NOT tested: a pixel that moves on its
 * own gets a meaningless depth, so pass RESIDUAL's inlier as valid.  Checks: null pointers but valid and parallax, sizes < 1,
 * flow_cs < 2, a negative or NaN min_parallax (PWC_EINVAL); the range as above (PWC_ERANGE); flows, depth or parallax off a
 * 4-byte, rotation, translation or intrinsics off an 8-byte boundary (PWC_EALIGN).
 *
 * What this cannot do: the scale of t; a scene that moves; pixels near the epipole, where pp is small and the depth is noise; a
 * camera that only rotates (FIT's ok = 0 upstream: F is all zeros and so is everything here). */
size_t pwc_camera_pose_workspace_bytes(int N);
int pwc_camera_pose_f64(const float* flows, int flow_cs, const uint8_t* valid, const double* matrices, const double* intrinsics,
                        int N, int H, int W, double threshold, void* workspace, size_t workspace_bytes, double* rotation,
                        double* translation, uint8_t* ok, int32_t* votes, int32_t* voters, double* singular, double* essential,
                        pwc_stream_t stream);
int pwc_triangulate_depth_f32(const float* flows, int flow_cs, const uint8_t* valid, const double* rotation,
                              const double* translation, const double* intrinsics, int N, int H, int W, double min_parallax,
                              float* depth, uint8_t* known, float* parallax, pwc_stream_t stream);

/* ==== scale chain and camera trajectory: one unit of length for the pairs of a sequence, and the camera's path in it ====
 * (pwc_trajectory.hip, two_view.h; launch plan, digit choice, bytes and what is unmeasured in DESIGN.md 29.)  The T pairs of ONE
 * sequence: pair j is frames j -> j + 1 with the pose (R_j, t_j), |t_j| = 1, and the depth map of "relative pose and depth" in the
 * baseline b_j of that pair.  A SEAM j lies between pair j - 1 and pair j: a rigid point that pair j - 1 sees has two depths in
 * camera j, Z1 in baselines of pair j - 1 and d in baselines of pair j, and Z1 / d = b_j / b_(j-1).  RAYS, TRIANGULATE, KNOWN and
 * FINE are "relative pose and depth"'s; the same arithmetic rules hold: IEEE double + - x / in the order given, no fused
 * multiply-add; floor is the only library call; tests/trajectory_ref.py restates both entry points in numpy bit for bit.
 *
 * LINKS (pwc_scale_links_f32).  Inputs: flows T x H x W records of flow_cs floats; rotation T x 9, translation T x 3, intrinsics
 * T x 4 doubles; depth T x H x W floats and known T x H x W bytes as DEPTH wrote them.  Optionally ONE previous pair (prev_flow not
 * null: prev_flow H x W records of prev_cs floats, prev_rotation, prev_translation, prev_intrinsics, prev_known; its depth map is not
 * read): seam 0 then lies between it and pair 0.  Seams: 1 .. T - 1, and 0 with a previous pair.
 * A seam is DEAD where either pair's rotation is all zeros (POSE's ok = 0) or the EARLIER pair's intrinsics are not FINE.
 * SAMPLE of pixel p = (x, y) of the earlier pair, in this order; a failing step ends it (the pixel is no sample):
 *   the seam is not DEAD; known[p] of the earlier pair is not 0; its flow (u, v) is KNOWN;
 *   q = (qx, qy) = (x + u, y + v) in doubles lies in the frame: 0 <= qx <= W - 1 and 0 <= qy <= H - 1;
 *   x0 = floor(qx), y0 = floor(qy), x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1); the LATER pair's known is not 0 at ALL FOUR
 *   corners (y0, x0), (y0, x1), (y1, x0), (y1, x1), whatever their weight -- "flow composition"'s rule for a sample, not a second one;
 *   wx1 = qx - x0, wy1 = qy - y0, wx0 = 1 - wx1, wy0 = 1 - wy1; with the later pair's depths widened to doubles
 *   top = (wx0 D(y0,x0)) + (wx1 D(y0,x1)), bot = (wx0 D(y1,x0)) + (wx1 D(y1,x1)), d = (wy0 top) + (wy1 bot);
 *   RAYS with the earlier pair's intrinsics (x' = qx, y' = qy) and TRIANGULATE with its pose: den > 0, Z1 > 0, d > 0;
 *   r = (float)(Z1 / d), rounded once, is finite and > 0.
 * WHICH WAY ROUND: r = Z1 / d = b_j / b_(j-1) is what multiplies scale[j - 1] to give scale[j], where scale[j] is pair j's baseline
 * in the unit of its segment (TRAJECTORY); the quotient d / Z1 of the two depth maps is its reciprocal.
 * samples[j] = n, the samples of seam j; ratio[j] = the sample of rank (n - 1) / 2 (integer division) in ascending order, the LOWER
 * median; n = 0: ratio[j] = 0.  Without a previous pair ratio[0] = 0 and samples[0] = 0.
 * The selection is exact.  The bits of a positive float32 order as unsigned integers do; the key of a pixel is the bits of r, 0 for
 * no sample.  Digits: 11 bits (key >> 21), 11 bits ((key >> 10) & 2047), 10 bits (key & 1023).  Launches, each reading what the one
 * before wrote: keys (grid (parts, seams), "dominant motion"'s partition: the keys into the workspace and the first digit's
 * histogram), then per digit a select (a workgroup per seam: the bin b with before <= rank < before + count[b], bins in ascending
 * order; rank -= before) and, for the second and third digit, a histogram of that digit over the keys whose higher digits are the
 * chosen ones.  A workgroup's histogram is in the LDS and is merged into the seam's table with one integer atomic per non-empty bin.
 * Integers only: the result is the same bits on every run; no floating-point atomic, no sort, no host synchronisation, no lane or
 * workgroup waits for another.  A seam's result does not depend on the other seams.
 * workspace: pwc_scale_links_workspace_bytes(T, H, W, has_prev) = 4 (seams (4 + 5120) + seams H W) + 16, 0 for a size < 1, H W >
 * 2^26 or T > 65535; 8-byte aligned.  Checks: a null pointer but the prev_ ones, a previous pair that is given in part, sizes < 1, a
 * channel stride < 2, a workspace that is too small (PWC_EINVAL); H W > 2^26 or T > 65535 (PWC_ERANGE); flows, depth, ratio or samples
 * off a 4-byte, a double array or the workspace off an 8-byte boundary (PWC_EALIGN).
 *
 * TRAJECTORY (pwc_camera_trajectory_f64), one launch, one lane, the pairs in order.  OK(j): pair j's rotation is not all zeros.
 * State before pair 0: [A | c] = [I | 0], scale = 0, seg = -1, opened = 0, before = false; or, with prev_rotation not null, [A | c] =
 * prev_row (3 x 4 row-major), scale = prev_scale[0], seg = prev_segment[0], opened = prev_segment[1], before = (prev_rotation is not
 * all zeros).  For j = 0 .. T - 1:
 *   linked[j] = OK(j) and before and samples[j] >= min_samples and ratio[j] is finite and > 0;
 *   OK(j) and not linked[j]: [A | c] = [I | 0] -- a new segment starts, the world frame restarts at this pair's first camera;
 *   trajectory[j] = [A | c];
 *   not OK(j): scale = 0, seg = -1;  linked[j]: scale = scale x (double)ratio[j];  else: scale = 1, seg = opened, opened += 1;
 *   scales[j] = scale, segment[j] = seg;
 *   OK(j): A <- R_j A, entry (r, q) = ((R_r0 A_0q) + (R_r1 A_1q)) + (R_r2 A_2q), and c_r <- (((R_r0 c_0) + (R_r1 c_1)) + (R_r2 c_2)) +
 *   (scale t_r) (from the old c);  not OK(j): [A | c] = [I | 0];
 *   before = OK(j).
 * trajectory[T] = [A | c]; segment_state = (seg, opened).  trajectory is world-to-camera, X_cam_i = A_i X_world + c_i, the world
 * being the first camera of the frame's segment and every length in the baseline of that segment's first pair: depth[j] x scales[j]
 * is pair j's depth in that unit.  Frame j is the LAST camera of one segment and the FIRST of the next where a segment starts at
 * pair j: its row holds [I | 0], the start.  The frame after a pair that is not OK holds [I | 0].
 * STREAMING: a sequence fed in pieces, each call given the piece before's last pair as the previous pair of LINKS and trajectory[T]
 * of that call, scales[T - 1] and segment_state as prev_row, prev_scale and prev_segment, gives the bits of one call; row 0 of a call
 * is the final word on the frame it shares with the call before (it replaces that call's last row).
 * trajectory (T + 1) x 12, scales T doubles; segment T int32; linked T bytes; segment_state 2 int32.  Checks: a null pointer but the
 * prev_ ones, prev_rotation given without the other three, T < 1, min_samples < 1 (PWC_EINVAL); T > 65535 (PWC_ERANGE); a double
 * array off an 8-byte, ratio, samples or an int32 array off a 4-byte boundary (PWC_EALIGN).
 *
 * What this cannot do: a point that moves along its epipolar line has a consistent but wrong depth in both pairs and is a sample; a
 * pair that only rotates is not OK and breaks the chain (nothing bridges it); the scale is a running product, so its error grows with
 * the length of the clip -- no loop closure, no refinement; segments do not share a unit. */
size_t pwc_scale_links_workspace_bytes(int T, int H, int W, int has_prev);
int pwc_scale_links_f32(const float* flows, int flow_cs, const double* rotation, const double* translation, const double* intrinsics,
                        const float* depth, const uint8_t* known, int T, int H, int W, const float* prev_flow, int prev_cs,
                        const double* prev_rotation, const double* prev_translation, const double* prev_intrinsics,
                        const uint8_t* prev_known, void* workspace, size_t workspace_bytes, float* ratio, int32_t* samples,
                        pwc_stream_t stream);
int pwc_camera_trajectory_f64(const double* rotation, const double* translation, const float* ratio, const int32_t* samples, int T,
                              int min_samples, const double* prev_rotation, const double* prev_row, const double* prev_scale,
                              const int32_t* prev_segment, double* trajectory, double* scales, int32_t* segment, uint8_t* linked,
                              int32_t* segment_state, pwc_stream_t stream);

/* ==== pose refinement: the pose of "relative pose and depth" fitted to the Sampson distance of its inliers, five parameters ====
 * (pwc_pose_refine.hip, two_view.h, motion_ldlt.h; launch plan, bytes and what is unmeasured in DESIGN.md 30.)  POSE stops at the
 * closed form: an algebraic fit with eight unknowns, projected.  This is the textbook next step, a reweighted Gauss-Newton fit of
 * the five parameters of (R, t), |t| = 1, to the Sampson distance in pixels over a FIXED set of pixels.  Flows, valid, KNOWN, the
 * partition of the sums, the tree, the part order and the L D L^T elimination are "dominant motion"'s; RAYS, FINE and the vectors a,
 * c, e of TRIANGULATE are "relative pose and depth"'s; the same arithmetic rules hold: IEEE double + - x / sqrt and comparisons in
 * the order given, no fused multiply-add, sqrt the only library call; tests/pose_refine_ref.py restates it in numpy bit for bit.
 * Inputs: flows, valid, intrinsics as POSE's; rotation0 N x 9 and translation0 N x 3 doubles as POSE wrote them (they are read in
 * every pass and may not overlap an output).  An image is OFF where all nine entries of its rotation0 are zero or its intrinsics
 * are not FINE: its outputs are all zeros, ok = 0, and its workgroups return before any pixel is read.
 *
 * EPIPOLAR(R, t, d0, d1): a, c, e as in TRIANGULATE; r = ((e0 a0) + (e1 a1)) + (e2 a2) (= d1 . (t x a) = d1^T E d0 with E = [t]x R);
 * l0 = ((t1 a2) - (t2 a1)) / fx, l1 = ((t2 a0) - (t0 a2)) / fy (the first two entries of E d0 = t x a, taken to pixels); m0 =
 * (((R_00 e0) + (R_10 e1)) + (R_20 e2)) / fx, m1 = (((R_01 e0) + (R_11 e1)) + (R_21 e2)) / fy (of E^T d1 = R^T e); g = (((l0 l0) +
 * (l1 l1)) + (m0 m0)) + (m1 m1).  r r / g is the squared Sampson distance in pixels.
 * BASIS(t): i the index of the entry of t smallest in magnitude, ties to the lowest index; v = e_i x t, that is (0, -t2, t1), (t2, 0,
 * -t0) or (-t1, t0, 0); nrm = sqrt((p p) + (q q)) with (p, q) = (t2, t1), (t2, t0) or (t1, t0); b1 = v / nrm entry by entry (a negated
 * entry is negated first; the zero entry is 0); b2 = t x b1 as b2_0 = (t1 b1_2) - (t2 b1_1), b2_1 = (t2 b1_0) - (t0 b1_2), b2_2 =
 * (t0 b1_1) - (t1 b1_0).
 * THE SET, the same in every pass: a pixel that is KNOWN, with RAYS and r, g = EPIPOLAR(rotation0, translation0) has g > 0 and
 * (|r| / sqrt(g)) <= threshold.  threshold = +inf admits every known pixel with g > 0.  samples = the pixels of the set.
 * PASS k = 0 .. iters against the pose theta_k = (R, t): theta_0 is the input, theta_k+1 what the solve of pass k wrote into the
 * workspace (with BASIS of its t).  Per pixel of the set: r, g = EPIPOLAR(R, t); a pixel with !(g > 0) adds nothing to this pass;
 * sg = sqrt(g), rho = r / sg, d2 = (r r) / g, w = 1 / (1 + (d2 / (scale scale))) -- the Cauchy weight; J0 = ((a1 e2) - (a2 e1)) / sg,
 * J1 = ((a2 e0) - (a0 e2)) / sg, J2 = ((a0 e1) - (a1 e0)) / sg (a x e: the derivative of r by a left rotation of R), J3 = (-(((c0
 * b1_0) + (c1 b1_1)) + (c2 b1_2))) / sg, J4 likewise with b2 (by a step of t along b1, b2): the derivative of rho with g HELD FIXED.
 * With wJ_i = w J_i the 22 sums are S[i (i + 1) / 2 + j] += wJ_i J_j (j <= i: the triangle of sum w J J^T, 15), S[15 + i] += wJ_i rho
 * (5), S[20] += w, S[21] += w d2 (the cost: sum of d2 / (1 + d2 / scale^2), Geman-McClure's bounded function), plus the integer
 * count of the set; lanes in "dominant motion"'s lane order, ONE tree round over all 22 (22 x 256 doubles and 256 ints of LDS), and
 * one lane per image adds the parts in index order.
 * SOLVE of pass k, that lane.  Pass 0: ok = 1 where the image is not OFF and samples >= 5; else every output but samples is 0 and the
 * image is frozen.  best = theta_0: rotation, translation = the input's bits, best_pass = 0, weight_sum = S[20], cost[0] = S[21].
 * Pass k > 0 of an image that is not frozen: a sum that is not finite freezes the image (cost[k] = 0); else cost[k] = S[21] and,
 * where S[21] < cost[best_pass] -- strictly: ties stay with the earlier pass --, rotation, translation = theta_k, best_pass = k,
 * weight_sum = S[20].  A pass that a frozen image skips has cost 0.  For k < iters the STEP: the 5 x 5 system (sum w J J^T) x = -(sum
 * w J rho), tr = (((S[0] + S[2]) + S[5]) + S[9]) + S[14], motion_ldlt at size 5 with the right-hand side (-S[15], .., -S[19]) and the
 * pivot rule d > 1e-9 tr (a NaN fails); x = (omega (3), beta1, beta2).  UPDATE: a = omega / 2 entry by entry, q = ((a0 a0) + (a1
 * a1)) + (a2 a2), p = 1 - q, den = 1 + q; the Cayley map C = ((1 - q) I + 2 a a^T + 2 [a]x) / den as C_ii = (p + (2 (a_i a_i))) / den,
 * C_01 = ((2 (a0 a1)) - (2 a2)) / den, C_02 = ((2 (a0 a2)) + (2 a1)) / den, C_10 = ((2 (a1 a0)) + (2 a2)) / den, C_12 = ((2 (a1 a2)) -
 * (2 a0)) / den, C_20 = ((2 (a2 a0)) - (2 a1)) / den, C_21 = ((2 (a2 a1)) + (2 a0)) / den -- rational, orthogonal up to rounding, no
 * sine or cosine; R <- C R, entry (r, c) = ((C_r0 R_0c) + (C_r1 R_1c)) + (C_r2 R_2c); u_i = (t_i + (beta1 b1_i)) + (beta2 b2_i) with
 * BASIS(t), t <- u / sqrt(((u0 u0) + (u1 u1)) + (u2 u2)).  A sum of pass 0 that is not finite, a failed pivot, or an entry of the new
 * R or t that is not finite FREEZES the image: it keeps its best pose so far and its later passes add nothing.
 * By construction iters = 0 returns the input pose bit for bit with its cost, and cost[best_pass] <= cost[0] for any iters.
 * rotation N x 9, translation N x 3 doubles; ok N bytes; samples, best_pass N int32; cost N x (iters + 1), weight_sum N doubles; every
 * element is written.  2 (iters + 1) launches on `stream`: sums on the grid (parts, N), then solve; no atomic, no host
 * synchronisation, no process-wide state; an image's result does not depend on its neighbours in the batch and two calls give the
 * same bits.  workspace: pwc_pose_refine_workspace_bytes = 8 (N parts 22 + N 19) + 4 N parts rounded up to 8 (0 for sizes the call
 * refuses), 8-byte aligned.  Checks, in pwc_camera_pose_f64's order: a null pointer but valid, N, H, W < 1, iters outside 0 ..
 * PWC_MOTION_MAX_ITERS, scale not > 0 (a NaN fails), a negative or NaN threshold, flow_cs < 2 (PWC_EINVAL); H W > 2^31 - 65537 or N >
 * 65535 (PWC_ERANGE); flows, samples or best_pass off a 4-byte, any double array or the workspace off an 8-byte boundary
 * (PWC_EALIGN); a workspace that is too small (PWC_EINVAL).
 *
 * What this cannot do: what the closed form cannot -- a point that moves along its epipolar line, a camera that only rotates (OFF
 * here); it refines one pair at a time and no structure: no bundle adjustment over a sequence; a bad start stays bad (the set is
 * chosen by the input pose).  scale, threshold, iters, the pivot rule and the fixed-g Jacobian are choices nobody has tuned. */
size_t pwc_pose_refine_workspace_bytes(int N, int H, int W);
int pwc_pose_refine_f64(const float* flows, int flow_cs, const uint8_t* valid, const double* intrinsics, const double* rotation0,
                        const double* translation0, int N, int H, int W, int iters, double scale, double threshold, void* workspace,
                        size_t workspace_bytes, double* rotation, double* translation, uint8_t* ok, int32_t* samples,
                        int32_t* best_pass, double* cost, double* weight_sum, pwc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PWC_HIP_H */
