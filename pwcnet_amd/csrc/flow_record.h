// flow_record.h -- what the flow consumers and the geometry kernels share about a flow record and the small rules around it, each
// written once: the record's two floats as one 8-byte access or two 4-byte ones and the host rule that picks between
// them, the known-flow rule of flow_io.flow_valid, the sentinel, `finite`, and the conversions to a byte.  They are parts of bit-level contracts (tests/*_ref.py restate them in numpy).
// The pragma below holds for everything AFTER this header in a translation unit too: a file whose arithmetic is contracted says so
// again behind its includes.
#pragma once
#include <initializer_list>

#include "pwc_common.h"

#pragma clang fp contract(off)

// What an output holds where there is no value (the .flo sentinel).
#define PWC_FLOW_SENTINEL 1e10f

// A record's two floats.  VEC: one 8-byte access -- the values, and so every bit, are the same.
template <bool VEC>
__device__ __forceinline__ void pwc_flow_load2(const float* p, float& a, float& b) {
    if (VEC) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(p);
        a = v[0]; b = v[1];
    } else {
        a = p[0]; b = p[1];
    }
}
template <bool VEC>
__device__ __forceinline__ void pwc_flow_store2(float* p, float a, float b) {
    if (VEC) {
        *reinterpret_cast<f32x2*>(p) = f32x2{a, b};
    } else {
        p[0] = a; p[1] = b;
    }
}

// The .flo sentinel rule (flow_io.flow_valid): false for a NaN, an Inf, the sentinel.
__device__ __forceinline__ bool pwc_flow_known(float a, float b) { return fabsf(a) <= 1e9f && fabsf(b) <= 1e9f; }

__host__ __device__ __forceinline__ bool pwc_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (false for a NaN)
__device__ __forceinline__ bool pwc_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

// A rounded double as a byte: clamped to [0, 255]; 0 for a NaN.
__device__ __forceinline__ unsigned pwc_clamp_byte(double t) { return t >= 255.0 ? 255u : (t >= 0.0 ? (unsigned)(int)t : 0u); }
// A double as a byte: rint, ties to even, then the clamp.
__device__ __forceinline__ unsigned pwc_round_byte(double v) { return pwc_clamp_byte(rint(v)); }

// ---------------------------------------------------------------- host
// VEC of a call: every channel stride even (cs: the strides or-ed together) and every float pointer on an 8-byte boundary (a null
// pointer, an operand the call does not have, counts as aligned).
static inline bool pwc_flow_vec(int cs, std::initializer_list<const void*> ptrs) {
    bool vec = !(cs & 1);
    for (const void* p : ptrs) vec = vec && !pwc_off(p, 7u);
    return vec;
}
