// The vector types of the matrix-core kernels and the three-term bf16 operand form ("bf16x6": x = hi + mid + lo, six products).
// Device code only; everything lives in the including file's anonymous namespace.
#pragma once
#include "common.h"

namespace {

using f32x2_t = __attribute__((ext_vector_type(2))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;      // the 32x32 MFMA accumulator
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using bf16x8 = __attribute__((ext_vector_type(8))) short;       // the bf16 MFMA operand (bit patterns)
using bf16x2_t = __attribute__((ext_vector_type(2))) __bf16;

__device__ __forceinline__ unsigned bf16_rne(float x) {       // finite inputs
    unsigned u = __float_as_uint(x);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float bf16_up(unsigned b) { return __uint_as_float(b << 16); }

// x -> (hi, mid, lo) bf16 bit patterns with hi + mid + lo == x up to 2^-25 |x|
__device__ __forceinline__ void split3(float x, unsigned& h, unsigned& m, unsigned& l) {
    h = bf16_rne(x);
    const float r1 = x - bf16_up(h);
    m = bf16_rne(r1);
    const float r2 = r1 - bf16_up(m);
    l = bf16_rne(r2);
}

// the same split for two values at once on gfx950's packed converter: v_cvt_pk_bf16_f32 (RNE) gives
// lo16 = bf16(x0), hi16 = bf16(x1) -- exactly the LDS slot layout -- and the residuals are one v_pk_add_f32
__device__ __forceinline__ unsigned cvt_pk_bf16(float x0, float x1) {
    const f32x2_t v = {x0, x1};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ void split3_pk(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    h = cvt_pk_bf16(x0, x1);
    const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);
    m = cvt_pk_bf16(r0, r1);
    const float s0 = r0 - __uint_as_float(m << 16), s1 = r1 - __uint_as_float(m & 0xffff0000u);
    l = cvt_pk_bf16(s0, s1);
}

}  // namespace
