// float -> bf16 hi + bf16 lo, the split the three-product bf16 convolutions multiply with (pcnet_kernels.h), in its two forms.  A header
// of its own so that tests/tools/bf16_split_check.hip can walk both over every bit pattern.
#pragma once

#include <hip/hip_runtime.h>

namespace ake_k {

// float -> bf16 bits, round to nearest even (finite inputs)
__device__ __forceinline__ unsigned int bf16_bits(float v) {
    const unsigned int u = __float_as_uint(v);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

typedef float f32x2c __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2c __attribute__((ext_vector_type(2)));
// two floats -> their bf16 hi and lo halves, packed (low 16 bits: a's).  v_cvt_pk_bf16_f32 rounds to nearest even: for every non-NaN
// input hi and lo are the bits of bf16_bits(v) and bf16_bits(v - hi) (tests/test_gpu_bf16_split.py walks all 2^32 patterns)
__device__ __forceinline__ void bf16_split2(float a, float b, unsigned int& hi, unsigned int& lo) {
    const f32x2c v = {a, b};
    const bf16x2c h = __builtin_convertvector(v, bf16x2c);
    const f32x2c r = v - __builtin_convertvector(h, f32x2c);
    hi = __builtin_bit_cast(unsigned int, h);
    lo = __builtin_bit_cast(unsigned int, __builtin_convertvector(r, bf16x2c));
}

}  // namespace ake_k
