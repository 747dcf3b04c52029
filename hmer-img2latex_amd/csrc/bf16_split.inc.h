// The 3 x bf16 split of the fp32-grade matrix-core kernels (conv_bf16x3.hip, gemm.hip, resnet.hip, resnet_train.hip,
// decode_group16.inc.h): x = x0 + x1 + x2 with x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1) -- 3 x 8 = 24
// mantissa bits, every difference exact in fp32.  A product evaluated as the six partial products a_i b_j, i + j <= 2,
// drops terms of at most 2^-24 |a||b| only if every split rounds to nearest even in the same
// way: f2bf and v_cvt_pk_bf16_f32 (split3_pair) both do, which is why this file is the only copy.
// Included inside each translation unit's anonymous namespace.
#pragma once

typedef unsigned short bf16_t;                                // one bf16 as its bit pattern
typedef short i16x8_t __attribute__((ext_vector_type(8)));    // 8 bf16 bit patterns: the *_bf16_1k-style operand
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));  // 8 bf16 values: the v_mfma_f32_16x16x32_bf16 operand

__device__ __forceinline__ bf16_t f2bf(float f) {
    unsigned u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);          // round to nearest even (finite inputs)
    return (bf16_t)(u >> 16);
}
__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ void split3(float x, bf16_t& s0, bf16_t& s1, bf16_t& s2) {
    s0 = f2bf(x);
    const float r1 = x - bf2f(s0);
    s1 = f2bf(r1);
    s2 = f2bf(r1 - bf2f(s1));
}

// two values at once: v_cvt_pk_bf16_f32 (round to nearest even, as f2bf) packs the pair into one dword
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned& s0, unsigned& s1, unsigned& s2) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    f32x2_t v = {x0, x1};
    bf16x2_t b0 = __builtin_convertvector(v, bf16x2_t);
    v -= __builtin_convertvector(b0, f32x2_t);
    bf16x2_t b1 = __builtin_convertvector(v, bf16x2_t);
    v -= __builtin_convertvector(b1, f32x2_t);
    bf16x2_t b2 = __builtin_convertvector(v, bf16x2_t);
    s0 = *reinterpret_cast<unsigned*>(&b0);
    s1 = *reinterpret_cast<unsigned*>(&b1);
    s2 = *reinterpret_cast<unsigned*>(&b2);
}
