// "bf16x3": the exact three-way split of fp32 operands into bf16 terms, and the bf16 matrix instructions that multiply them.  The one
// definition of this arithmetic for every bf16x3 kernel (gemm.hip, conv_x3.hip, head_x3.hip, head_labels_x3.hip, stem_x3.hip).
//
// The split.  x = p0 + p1 + p2 with p0 = x truncated to its upper 16 bits (a bf16: sign, exponent, 8 significand bits), p1 the same of the
// remainder r = x - p0, p2 = r - p1.  Both subtractions are exact (they only clear leading bits), and each term carries 8 of x's 24
// significand bits: nothing is lost.  A term's bf16 is the upper half of its fp32 word, so packing truncates nothing.  Then
//   a * b = a0 b0 + (a0 b1 + a1 b0) + (a0 b2 + a1 b1 + a2 b0) + terms below 2^-24 |a| |b|,
// six bf16 products in fp32 accumulation, and the kernels issue them smallest first.  v_mfma_f32_32x32x16_bf16 does K = 16 in 32 cycles
// where v_mfma_f32_32x32x2_f32 needs 8 x 64: the six of them are 2.67x the fp32-MFMA rate.  Against an fp64 contraction the result is as
// accurate as the fp32-MFMA kernels' (the dropped terms are below the rounding of the fp32 accumulation).  Non-finite inputs: +-inf splits
// into (inf, NaN, NaN), so the output is NaN where an fp32 kernel gives +-inf or NaN -- non-finite either way.
//
// Why the products truncate.  The bf16 matrix instructions align every product to the largest addend (normally the accumulator) and
// TRUNCATE what falls below its last bit (tools/probe_mfma_rounding.hip: 1 + 0.75 ulp -> 1 when the 0.75 ulp is a product of the same
// instruction).  Small products added to a large accumulator lose their low bits, with a bias; issuing them smallest first, or into an
// accumulator of their own (conv_x3.hip), keeps that loss below the fp32 rounding.
//
// The product order of a K-step, and every fragment and plane layout, belong to the kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace bf16x3 {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// x truncated to a bf16 (its upper 16 bits), as an fp32
__device__ __forceinline__ float hi16(float x) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & 0xffff0000u); }
// the bf16 (upper halves) of two floats in one word: low half <- x0, high half <- x1 (truncation)
__device__ __forceinline__ unsigned pack_hi(float x0, float x1) {
    return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, x1), __builtin_bit_cast(unsigned, x0), 0x07060302u);
}
// the bf16 bit pattern of a split term (for packers that write unsigned short)
__device__ __forceinline__ unsigned short bits(float p) { return (unsigned short)(__builtin_bit_cast(unsigned, p) >> 16); }

// x = p0 + p1 + p2 exactly, each p a bf16 (the upper half of an fp32)
__device__ __forceinline__ void split(float x, float& p0, float& p1, float& p2) {
    p0 = hi16(x);
    const float r = x - p0;
    p1 = hi16(r);
    p2 = r - p1;
}
// four consecutive k -> the three planes of 4 x bf16
__device__ __forceinline__ void split4(float f0, float f1, float f2, float f3, u32x2_t& p0, u32x2_t& p1, u32x2_t& p2) {
    const float r0 = f0 - hi16(f0), r1 = f1 - hi16(f1), r2 = f2 - hi16(f2), r3 = f3 - hi16(f3);
    const float q0 = r0 - hi16(r0), q1 = r1 - hi16(r1), q2 = r2 - hi16(r2), q3 = r3 - hi16(r3);
    p0 = u32x2_t{pack_hi(f0, f1), pack_hi(f2, f3)};
    p1 = u32x2_t{pack_hi(r0, r1), pack_hi(r2, r3)};
    p2 = u32x2_t{pack_hi(q0, q1), pack_hi(q2, q3)};
}
// eight consecutive k -> the three planes of 8 x bf16 (one 16-byte fragment each)
__device__ __forceinline__ void split8(const float (&f)[8], u32x4_t& p0, u32x4_t& p1, u32x4_t& p2) {
    float r[8], q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { r[i] = f[i] - hi16(f[i]); q[i] = r[i] - hi16(r[i]); }
    p0 = u32x4_t{pack_hi(f[0], f[1]), pack_hi(f[2], f[3]), pack_hi(f[4], f[5]), pack_hi(f[6], f[7])};
    p1 = u32x4_t{pack_hi(r[0], r[1]), pack_hi(r[2], r[3]), pack_hi(r[4], r[5]), pack_hi(r[6], r[7])};
    p2 = u32x4_t{pack_hi(q[0], q[1]), pack_hi(q[2], q[3]), pack_hi(q[4], q[5]), pack_hi(q[6], q[7])};
}

// c + a * b on the bf16 matrix instructions, by the accumulator's shape: 32 x 32 x 16 (f32x16) or 16 x 16 x 32 (f32x4)
__device__ __forceinline__ f32x16 mma(const u32x4_t& a, const u32x4_t& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma(const u32x4_t& a, const u32x4_t& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

}  // namespace bf16x3
