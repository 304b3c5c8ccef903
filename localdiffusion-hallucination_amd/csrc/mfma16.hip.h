// What the two attention cores on the 16-bit matrix cores (linattn16.hip, attention16.hip) share: v_mfma_f32_32x32x16_bf16
// or _f16 (mfma16<T>: the operand format T is bf16 or f16, the same 16 bytes per lane read as either) with its accumulator,
// and the swizzled [channel][64 rows] 16-bit image in LDS that feeds it.  The two forms share the lane map and the rate.
//
// Lane map of the MFMA, lane l with r = l & 31, hh = l >> 5: the lane holds A[r][8 hh + j] and B[8 hh + j][r], j = 0..7,
// and D[(reg & 3) + 8 (reg >> 2) + 4 hh][r] in its 16 accumulator registers.
#pragma once
#include "common.hip.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

// (a fragment travels as bf16x8 whatever T is: eight 16-bit operands rounded by pack2<T>)
template <typename T> __device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 acc);
template <> __device__ __forceinline__ f32x16 mfma16<bf16>(bf16x8 a, bf16x8 b, f32x16 acc) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x16 mfma16<f16>(bf16x8 a, bf16x8 b, f32x16 acc) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
}
// ... on operands that are four dwords of packed pairs (pack2<T>, a ds_read_b128)
template <typename T> __device__ __forceinline__ f32x16 mfma16(uint4 a, uint4 b, f32x16 acc) {
  return mfma16<T>(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc);
}
__device__ __forceinline__ f32x16 mfma16_zero() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.0f;
  return z;
}
// byte offset of the 16-byte group grp (rows 8 grp .. 8 grp + 7) of channel c in an image: 128-byte rows, the 16-byte
// groups swizzled by the row
__device__ __forceinline__ int mfma16_off(int c, int grp) { return c * 128 + 16 * (grp ^ (((c >> 2) ^ ((c >> 1) & 1)) & 7)); }
}  // namespace
