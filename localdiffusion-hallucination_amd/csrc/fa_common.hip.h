// What the fp32 kernels of full Attention's core (attention_grad.hip) and their bf16 siblings (attention16.hip) share: the
// sizes, the softmax's constants and exp, the workgroup columns that zero an output's padding, and the shape checks.
// Moved here unchanged, so both files check and launch over the same grid.
#pragma once
#include "common.hip.h"
#include "dn_common.hip.h"

namespace {

constexpr int FA_D = 32;              // channels per head (the reference's only dim_head)
constexpr int FA_BS = 256;            // threads per workgroup: four waves
constexpr int FA_T = 64;              // rows per workgroup and rows per LDS tile
constexpr float FA_SCALE = 0.17677669529663687f;      // 32^-0.5
constexpr float FA_NEG = -1e30f;      // the running maximum before the first valid key (finite on purpose)
constexpr long FA_MAX_N = 1L << 30;   // pixels at most

__device__ __forceinline__ float fa_exp(float a) { return __builtin_amdgcn_exp2f(1.4426950408889634f * a); }

// dst [row][c0 .. c0 + 32) = 0 for the rows of this workgroup's tile (the padding columns of an output)
__device__ __forceinline__ void fa_zero_cols(float* __restrict__ dst, long r0, long n, int ld, int c0, int tid) {
  const int c = c0 + 4 * (tid & 7);
  if (c >= ld) return;
  for (int r = tid >> 3; r < FA_T; r += FA_BS / 8)
    if (r0 + r < n) st4(dst + (size_t)(r0 + r) * ld + c, 0.f, 0.f, 0.f, 0.f);
}

inline bool fa_shape_ok(int B, int H, int W, int heads) {
  return B > 0 && B <= 65535 && H > 0 && W > 0 && (long)H * W <= FA_MAX_N && heads >= 1 && heads <= 16384;
}
inline bool fa_strides_ok(int heads, int ld3, int ldo) {
  return ld3 >= 3 * heads * FA_D && ld3 % 4 == 0 && ldo >= heads * FA_D && ldo % 4 == 0;
}
// workgroup columns: one per head and one per 32 channels of padding behind `used`
inline int fa_slots(int heads, int ld, int used) { return heads + (ld - used + FA_D - 1) / FA_D; }
}  // namespace
