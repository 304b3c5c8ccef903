// What the exact-f32 nearest-neighbour search (patchcore.hip) and the fp16 screen in front of it (knn16.hip) share: the
// 64-bit (distance, index) key that both merge with an integer atomicMin, and the exact search of a listed subset.
#pragma once
#include "common.hip.h"

namespace {
__device__ __forceinline__ unsigned long long pc_key(float d2, unsigned idx) {
  return ((unsigned long long)(__float_as_uint(d2) & 0x7fffffffu) << 32) | idx;   // (d2 >= 0: drops a -0's sign)
}
__device__ __forceinline__ unsigned long long pc_shfl_xor64(unsigned long long v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
  return ((unsigned long long)hi << 32) | lo;
}
}  // namespace

// pc_knn_kernel's MODE 0 search for the *count (a device word, at most N) queries whose row numbers are list[0 ..
// *count): atomicMin of their keys into keys[row] (~0 on entry).  The grid is sized for N, so no host read of the count.
void pc_knn_exact_listed(const float* q, const float* qn, int N, const float* bank, const float* bn, long M, int D,
                         unsigned long long* keys, const int32_t* list, const int32_t* count, hipStream_t st);
