// What the kernels of the denoiser's backward pass share (denoiser_grad.hip, linattn_grad.hip): how a memory-bound pass
// over an NHWC fp32 activation with a pixel stride spreads over the chip -- a thread owns four consecutive channels (one
// 16-byte load / store per pixel) and a fixed set of pixels of its workgroup's run -- and the workgroup's fixed-order fp64
// sum of what its threads gathered.
#pragma once
#include "common.hip.h"

namespace {

constexpr int DN_BS = 256;          // threads per workgroup of the GroupNorm passes
constexpr int DN_LANES = 64;        // 16-byte channel lanes per workgroup (256 channels)
constexpr int DN_MAX_CHUNKS = 128;  // pixel runs per sample
constexpr int DN_MIN_RUN = 16;      // pixels per run at least

inline hipStream_t dn_st(void* s) { return reinterpret_cast<hipStream_t>(s); }

// pixels per run and number of runs for a pass with Q channel lanes per pixel
inline void dn_runs(int B, long HW, int Q, long& ppc, int& nchunk) {
  const int ncb = (Q + DN_LANES - 1) / DN_LANES;
  long want = 1024 / ((long)B * ncb);                 // about four workgroups per CU in all
  if (want < 1) want = 1;
  if (want > DN_MAX_CHUNKS) want = DN_MAX_CHUNKS;
  ppc = (HW + want - 1) / want;
  if (ppc < DN_MIN_RUN) ppc = DN_MIN_RUN;
  nchunk = (int)((HW + ppc - 1) / ppc);
}

// Where a thread works: lane q of the Q 16-byte channel lanes of a pixel (channels 4q..4q+3), row r of the R rows of
// pixels its workgroup walks through its run [p0, p1).
struct DnPos {
  int q, ql, r, Qb, R;
  long p0, p1;
  bool active;
};
__device__ __forceinline__ DnPos dn_pos(int Q, long HW, long ppc) {
  DnPos t;
  const int rest = Q - (int)blockIdx.y * DN_LANES;
  t.Qb = rest < DN_LANES ? rest : DN_LANES;
  t.R = DN_BS / t.Qb;
  t.r = (int)threadIdx.x / t.Qb;
  t.ql = (int)threadIdx.x - t.r * t.Qb;
  t.q = (int)blockIdx.y * DN_LANES + t.ql;
  t.active = t.r < t.R;
  t.p0 = (long)blockIdx.x * ppc;
  t.p1 = t.p0 + ppc < HW ? t.p0 + ppc : HW;
  return t;
}

// The NV sums of every thread of the workgroup, added over the rows of pixels in a fixed order; threads 0..Qb-1 end with
// the totals of their lane.  Lanes of a wave that hold the same channels (Qb a power of two below 64: 64 / Qb rows per
// wave) meet by shuffles first, then one trip through LDS.
template <int NV>
__device__ __forceinline__ bool dn_block_sum(const DnPos& t, double (&v)[NV], double* red) {
  const bool pow2 = t.Qb < 64 && (t.Qb & (t.Qb - 1)) == 0;
  int rows = t.R, row = t.r;
  bool writer = t.active;
  if (pow2) {                                             // (uniform; 256 % Qb == 0: every lane is active)
    for (int off = 32; off >= t.Qb; off >>= 1) {
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] += __shfl_xor(v[i], off);
    }
    rows = DN_BS / 64;
    row = (int)threadIdx.x >> 6;
    writer = ((int)threadIdx.x & 63) < t.Qb;
  }
  if (writer) {
#pragma unroll
    for (int i = 0; i < NV; ++i) red[((size_t)row * t.Qb + t.ql) * NV + i] = v[i];
  }
  __syncthreads();
  const bool owner = (int)threadIdx.x < t.Qb;
  if (owner) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = red[(size_t)t.ql * NV + i];
    for (int r = 1; r < rows; ++r) {
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] += red[((size_t)r * t.Qb + t.ql) * NV + i];
    }
  }
  return owner;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float a, float b, float c, float d) {
  store16_out(p, make_uint4(__float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(d)));
}

inline bool dn_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace
