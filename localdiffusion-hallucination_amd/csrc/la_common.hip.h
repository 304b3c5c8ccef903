// What the fp32 attention-core kernels (linattn_grad.hip) and their bf16 siblings (linattn16.hip) share: the sizes, the
// split of the pixel axis into parts and runs, the 8-lane softmax, the two merge kernels over the fp64 parts in `work`
// and the shape checks.  Moved here unchanged, so both files launch the same merge code on the same part format.
#pragma once
#include "common.hip.h"
#include "dn_common.hip.h"

namespace {

constexpr int LA_D = 32;              // channels per head (the reference's only dim_head)
constexpr int LA_BS = 256;            // threads per workgroup
constexpr int LA_TP = 64;             // pixels per LDS tile of the reductions
constexpr int LA_PART = 64 + LA_D * LA_D;     // doubles per part in `work`: m [32], Z [32], ctx [32][32]
constexpr int LA_MAX_PARTS = 256;          // parts of the pixel axis per (sample, head) at most
constexpr double LA_SCALE = 0.17677669529663687;      // 32^-0.5

__device__ __forceinline__ float la_exp(float a) { return __builtin_amdgcn_exp2f(1.4426950408889634f * a); }

// ================================================================================================ attention: reductions
// pixels per part (a multiple of the tile) and number of parts: a function of the shape alone
inline void la_parts(int B, int heads, long HW, long& ppp, int& S) {
  long want = 1024 / ((long)B * heads);               // about four workgroups per CU in all
  if (want < 1) want = 1;
  if (want > LA_MAX_PARTS) want = LA_MAX_PARTS;
  ppp = (HW + want - 1) / want;
  ppp = (ppp + LA_TP - 1) / LA_TP * LA_TP;
  S = (int)((HW + ppp - 1) / ppp);
}
// pixels per workgroup (a multiple of 32) of an element-wise pass with `slots` workgroup columns per sample
inline void la_runs(int B, int slots, long HW, long& run, unsigned& nrun) {
  long want = 2048 / ((long)B * slots);
  if (want < 1) want = 1;
  run = (HW + want - 1) / want;
  run = (run + 31) / 32 * 32;
  nrun = (unsigned)((HW + run - 1) / run);
}

// softmax over the 32 channels that the 8 lanes of a (pixel, head) hold four each; every lane gets the same bits
__device__ __forceinline__ float4 la_softmax8(float4 q) {
  float mx = fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w));
  for (int off = 1; off <= 4; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  const float4 e = make_float4(la_exp(q.x - mx), la_exp(q.y - mx), la_exp(q.z - mx), la_exp(q.w - mx));
  float s = (e.x + e.y) + (e.z + e.w);
  for (int off = 1; off <= 4; off <<= 1) s += __shfl_xor(s, off);
  const float inv = 1.0f / s;
  return make_float4(e.x * inv, e.y * inv, e.z * inv, e.w * inv);
}

// ctx [b][head][d][e], kstat [b][head][d] = (m, Z): the parts in index order, each rescaled to the common maximum
__global__ __launch_bounds__(256) void la_context_merge_kernel(const double* __restrict__ work, float* __restrict__ ctx,
                                                               float* __restrict__ kstat, int S) {
  const size_t bh = blockIdx.x;
  const int d = (int)threadIdx.x >> 3, eg = (int)threadIdx.x & 7;
  const double* part = work + bh * S * LA_PART;
  double M = part[d];
  for (int k = 1; k < S; ++k) M = fmax(M, part[(size_t)k * LA_PART + d]);
  double Z = 0.0, c[4] = {0, 0, 0, 0};
  for (int k = 0; k < S; ++k) {
    const double* p = part + (size_t)k * LA_PART;
    const double w = exp(p[d] - M);
    Z += w * p[32 + d];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] += w * p[64 + d * LA_D + 4 * eg + j];
  }
  float* dst = ctx + (bh * LA_D + d) * LA_D + 4 * eg;
#pragma unroll
  for (int j = 0; j < 4; ++j) dst[j] = (float)(c[j] / Z);
  if (eg == 0) {
    kstat[(bh * LA_D + d) * 2] = (float)M;
    kstat[(bh * LA_D + d) * 2 + 1] = (float)Z;
  }
}

// dctx = 32^-0.5 x the parts in index order; rk [d] = sum_e dctx[d][e] ctx[d][e]
__global__ __launch_bounds__(256) void la_reduce_merge_kernel(const double* __restrict__ work, const float* __restrict__ ctx,
                                                              float* __restrict__ dctx, float* __restrict__ rk, int S) {
  const size_t bh = blockIdx.x;
  const int d = (int)threadIdx.x >> 3, eg = (int)threadIdx.x & 7;
  const double* part = work + bh * S * LA_PART + 64 + d * LA_D + 4 * eg;
  double c[4] = {0, 0, 0, 0};
  for (int k = 0; k < S; ++k) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] += part[(size_t)k * LA_PART + j];
  }
  const size_t at = (bh * LA_D + d) * LA_D + 4 * eg;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] *= LA_SCALE;
    dctx[at + j] = (float)c[j];
    s += c[j] * (double)ctx[at + j];
  }
  for (int off = 1; off <= 4; off <<= 1) s += __shfl_xor(s, off);
  if (eg == 0) rk[bh * LA_D + d] = (float)s;
}

inline bool la_shape_ok(int B, int H, int W, int heads) {
  return B > 0 && B <= 65535 && H > 0 && W > 0 && heads >= 1 && heads <= 16384;
}
inline bool la_strides_ok(int heads, int ld3, int ldo) {
  return ld3 >= 3 * heads * LA_D && ld3 % 4 == 0 && ldo >= heads * LA_D && ldo % 4 == 0;
}
}  // namespace
