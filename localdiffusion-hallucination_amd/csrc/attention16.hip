// Full Attention's core on the bf16 matrix cores (Attention.full_attn_precision = "bf16" of attention_grad.py): the three
// passes of attention_grad.hip with every product on v_mfma_f32_32x32x16_bf16, two K-steps per 32-channel contraction.
// Both operands of a product are rounded to bf16 (round-to-nearest-even, NaN kept: pack_bf16x2), the products are exact
// in fp32 and are summed in the MFMA's fp32 accumulator.  The logits' scale, the online softmax (exp2(log2(e) x), the
// running maximum from the finite -1e30, masked keys' p selected to 0), the normaliser (the unrounded p), alpha, delta,
// ds = p (dP - delta) and the trailing 32^-0.5 are fp32, the formulas of attention_grad.hip.  Tensors, layouts, padding
// rules and `work` (delta [B, heads, n]) are the fp32 path's.  Nothing of size n x n is written, every sum has one fixed
// order, no floating-point atomics, nothing allocates.
// Every kernel is a template on the operand format T: <bf16> is the above (the ...16 entry points), <f16> the same code with
// pack2<f16> (v_cvt_pk_f16_f32: round-to-nearest-even, no saturation, beyond 65504 is inf) and v_mfma_f32_32x32x16_f16 (the
// ..._f16 entry points; amp_attn = "fp16"): the same operands rounded, everything else unchanged.
//
// The MFMA, its lane map (lane l: r = l & 31, hh = l >> 5) and the swizzle of the cols image are mfma16.hip.h's.  Every pass issues its products transposed, the tile's rows on M and the wave's own 32 rows on N, so that a lane owns one
// row of its side (a query in the forward and the row pass, a key in the column pass) and that row's q / dO (k / v) is a
// B operand held in registers for the whole launch:
//   S^T = K Q^T (keys on M):   the row maximum and the row sum are 16 in-lane values and those of lane l ^ 32;
//   O^T = V^T P^T:             the K index of this second product is permuted, K-step s element j <-> tile row
//                              8 (2 s + (j >> 2)) + 4 hh + (j & 3), so the 16 probabilities a lane holds in its
//                              accumulators are the 16 it feeds as B.  P and ds never go through LDS.
// The tile side comes from LDS as bf16, rounded once on its way in, in two images:
//   rows [64][32 channels], 80-byte rows: the A operand of a contraction over channels (K, V, Q, dO) is one ds_read_b128
//        per K-step, and 16 consecutive rows fall on 64 different banks (20 r mod 64 dwords);
//   cols [32 channels][64 rows], 128-byte rows with the XOR swizzle of the 16-byte groups (mfma16_off), the rows of a tile
//        stored in the permuted order above: the A operand of a contraction over the tile's rows (V^T, K^T, Q^T, dO^T)
//        is one ds_read_b128 per K-step as well.  A loader thread takes four channels of two neighbouring rows that are
//        neighbours in the permuted order too, and stores each channel's pair as one dword.
// Workgroup = 64 rows x four waves: wave (a, b) owns rows 32 a .. 32 a + 31 and takes rows 32 b .. 32 b + 31 of every
// 64-row tile; the two waves of a row meet at the end in wave order (the forward rescaled to the common maximum), in an
// fp32 tile in LDS from which the result leaves as 128 contiguous bytes per (row, head).  No store reads an accumulator.
#include "common.hip.h"
#include "dn_common.hip.h"
#include "fa_common.hip.h"
#include "mfma16.hip.h"

namespace {

constexpr int F16_RS = 80;             // bytes per row of a rows image
constexpr int F16_ROWS = FA_T * F16_RS;                // bytes of a rows image
constexpr int F16_COLS = FA_D * FA_T * 2;              // bytes of a cols image
constexpr int F16_TS = 36;             // floats per row of the fp32 exchange tile (linattn16's L16_TS)

// tile row of accumulator register i (and of element i & 7 of K-step i >> 3 of the second product)
__device__ __forceinline__ int f16_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// A loader thread's share of a 64-row tile: channels 4 l .. 4 l + 3 (l = tid & 7) of the rows at positions 2 rr, 2 rr + 1
// (rr = tid >> 3) of the permuted order, which are the neighbouring rows f16_ldrow, f16_ldrow + 1.
struct F16Raw {
  float4 x[2];
};
__device__ __forceinline__ int f16_ldrow(int tid) {
  const int p = 2 * (tid >> 3);                           // position: 32 half + 16 s + 8 hh + 4 g + i
  return (p & 32) + (p & 16) + 8 * ((p >> 2) & 1) + 4 * ((p >> 3) & 1) + (p & 3);
}
// rows r0 + .. of a [n][ld] matrix; zeros past n
__device__ __forceinline__ F16Raw f16_fetch(const float* __restrict__ src, long r0, long n, int ld, int tid) {
  F16Raw v;
  const int row = f16_ldrow(tid);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    v.x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + row + j < n) v.x[j] = ld4(src + (size_t)(r0 + row + j) * ld + 4 * (tid & 7));
  }
  return v;
}
template <typename T> __device__ __forceinline__ void f16_put_rows(unsigned char* img, const F16Raw& v, int tid) {
  const int row = f16_ldrow(tid);
#pragma unroll
  for (int j = 0; j < 2; ++j)
    *reinterpret_cast<uint2*>(img + (row + j) * F16_RS + 8 * (tid & 7)) =
        make_uint2(pack2<T>(v.x[j].x, v.x[j].y), pack2<T>(v.x[j].z, v.x[j].w));
}
template <typename T> __device__ __forceinline__ void f16_put_cols(unsigned char* img, const F16Raw& v, int tid) {
  const int rr = tid >> 3, c = 4 * (tid & 7);
  const int at = 4 * (rr & 3);
  *reinterpret_cast<unsigned*>(img + mfma16_off(c, rr >> 2) + at) = pack2<T>(v.x[0].x, v.x[1].x);
  *reinterpret_cast<unsigned*>(img + mfma16_off(c + 1, rr >> 2) + at) = pack2<T>(v.x[0].y, v.x[1].y);
  *reinterpret_cast<unsigned*>(img + mfma16_off(c + 2, rr >> 2) + at) = pack2<T>(v.x[0].z, v.x[1].z);
  *reinterpret_cast<unsigned*>(img + mfma16_off(c + 3, rr >> 2) + at) = pack2<T>(v.x[0].w, v.x[1].w);
}
// A operand of K-step s over channels: row `row` of a rows image, channels 16 s + 8 hh .. + 7
__device__ __forceinline__ uint4 f16_a_rows(const unsigned char* img, int row, int hh, int s) {
  return *reinterpret_cast<const uint4*>(img + row * F16_RS + 32 * s + 16 * hh);
}
// A operand of K-step s over the rows of half `half` of the tile: channel r of a cols image
__device__ __forceinline__ uint4 f16_a_cols(const unsigned char* img, int r, int hh, int half, int s) {
  return *reinterpret_cast<const uint4*>(img + mfma16_off(r, 4 * half + 2 * s + hh));
}
// The lane's B operands of a contraction over channels from its own row in memory: channels 16 s + 8 hh .. + 7; x keeps
// the 16 unrounded values.
template <typename T> __device__ __forceinline__ void f16_b_row(const float* __restrict__ src, int hh, uint4 (&b)[2], float (&x)[16]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const float4 u = ld4(src + 16 * s + 8 * hh), w = ld4(src + 16 * s + 8 * hh + 4);
    x[8 * s] = u.x; x[8 * s + 1] = u.y; x[8 * s + 2] = u.z; x[8 * s + 3] = u.w;
    x[8 * s + 4] = w.x; x[8 * s + 5] = w.y; x[8 * s + 6] = w.z; x[8 * s + 7] = w.w;
    b[s] = make_uint4(pack2<T>(u.x, u.y), pack2<T>(u.z, u.w), pack2<T>(w.x, w.y), pack2<T>(w.z, w.w));
  }
}
// B operand of K-step s of the second product from 16 values in accumulator order
template <typename T> __device__ __forceinline__ uint4 f16_b_acc(const float (&p)[16], int s) {
  return make_uint4(pack2<T>(p[8 * s], p[8 * s + 1]), pack2<T>(p[8 * s + 2], p[8 * s + 3]),
                    pack2<T>(p[8 * s + 4], p[8 * s + 5]), pack2<T>(p[8 * s + 6], p[8 * s + 7]));
}
// The exchange tile [64 rows][F16_TS] fp32: a lane's 16 channels 8 g + 4 hh + i of row `row`, accumulator order
__device__ __forceinline__ void f16_give(float* tile, int row, int hh, const float (&x)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
    *reinterpret_cast<float4*>(tile + row * F16_TS + 8 * g + 4 * hh) = make_float4(x[4 * g], x[4 * g + 1], x[4 * g + 2], x[4 * g + 3]);
}
__device__ __forceinline__ void f16_take(const float* tile, int row, int hh, float (&x)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 q = *reinterpret_cast<const float4*>(tile + row * F16_TS + 8 * g + 4 * hh);
    x[4 * g] = q.x; x[4 * g + 1] = q.y; x[4 * g + 2] = q.z; x[4 * g + 3] = q.w;
  }
}
// the tile to memory, 128 contiguous bytes per (row, head); rows past n store nothing
__device__ __forceinline__ void f16_flush(const float* tile, float* __restrict__ dst, long r0, long n, int ld, int tid) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = 32 * j + (tid >> 3);
    const float4 y = *reinterpret_cast<const float4*>(tile + row * F16_TS + 4 * (tid & 7));
    if (r0 + row < n) st4(dst + (size_t)(r0 + row) * ld + 4 * (tid & 7), y.x, y.y, y.z, y.w);
  }
}

// ================================================================================================ forward
template <typename T>
__global__ __launch_bounds__(FA_BS) void fa16_forward_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                              float* __restrict__ lse, long n, int heads, int ld3, int ldo) {
  __shared__ __attribute__((aligned(16))) unsigned char s_k[F16_ROWS];      // K  [key][channel]
  __shared__ __attribute__((aligned(16))) unsigned char s_vt[F16_COLS];     // V^T [channel][key]
  __shared__ __attribute__((aligned(16))) float s_o[FA_T * F16_TS];
  __shared__ float s_m[FA_T], s_l[FA_T];
  const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, hidden = heads * FA_D;
  const int r = lane & 31, hh = lane >> 5, qh = wv & 1, kh = wv >> 1, row = 32 * qh + r;
  const long q0 = (long)blockIdx.x * FA_T;
  float* orow = out + (size_t)b * n * ldo;
  if (h >= heads) {
    fa_zero_cols(orow, q0, n, ldo, h * FA_D, tid);
    return;
  }
  const float* base = qkv + (size_t)b * n * ld3 + h * FA_D;
  const long qi = q0 + row < n ? q0 + row : n - 1;
  uint4 qb[2];
  {
    float x[16];
    f16_b_row<T>(base + (size_t)qi * ld3, hh, qb, x);
  }
  f32x16 o = mfma16_zero();
  float m = FA_NEG, l = 0.f;
  F16Raw rk = f16_fetch(base + hidden, 0, n, ld3, tid), rv = f16_fetch(base + 2 * hidden, 0, n, ld3, tid);
  for (long j0 = 0; j0 < n; j0 += FA_T) {                   // (uniform: the barriers, the shuffles and the MFMAs)
    __syncthreads();
    f16_put_rows<T>(s_k, rk, tid);
    f16_put_cols<T>(s_vt, rv, tid);
    __syncthreads();
    if (j0 + FA_T < n) {                                    // the next tile's requests fly over the products
      rk = f16_fetch(base + hidden, j0 + FA_T, n, ld3, tid);
      rv = f16_fetch(base + 2 * hidden, j0 + FA_T, n, ld3, tid);
    }
    f32x16 sa = mfma16<T>(f16_a_rows(s_k, 32 * kh + r, hh, 0), qb[0], mfma16_zero());
    sa = mfma16<T>(f16_a_rows(s_k, 32 * kh + r, hh, 1), qb[1], sa);
    const long key0 = j0 + 32 * kh;
    float s[16], tmax = FA_NEG;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float a = sa[i] * FA_SCALE;
      s[i] = key0 + f16_row(i, hh) < n ? a : FA_NEG;
      tmax = fmaxf(tmax, s[i]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float mn = fmaxf(m, tmax);
    const float alpha = fa_exp(m - mn);                     // (both -1e30 while the wave has seen no valid key: 1, on l = o = 0)
    m = mn;
    float p[16], ps = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      p[i] = key0 + f16_row(i, hh) < n ? fa_exp(s[i] - m) : 0.f;
      ps += p[i];
    }
    ps += __shfl_xor(ps, 32);                               // (the same bits in both lanes of a query)
    l = l * alpha + ps;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] *= alpha;
    o = mfma16<T>(f16_a_cols(s_vt, r, hh, kh, 0), f16_b_acc<T>(p, 0), o);
    o = mfma16<T>(f16_a_cols(s_vt, r, hh, kh, 1), f16_b_acc<T>(p, 1), o);
  }
  // the two waves of a query meet, rescaled to the common maximum, in wave order
  float ov[16];
  if (kh == 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) ov[i] = o[i];
    f16_give(s_o, row, hh, ov);
    if (hh == 0) {
      s_m[row] = m;
      s_l[row] = l;
    }
  }
  __syncthreads();
  if (kh == 0) {
    const float m1 = s_m[row], l1 = s_l[row];
    const float M = fmaxf(m, m1);
    const float f0 = fa_exp(m - M), f1 = fa_exp(m1 - M);    // (a wave without a valid key: exp2(-huge) = 0, on l = o = 0)
    const float L = l * f0 + l1 * f1;
    const float inv = 1.0f / L;                             // (L >= 1: the wave that holds the maximum has f = 1 and l >= 1)
    float o1[16];
    f16_take(s_o, row, hh, o1);
#pragma unroll
    for (int i = 0; i < 16; ++i) ov[i] = (o[i] * f0 + o1[i] * f1) * inv;
    f16_give(s_o, row, hh, ov);
    if (lse && hh == 0 && q0 + row < n) lse[((size_t)b * heads + h) * n + q0 + row] = M + logf(L);
  }
  __syncthreads();
  f16_flush(s_o, orow + h * FA_D, q0, n, ldo, tid);
}

// ================================================================================================ backward: rows (dq)
template <typename T>
__global__ __launch_bounds__(FA_BS) void fa16_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                         const float* __restrict__ dout, const float* __restrict__ lse,
                                                         float* __restrict__ delta, float* __restrict__ dqkv, long n, int heads,
                                                         int ld3, int ldo) {
  __shared__ __attribute__((aligned(16))) unsigned char s_k[F16_ROWS];      // K  [key][channel]
  __shared__ __attribute__((aligned(16))) unsigned char s_v[F16_ROWS];      // V  [key][channel]
  __shared__ __attribute__((aligned(16))) unsigned char s_kt[F16_COLS];     // K^T [channel][key]
  __shared__ __attribute__((aligned(16))) float s_o[FA_T * F16_TS];
  const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, hidden = heads * FA_D;
  const int r = lane & 31, hh = lane >> 5, qh = wv & 1, kh = wv >> 1, row = 32 * qh + r;
  const long q0 = (long)blockIdx.x * FA_T;
  float* drow = dqkv + (size_t)b * n * ld3;
  if (h >= heads) {
    fa_zero_cols(drow, q0, n, ld3, 3 * hidden + (h - heads) * FA_D, tid);
    return;
  }
  const float* base = qkv + (size_t)b * n * ld3 + h * FA_D;
  const long qi = q0 + row < n ? q0 + row : n - 1;
  const size_t stat = ((size_t)b * heads + h) * n + qi;
  uint4 qb[2], gb[2];
  float dl;
  {
    float x[16], g[16], oo[16];
    uint4 unused[2];
    f16_b_row<T>(base + (size_t)qi * ld3, hh, qb, x);
    f16_b_row<T>(dout + ((size_t)b * n + qi) * ldo + h * FA_D, hh, gb, g);
    f16_b_row<T>(out + ((size_t)b * n + qi) * ldo + h * FA_D, hh, unused, oo);
    dl = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) dl = fmaf(g[i], oo[i], dl);
    dl += __shfl_xor(dl, 32);                               // (the same bits in both lanes of a query)
  }
  if (kh == 0 && hh == 0 && q0 + row < n) delta[stat] = dl;
  const float ls = lse[stat];
  f32x16 dq = mfma16_zero();
  F16Raw rk = f16_fetch(base + hidden, 0, n, ld3, tid), rv = f16_fetch(base + 2 * hidden, 0, n, ld3, tid);
  for (long j0 = 0; j0 < n; j0 += FA_T) {                   // (uniform: the barriers and the MFMAs)
    __syncthreads();
    f16_put_rows<T>(s_k, rk, tid);
    f16_put_cols<T>(s_kt, rk, tid);
    f16_put_rows<T>(s_v, rv, tid);
    __syncthreads();
    if (j0 + FA_T < n) {
      rk = f16_fetch(base + hidden, j0 + FA_T, n, ld3, tid);
      rv = f16_fetch(base + 2 * hidden, j0 + FA_T, n, ld3, tid);
    }
    f32x16 sa = mfma16<T>(f16_a_rows(s_k, 32 * kh + r, hh, 0), qb[0], mfma16_zero());
    sa = mfma16<T>(f16_a_rows(s_k, 32 * kh + r, hh, 1), qb[1], sa);
    f32x16 dp = mfma16<T>(f16_a_rows(s_v, 32 * kh + r, hh, 0), gb[0], mfma16_zero());
    dp = mfma16<T>(f16_a_rows(s_v, 32 * kh + r, hh, 1), gb[1], dp);
    const long key0 = j0 + 32 * kh;
    float ds[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float p = key0 + f16_row(i, hh) < n ? fa_exp(sa[i] * FA_SCALE - ls) : 0.f;
      ds[i] = p * (dp[i] - dl);
    }
    dq = mfma16<T>(f16_a_cols(s_kt, r, hh, kh, 0), f16_b_acc<T>(ds, 0), dq);
    dq = mfma16<T>(f16_a_cols(s_kt, r, hh, kh, 1), f16_b_acc<T>(ds, 1), dq);
  }
  float ov[16];
  if (kh == 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) ov[i] = dq[i];
    f16_give(s_o, row, hh, ov);
  }
  __syncthreads();
  if (kh == 0) {
    float o1[16];
    f16_take(s_o, row, hh, o1);
#pragma unroll
    for (int i = 0; i < 16; ++i) ov[i] = (dq[i] + o1[i]) * FA_SCALE;
    f16_give(s_o, row, hh, ov);
  }
  __syncthreads();
  f16_flush(s_o, drow + h * FA_D, q0, n, ld3, tid);
}

// ================================================================================================ backward: columns (dk, dv)
template <typename T>
__global__ __launch_bounds__(FA_BS) void fa16_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          float* __restrict__ dqkv, long n, int heads, int ld3, int ldo) {
  __shared__ __attribute__((aligned(16))) unsigned char s_q[F16_ROWS];      // Q   [query][channel]
  __shared__ __attribute__((aligned(16))) unsigned char s_g[F16_ROWS];      // dO  [query][channel]
  __shared__ __attribute__((aligned(16))) unsigned char s_qt[F16_COLS];     // Q^T  [channel][query]
  __shared__ __attribute__((aligned(16))) unsigned char s_gt[F16_COLS];     // dO^T [channel][query]
  __shared__ __attribute__((aligned(16))) float s_ls[FA_T], s_dl[FA_T];
  __shared__ __attribute__((aligned(16))) float s_o[2][FA_T * F16_TS];      // dk, dv
  const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, hidden = heads * FA_D;
  const int r = lane & 31, hh = lane >> 5, kh = wv & 1, qh = wv >> 1, row = 32 * kh + r;
  const long k0 = (long)blockIdx.x * FA_T;
  const float* base = qkv + (size_t)b * n * ld3 + h * FA_D;
  const float* gbase = dout + (size_t)b * n * ldo + h * FA_D;
  const size_t stat = ((size_t)b * heads + h) * n;
  const long ki = k0 + row < n ? k0 + row : n - 1;
  uint4 kb[2], vb[2];
  {
    float x[16];
    f16_b_row<T>(base + hidden + (size_t)ki * ld3, hh, kb, x);
    f16_b_row<T>(base + 2 * hidden + (size_t)ki * ld3, hh, vb, x);
  }
  f32x16 dk = mfma16_zero(), dv = mfma16_zero();
  F16Raw rq = f16_fetch(base, 0, n, ld3, tid), rg = f16_fetch(gbase, 0, n, ldo, tid);
  float rls = 0.f, rdl = 0.f;
  if (tid < FA_T && tid < n) {
    rls = lse[stat + tid];
    rdl = delta[stat + tid];
  }
  for (long i0 = 0; i0 < n; i0 += FA_T) {                   // (uniform: the barriers and the MFMAs)
    __syncthreads();
    f16_put_rows<T>(s_q, rq, tid);
    f16_put_cols<T>(s_qt, rq, tid);
    f16_put_rows<T>(s_g, rg, tid);
    f16_put_cols<T>(s_gt, rg, tid);
    if (tid < FA_T) {
      s_ls[tid] = rls;
      s_dl[tid] = rdl;
    }
    __syncthreads();
    if (i0 + FA_T < n) {
      rq = f16_fetch(base, i0 + FA_T, n, ld3, tid);
      rg = f16_fetch(gbase, i0 + FA_T, n, ldo, tid);
      if (tid < FA_T) {
        const bool ok = i0 + FA_T + tid < n;
        rls = ok ? lse[stat + i0 + FA_T + tid] : 0.f;
        rdl = ok ? delta[stat + i0 + FA_T + tid] : 0.f;
      }
    }
    f32x16 sa = mfma16<T>(f16_a_rows(s_q, 32 * qh + r, hh, 0), kb[0], mfma16_zero());
    sa = mfma16<T>(f16_a_rows(s_q, 32 * qh + r, hh, 1), kb[1], sa);
    f32x16 dp = mfma16<T>(f16_a_rows(s_g, 32 * qh + r, hh, 0), vb[0], mfma16_zero());
    dp = mfma16<T>(f16_a_rows(s_g, 32 * qh + r, hh, 1), vb[1], dp);
    const long qq0 = i0 + 32 * qh;
    float p[16], ds[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {                           // rows 8 g + 4 hh .. + 3 of the half (a broadcast read)
      const float4 l4 = *reinterpret_cast<const float4*>(s_ls + 32 * qh + 8 * g + 4 * hh);
      const float4 d4 = *reinterpret_cast<const float4*>(s_dl + 32 * qh + 8 * g + 4 * hh);
      const float lsv[4] = {l4.x, l4.y, l4.z, l4.w}, dlv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * g + j;
        p[i] = qq0 + f16_row(i, hh) < n ? fa_exp(sa[i] * FA_SCALE - lsv[j]) : 0.f;
        ds[i] = p[i] * (dp[i] - dlv[j]);
      }
    }
    dv = mfma16<T>(f16_a_cols(s_gt, r, hh, qh, 0), f16_b_acc<T>(p, 0), dv);
    dv = mfma16<T>(f16_a_cols(s_gt, r, hh, qh, 1), f16_b_acc<T>(p, 1), dv);
    dk = mfma16<T>(f16_a_cols(s_qt, r, hh, qh, 0), f16_b_acc<T>(ds, 0), dk);
    dk = mfma16<T>(f16_a_cols(s_qt, r, hh, qh, 1), f16_b_acc<T>(ds, 1), dk);
  }
  float xk[16], xv[16];
  if (qh == 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      xk[i] = dk[i];
      xv[i] = dv[i];
    }
    f16_give(s_o[0], row, hh, xk);
    f16_give(s_o[1], row, hh, xv);
  }
  __syncthreads();
  if (qh == 0) {
    float o1[16];
    f16_take(s_o[0], row, hh, o1);
#pragma unroll
    for (int i = 0; i < 16; ++i) xk[i] = (dk[i] + o1[i]) * FA_SCALE;
    f16_give(s_o[0], row, hh, xk);
    f16_take(s_o[1], row, hh, o1);
#pragma unroll
    for (int i = 0; i < 16; ++i) xv[i] = dv[i] + o1[i];
    f16_give(s_o[1], row, hh, xv);
  }
  __syncthreads();
  float* dst = dqkv + (size_t)b * n * ld3 + h * FA_D;
  f16_flush(s_o[0], dst + hidden, k0, n, ld3, tid);
  f16_flush(s_o[1], dst + 2 * hidden, k0, n, ld3, tid);
}

// ================================================================================================ host side
// One body per entry point for both formats; `fn` is the entry point's name in the messages.
template <typename T>
int fa16_forward(const char* fn, const float* qkv, float* out, float* lse, int B, int H, int W, int heads, int ld3, int ldo,
                 void* stream) {
  LD_REQUIRE(fa_shape_ok(B, H, W, heads) && fa_strides_ok(heads, ld3, ldo),
             "%s: B=%d H=%d W=%d heads=%d ld3=%d ldo=%d (heads >= 1, ld3 >= 96 heads, ldo >= 32 heads, multiples of 4)", fn, B, H, W,
             heads, ld3, ldo);
  LD_REQUIRE(qkv && out, "%s: null pointer", fn);
  LD_REQUIRE(dn_aligned16(qkv) && dn_aligned16(out) && (reinterpret_cast<uintptr_t>(lse) & 3) == 0,
             "%s: a pointer is not aligned (qkv, out: 16 bytes)", fn);
  const int slots = fa_slots(heads, ldo, heads * FA_D);
  LD_REQUIRE(slots <= 65535, "%s: ldo %d", fn, ldo);
  const long n = (long)H * W;
  LD_LAUNCH(fa16_forward_kernel<T>, dim3((unsigned)((n + FA_T - 1) / FA_T), (unsigned)slots, (unsigned)B), dim3(FA_BS), 0,
            dn_st(stream), qkv, out, lse, n, heads, ld3, ldo);
  LD_LAUNCH_CHECK(fn + 3);                                  // (without "ld_")
  return LD_OK;
}

template <typename T>
int fa16_backward(const char* fn, const float* qkv, const float* out, const float* dout, const float* lse, void* work, float* dqkv,
                  int B, int H, int W, int heads, int ld3, int ldo, void* stream) {
  LD_REQUIRE(fa_shape_ok(B, H, W, heads) && fa_strides_ok(heads, ld3, ldo),
             "%s: B=%d H=%d W=%d heads=%d ld3=%d ldo=%d (heads >= 1, ld3 >= 96 heads, ldo >= 32 heads, multiples of 4)", fn, B, H, W,
             heads, ld3, ldo);
  LD_REQUIRE(qkv && out && dout && lse && work && dqkv, "%s: null pointer", fn);
  LD_REQUIRE(dn_aligned16(qkv) && dn_aligned16(out) && dn_aligned16(dout) && dn_aligned16(dqkv) &&
                 (reinterpret_cast<uintptr_t>(lse) & 3) == 0 && (reinterpret_cast<uintptr_t>(work) & 3) == 0,
             "%s: a pointer is not aligned (qkv, out, dout, dqkv: 16 bytes)", fn);
  const int slots = fa_slots(heads, ld3, 3 * heads * FA_D);
  LD_REQUIRE(slots <= 65535, "%s: ld3 %d", fn, ld3);
  const long n = (long)H * W;
  const unsigned tiles = (unsigned)((n + FA_T - 1) / FA_T);
  hipStream_t st = dn_st(stream);
  float* delta = static_cast<float*>(work);                // [B, heads, n]: ld_dn_fa_work_bytes
  LD_LAUNCH(fa16_dq_kernel<T>, dim3(tiles, (unsigned)slots, (unsigned)B), dim3(FA_BS), 0, st, qkv, out, dout, lse, delta, dqkv, n,
            heads, ld3, ldo);
  LD_LAUNCH(fa16_dkv_kernel<T>, dim3(tiles, (unsigned)heads, (unsigned)B), dim3(FA_BS), 0, st, qkv, dout, lse, (const float*)delta,
            dqkv, n, heads, ld3, ldo);
  LD_LAUNCH_CHECK(fn + 3);
  return LD_OK;
}
}  // namespace

#define FA16_ENTRY(suffix, T)                                                                                                  \
  extern "C" int ld_dn_fa_forward##suffix(const float* qkv, float* out, float* lse, int B, int H, int W, int heads, int ld3,   \
                                          int ldo, void* stream) {                                                             \
    return fa16_forward<T>("ld_dn_fa_forward" #suffix, qkv, out, lse, B, H, W, heads, ld3, ldo, stream);                       \
  }                                                                                                                            \
  extern "C" int ld_dn_fa_backward##suffix(const float* qkv, const float* out, const float* dout, const float* lse, void* work, \
                                           float* dqkv, int B, int H, int W, int heads, int ld3, int ldo, void* stream) {       \
    return fa16_backward<T>("ld_dn_fa_backward" #suffix, qkv, out, dout, lse, work, dqkv, B, H, W, heads, ld3, ldo, stream);    \
  }
FA16_ENTRY(16, bf16)
FA16_ENTRY(_f16, f16)
