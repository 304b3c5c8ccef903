// LinearAttention's core on the bf16 matrix cores (attn_precision = "bf16" of linattn_grad.py): the four passes of
// linattn_grad.hip with every 32 x 32 product of a head on v_mfma_f32_32x32x16_bf16.  Both operands of a product are
// rounded to bf16 (round-to-nearest-even, NaN kept: pack_bf16x2, as conv16.hip rounds), the products are exact in fp32 and
// are summed in the MFMA's fp32 accumulator; nothing else is rounded.  Tensors, layouts, the parts of the pixel axis, the
// fp64 part format in `work` and the two merge kernels are the fp32 path's (la_common.hip.h).  No floating-point atomics,
// every sum in one order, nothing allocates.
//
// Every kernel is a template on the operand format T: <bf16> is the above (the ...16 entry points), <f16> the same code with
// pack2<f16> (v_cvt_pk_f16_f32: round-to-nearest-even, no saturation, beyond 65504 is inf) and v_mfma_f32_32x32x16_f16 (the
// ..._f16 entry points; amp_attn = "fp16").  Images, swizzle, tiles, barriers, the order of every addition and the fp32
// formulas are the same; the one difference is the dv product of la16_apply_kernel, described there.
//
// The MFMA and its lane map (lane l: r = l & 31, hh = l >> 5) are mfma16.hip.h's.
//
//   * The two reductions over pixels (context; dctx of the backward): D[d][e] = sum_n P[n][d] V[n][e], K is the pixel axis.
//     The loader is the fp32 kernel's (8 lanes per (pixel, head), 16-byte loads, the same 8-lane softmax), a thread taking
//     the same four channels of two neighbouring pixels.  It stores the pair of each channel as one dword into an image
//     [channel][64 pixels] bf16 with 128-byte rows whose 16-byte groups are XOR-swizzled by the row (mfma16_off): the stores
//     of a half-wave fall on 32 different banks, and a lane's fragment (8 consecutive pixels of channel r) is one
//     ds_read_b128 whose four 16-lane groups each cover all 64 banks.  A tile is 64 pixels = four K-steps, one per wave;
//     two images alternate, so a tile costs one barrier.  A wave's fp32 accumulator holds at most L16_RUN tiles (16 x 16 =
//     256 pixels) before it is added into fp64 registers; the four waves' fp64 sums meet in wave order at the end of the
//     part.  Z sums the unrounded P: fp32 in a loader thread over a run (32 pixels), fp64 across runs and threads.
//   * The two element-wise passes (output; dqkv of the backward) issue the products transposed, channels on M and the 32
//     pixels of a wave's tile on N, so the constant matrices (ctx, dctx, their transposes) are A operands held in
//     registers for the whole workgroup and a lane owns one pixel.  The K index is permuted, k-step s element j <->
//     channel 8 (2 s + (j >> 2)) + 4 hh + (j & 3), so that the 16 channels a lane feeds as B are the 16 its accumulators
//     hold: one copy of q / k / v / dO serves the softmax, ks, the products and the epilogue, and the softmax and `dot`
//     over a head's 32 channels are 16 values here and 16 in lane l ^ 32.  Memory is read and written as the fp32
//     kernels do it (8 lanes x 16 bytes = the 128 contiguous bytes of a (pixel, head)); a wave-private fp32 tile in LDS
//     turns that into the lane-per-pixel view and back (l16_put / l16_take / l16_give / l16_flush), so no workgroup
//     barrier stands in the loop and no store reads an accumulator register directly.
#include "common.hip.h"
#include "dn_common.hip.h"
#include "la_common.hip.h"
#include "mfma16.hip.h"

namespace {

constexpr int L16_RUN = 16;        // tiles of 64 pixels per fp32 run of the reductions
constexpr int L16_IMG = LA_D * LA_TP * 2;      // bytes of one [32 channels][64 pixels] bf16 image

__device__ __forceinline__ bf16x8 l16_frag(unsigned a, unsigned b, unsigned c, unsigned d) {
  return __builtin_bit_cast(bf16x8, make_uint4(a, b, c, d));
}

// ================================================================================================ reductions
// part (b, head, s) of pixels [s ppp, (s + 1) ppp).  CTX: (m, Z, ctx Z) with P = exp(k - m_part), V = v; otherwise
// sum of softmax_d(q)[d] dO[e].
template <typename T, bool CTX>
__global__ __launch_bounds__(LA_BS) void la16_reduce_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                            double* __restrict__ work, long HW, int heads, int ld3, int ldo,
                                                            long ppp, int S) {
  __shared__ __attribute__((aligned(16))) unsigned char sT[2][2][L16_IMG];     // [buffer][P, V]
  __shared__ __attribute__((aligned(16))) float sm[LA_D];
  __shared__ double comb[3 * 16 * 64];
  const int t = threadIdx.x, h = blockIdx.y, b = blockIdx.z, hidden = heads * LA_D;
  const long p0 = (long)blockIdx.x * ppp, p1 = p0 + ppp < HW ? p0 + ppp : HW;
  const float* PA = qkv + (size_t)b * HW * ld3 + (CTX ? hidden : 0) + h * LA_D;                  // k, or q
  const float* PB = CTX ? PA + hidden : dout + (size_t)b * HW * ldo + h * LA_D;                  // v, or dO
  const int ldb = CTX ? ld3 : ldo;
  const int rr = t >> 3, l = t & 7;                        // loader: pixels 2 rr, 2 rr + 1 of a tile, channels 4 l .. 4 l + 3
  const int wave = t >> 6, lane = t & 63, r = lane & 31, hh = lane >> 5;
  float4 mk = make_float4(0.f, 0.f, 0.f, 0.f);
  if (CTX) {                                              // the part's maximum of every k channel (sT as scratch)
    float* scr = reinterpret_cast<float*>(&sT[0][0][0]);
    float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (long n = p0 + rr; n < p1; n += 32) {
      const float4 k = ld4(PA + (size_t)n * ld3 + 4 * l);
      mx.x = fmaxf(mx.x, k.x); mx.y = fmaxf(mx.y, k.y); mx.z = fmaxf(mx.z, k.z); mx.w = fmaxf(mx.w, k.w);
    }
    *reinterpret_cast<float4*>(scr + rr * LA_D + 4 * l) = mx;
    __syncthreads();
    if (t < LA_D) {
      float m = scr[t];
      for (int i = 1; i < 32; ++i) m = fmaxf(m, scr[i * LA_D + t]);
      sm[t] = m;                                          // (finite: a part holds at least one pixel)
    }
    __syncthreads();
    mk = *reinterpret_cast<const float4*>(sm + 4 * l);
  }
  f32x16 acc = mfma16_zero();
  double dacc[16], z[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 16; ++i) dacc[i] = 0.0;
  float zz[4] = {0, 0, 0, 0};
  float4 ra[2], rb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {                           // (a pixel past the end reads the part's last one and is dropped)
    const long n = p0 + 2 * rr + j;
    const size_t nc = (size_t)(n < p1 ? n : p1 - 1);
    ra[j] = ld4(PA + nc * ld3 + 4 * l);
    rb[j] = ld4(PB + nc * ldb + 4 * l);
  }
  int it = 0;
  for (long t0 = p0; t0 < p1; t0 += LA_TP, ++it) {        // (uniform: the barrier, the shuffles and the MFMA below)
    float pv[2][4], vv[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool live = t0 + 2 * rr + j < p1;
      float4 p;
      if (CTX) p = make_float4(la_exp(ra[j].x - mk.x), la_exp(ra[j].y - mk.y), la_exp(ra[j].z - mk.z), la_exp(ra[j].w - mk.w));
      else p = la_softmax8(ra[j]);
      float4 v = rb[j];
      if (!live) p = v = make_float4(0.f, 0.f, 0.f, 0.f);      // staged as zeros: contributes exactly nothing
      pv[j][0] = p.x; pv[j][1] = p.y; pv[j][2] = p.z; pv[j][3] = p.w;
      vv[j][0] = v.x; vv[j][1] = v.y; vv[j][2] = v.z; vv[j][3] = v.w;
    }
    if (CTX) {
#pragma unroll
      for (int i = 0; i < 4; ++i) zz[i] += pv[0][i] + pv[1][i];
    }
    unsigned char* img = &sT[it & 1][0][0];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int at = mfma16_off(4 * l + i, rr >> 2) + 4 * (rr & 3);
      *reinterpret_cast<unsigned*>(img + at) = pack2<T>(pv[0][i], pv[1][i]);
      *reinterpret_cast<unsigned*>(img + L16_IMG + at) = pack2<T>(vv[0][i], vv[1][i]);
    }
    if (t0 + LA_TP < p1) {                                // the next tile's requests fly over the barrier and the MFMA
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const long n = t0 + LA_TP + 2 * rr + j;
        const size_t nc = (size_t)(n < p1 ? n : p1 - 1);
        ra[j] = ld4(PA + nc * ld3 + 4 * l);
        rb[j] = ld4(PB + nc * ldb + 4 * l);
      }
    }
    __syncthreads();
    {                                                     // K-step `wave` of the tile: pixels 16 wave + 8 hh .. + 7
      const int at = mfma16_off(r, 2 * wave + hh);
      const uint4 a = *reinterpret_cast<const uint4*>(img + at), bb = *reinterpret_cast<const uint4*>(img + L16_IMG + at);
      acc = mfma16<T>(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bb), acc);
    }
    if ((it & (L16_RUN - 1)) == L16_RUN - 1) {            // the end of a run: fp32 -> fp64
#pragma unroll
      for (int i = 0; i < 16; ++i) dacc[i] += (double)acc[i];
      acc = mfma16_zero();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        z[i] += (double)zz[i];
        zz[i] = 0.0f;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) dacc[i] += (double)acc[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) z[i] += (double)zz[i];
  // the four waves (the four K-steps of every tile) meet in wave order
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) comb[((wave - 1) * 16 + i) * 64 + lane] = dacc[i];
  }
  __syncthreads();
  double* dst = work + ((size_t)(b * heads + h) * S + blockIdx.x) * LA_PART;
  if (wave == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const double s = ((dacc[i] + comb[i * 64 + lane]) + comb[(16 + i) * 64 + lane]) + comb[(32 + i) * 64 + lane];
      dst[64 + ((i & 3) + 8 * (i >> 2) + 4 * hh) * LA_D + r] = s;
    }
  }
  if (CTX) {                                              // Z [d]: the 32 loader rows in index order
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) comb[rr * LA_D + 4 * l + i] = z[i];
    __syncthreads();
    if (t < LA_D) {
      double s = comb[t];
      for (int k = 1; k < 32; ++k) s += comb[k * LA_D + t];
      dst[t] = (double)sm[t];
      dst[32 + t] = s;
    }
  }
}

// ================================================================================================ element-wise
// pixels per workgroup (a multiple of 128: 32 per wave and step) of an element-wise pass
inline void l16_runs(int B, int slots, long HW, long& run, unsigned& nrun) {
  long want = 2048 / ((long)B * slots);
  if (want < 1) want = 1;
  run = (HW + want - 1) / want;
  run = (run + 127) / 128 * 128;
  nrun = (unsigned)((HW + run - 1) / run);
}

// the lane's 16 channels of one pixel, 4 hh + 8 g + i at [g][i]
struct L16Vec {
  float v[4][4];
};
// B operand of K-step s: channels g = 2 s, 2 s + 1
template <typename T> __device__ __forceinline__ bf16x8 l16_b(const L16Vec& x, int s) {
  return l16_frag(pack2<T>(x.v[2 * s][0], x.v[2 * s][1]), pack2<T>(x.v[2 * s][2], x.v[2 * s][3]),
                  pack2<T>(x.v[2 * s + 1][0], x.v[2 * s + 1][1]), pack2<T>(x.v[2 * s + 1][2], x.v[2 * s + 1][3]));
}
// A operand M[r][k] of K-step s from a row-major 32 x 32 fp32 matrix: the row's channels 4 hh + 8 g .. + 3, g = 2 s, 2 s + 1
template <typename T> __device__ __forceinline__ bf16x8 l16_a_rows(const float* M, int r, int hh, int s) {
  const float4 x = ld4(M + r * LA_D + 16 * s + 4 * hh), y = ld4(M + r * LA_D + 16 * s + 8 + 4 * hh);
  return l16_frag(pack2<T>(x.x, x.y), pack2<T>(x.z, x.w), pack2<T>(y.x, y.y), pack2<T>(y.z, y.w));
}
// A operand M^T[r][k] of K-step s: column r of the rows 4 hh + 8 g + i
template <typename T> __device__ __forceinline__ bf16x8 l16_a_cols(const float* M, int r, int hh, int s) {
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = M[(8 * (2 * s + (j >> 2)) + 4 * hh + (j & 3)) * LA_D + r];
  return l16_frag(pack2<T>(x[0], x[1]), pack2<T>(x[2], x[3]), pack2<T>(x[4], x[5]), pack2<T>(x[6], x[7]));
}
// ... with row d = 8 g + 4 hh + i of M scaled by sc[d] before it is rounded (the fp16 dv product of la16_apply_kernel)
template <typename T> __device__ __forceinline__ bf16x8 l16_a_cols_scaled(const float* M, const float* sc, int r, int hh, int s) {
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int d = 8 * (2 * s + (j >> 2)) + 4 * hh + (j & 3);
    x[j] = M[d * LA_D + r] * sc[d];
  }
  return l16_frag(pack2<T>(x[0], x[1]), pack2<T>(x[2], x[3]), pack2<T>(x[4], x[5]), pack2<T>(x[6], x[7]));
}
// softmax over a head's 32 channels: 16 here, 16 in lane l ^ 32; both lanes get the same maximum and sum
__device__ __forceinline__ L16Vec l16_softmax(const L16Vec& q) {
  float mx = q.v[0][0];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) mx = fmaxf(mx, q.v[g][i]);
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  L16Vec e;
  float s = 0.0f;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int i = 0; i < 4; ++i) e.v[g][i] = la_exp(q.v[g][i] - mx);
    s += (e.v[g][0] + e.v[g][1]) + (e.v[g][2] + e.v[g][3]);
  }
  s += __shfl_xor(s, 32);
  const float inv = 1.0f / s;
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) e.v[g][i] *= inv;
  return e;
}

// A wave's staging tile: [32 pixels][32 channels] fp32 in rows of L16_TS floats (144 bytes).  Global memory is touched the
// way the fp32 kernels touch it -- the 8 lanes of a (pixel, head) take 16 bytes each, 128 contiguous bytes -- and the tile
// turns that into the MFMA's view, a lane per pixel: with 36-float rows the 16-byte row reads of a ds_read_b128's 16-lane
// groups fall on 16 different bank quads (36 r mod 64 = 4 (9 r mod 16)), and so do the 8-lane groups of the stores.  The
// tile belongs to one wave, whose LDS instructions execute in program order: no workgroup barrier, only a fence that keeps
// the compiler from moving an access across it.
constexpr int L16_TS = 36;
constexpr int L16_TILE = 32 * L16_TS;

__device__ __forceinline__ void l16_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the wave's 32 pixels base .. base + 31 of one 32-channel tensor, four 16-byte loads per lane (lane = (pixel & 7, chunk));
// a pixel past the end reads the run's last one and is never stored
struct L16Raw {
  float4 x[4];
};
__device__ __forceinline__ L16Raw l16_fetch(const float* p, int ld, long base, long p1, int lane) {
  L16Raw v;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long n = base + 8 * j + (lane >> 3);
    v.x[j] = ld4(p + (size_t)(n < p1 ? n : p1 - 1) * ld + 4 * (lane & 7));
  }
  return v;
}
__device__ __forceinline__ void l16_put(float* tile, const L16Raw& v, int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(tile + (8 * j + (lane >> 3)) * L16_TS + 4 * (lane & 7)) = v.x[j];
}
// the lane's view: pixel r, channels 4 hh + 8 g + i
__device__ __forceinline__ L16Vec l16_take(const float* tile, int r, int hh) {
  L16Vec x;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 q = *reinterpret_cast<const float4*>(tile + r * L16_TS + 4 * hh + 8 * g);
    x.v[g][0] = q.x; x.v[g][1] = q.y; x.v[g][2] = q.z; x.v[g][3] = q.w;
  }
  return x;
}
__device__ __forceinline__ void l16_give(float* tile, int r, int hh, const L16Vec& x) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
    *reinterpret_cast<float4*>(tile + r * L16_TS + 4 * hh + 8 * g) = make_float4(x.v[g][0], x.v[g][1], x.v[g][2], x.v[g][3]);
}
// the tile to memory, 128 contiguous bytes per (pixel, head)
__device__ __forceinline__ void l16_flush(const float* tile, float* p, int ld, long base, long p1, int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long n = base + 8 * j + (lane >> 3);
    const float4 y = *reinterpret_cast<const float4*>(tile + (8 * j + (lane >> 3)) * L16_TS + 4 * (lane & 7));
    if (n < p1) st4(p + (size_t)n * ld + 4 * (lane & 7), y.x, y.y, y.z, y.w);
  }
}

// out[n][head 32 + e] = 32^-0.5 sum_d ctx[d][e] softmax_d(q)[d]; workgroup columns >= heads zero the padding
template <typename T>
__global__ __launch_bounds__(LA_BS) void la16_out_kernel(const float* __restrict__ qkv, const float* __restrict__ ctx,
                                                         float* __restrict__ out, long HW, int heads, int ld3, int ldo, long run) {
  __shared__ __attribute__((aligned(16))) float sT[LA_BS / 64][L16_TILE];
  const int t = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
  const long p0 = (long)blockIdx.x * run, p1 = p0 + run < HW ? p0 + run : HW;
  if (h >= heads) {
    const int c = h * LA_D + 4 * (t & 7);
    if (c < ldo)
      for (long n = p0 + (t >> 3); n < p1; n += 32) st4(out + ((size_t)b * HW + n) * ldo + c, 0.f, 0.f, 0.f, 0.f);
    return;
  }
  const int wave = t >> 6, lane = t & 63, r = lane & 31, hh = lane >> 5;
  float* tile = sT[wave];
  const float* Q = qkv + (size_t)b * HW * ld3 + h * LA_D;
  float* O = out + (size_t)b * HW * ldo + h * LA_D;
  long base = p0 + 32 * wave;
  if (base >= p1) return;
  L16Raw raw = l16_fetch(Q, ld3, base, p1, lane);         // (in flight while the A operands load)
  const float* C = ctx + (size_t)(b * heads + h) * LA_D * LA_D;
  const bf16x8 a0 = l16_a_cols<T>(C, r, hh, 0), a1 = l16_a_cols<T>(C, r, hh, 1);            // ctx^T [e][d]
  const float scale = (float)LA_SCALE;
  for (; base < p1; base += 128) {                        // (uniform in the wave: the shuffles and the MFMA)
    l16_put(tile, raw, lane);
    l16_wave_sync();
    const L16Vec qv = l16_take(tile, r, hh);
    if (base + 128 < p1) raw = l16_fetch(Q, ld3, base + 128, p1, lane);
    const L16Vec p = l16_softmax(qv);
    f32x16 o = mfma16<T>(a0, l16_b<T>(p, 0), mfma16_zero());
    o = mfma16<T>(a1, l16_b<T>(p, 1), o);
    L16Vec ov;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i) ov.v[g][i] = o[4 * g + i] * scale;
    l16_wave_sync();
    l16_give(tile, r, hh, ov);
    l16_wave_sync();
    l16_flush(tile, O, ldo, base, p1, lane);
    l16_wave_sync();
  }
}

// dqkv of one (pixel, head) from q, k, v, dO and the head's ctx, (m, Z), dctx, rk; columns >= heads zero the padding.
// s = ctx dO, tk = dctx v and dv = dctx^T ks on the matrix cores; ks, p, dot and the three output formulas in fp32 with
// the unrounded p and ks, as la_apply_kernel writes them.  Two tiles per wave: (dO, q), then (k, v), then (dq, dk), then dv.
// The dv product differs by format.  bf16 rounds ks = exp(k - m) (1 / Z) as the operand.  ks is about 1 / n, which from
// 128 x 128 pixels on lies in fp16's subnormals, so fp16 moves the division to the other side:
//   dv[e][n] = sum_d fp16(dctx[d][e] iz[d]) fp16(exp(k[d][n] - m[d])),
// a second pair of dctx^T fragments scaled per contraction row, built once per workgroup, against an operand in (0, 1].
template <typename T>
__global__ __launch_bounds__(LA_BS) void la16_apply_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                           const float* __restrict__ ctx, const float* __restrict__ kstat,
                                                           const float* __restrict__ dctx, const float* __restrict__ rk,
                                                           float* __restrict__ dqkv, long HW, int heads, int ld3, int ldo,
                                                           long run) {
  __shared__ __attribute__((aligned(16))) float sT[LA_BS / 64][2][L16_TILE];
  __shared__ __attribute__((aligned(16))) float sK[3 * LA_D];         // m, 1 / Z, rk
  const int t = threadIdx.x, h = blockIdx.y, b = blockIdx.z, hidden = heads * LA_D;
  const long p0 = (long)blockIdx.x * run, p1 = p0 + run < HW ? p0 + run : HW;
  if (h >= heads) {
    const int c = 3 * hidden + (h - heads) * LA_D + 4 * (t & 7);
    if (c < ld3)
      for (long n = p0 + (t >> 3); n < p1; n += 32) st4(dqkv + ((size_t)b * HW + n) * ld3 + c, 0.f, 0.f, 0.f, 0.f);
    return;
  }
  const int wave = t >> 6, lane = t & 63, r = lane & 31, hh = lane >> 5;
  float *t0 = sT[wave][0], *t1 = sT[wave][1];
  const size_t bh = (size_t)(b * heads + h);
  const float* Q = qkv + (size_t)b * HW * ld3 + h * LA_D;
  const float* DO = dout + (size_t)b * HW * ldo + h * LA_D;
  float* G = dqkv + (size_t)b * HW * ld3 + h * LA_D;
  long base = p0 + 32 * wave;
  const bool any = base < p1;                             // (a wave without pixels still meets the barrier below)
  L16Raw rdo, rq, rk4, rv;
  if (any) {
    rdo = l16_fetch(DO, ldo, base, p1, lane);
    rq = l16_fetch(Q, ld3, base, p1, lane);
    rk4 = l16_fetch(Q + hidden, ld3, base, p1, lane);
    rv = l16_fetch(Q + 2 * hidden, ld3, base, p1, lane);
  }
  const float *C = ctx + bh * LA_D * LA_D, *D = dctx + bh * LA_D * LA_D;
  const bf16x8 c0 = l16_a_rows<T>(C, r, hh, 0), c1 = l16_a_rows<T>(C, r, hh, 1);            // ctx  [d][e]
  const bf16x8 d0 = l16_a_rows<T>(D, r, hh, 0), d1 = l16_a_rows<T>(D, r, hh, 1);            // dctx [d][e]
  constexpr bool FOLD = std::is_same<T, f16>::value;      // dv: 1 / Z on the dctx^T side (above)
  bf16x8 e0, e1;                                          // dctx^T [e][d]
  if (!FOLD) {
    e0 = l16_a_cols<T>(D, r, hh, 0);
    e1 = l16_a_cols<T>(D, r, hh, 1);
  }
  if (t < LA_D) {
    sK[t] = kstat[(bh * LA_D + t) * 2];
    sK[LA_D + t] = 1.0f / kstat[(bh * LA_D + t) * 2 + 1];
    sK[2 * LA_D + t] = rk[bh * LA_D + t];
  }
  __syncthreads();
  if (!any) return;
  if (FOLD) {                                             // dctx^T [e][d] iz[d]
    e0 = l16_a_cols_scaled<T>(D, sK + LA_D, r, hh, 0);
    e1 = l16_a_cols_scaled<T>(D, sK + LA_D, r, hh, 1);
  }
  const float scale = (float)LA_SCALE;
  for (; base < p1; base += 128) {                        // (uniform in the wave: the shuffles and the MFMAs)
    l16_put(t0, rdo, lane);
    l16_put(t1, rq, lane);
    l16_wave_sync();
    const L16Vec dov = l16_take(t0, r, hh), qv = l16_take(t1, r, hh);
    l16_wave_sync();
    l16_put(t0, rk4, lane);
    l16_put(t1, rv, lane);
    l16_wave_sync();
    const L16Vec kv = l16_take(t0, r, hh), vv = l16_take(t1, r, hh);
    if (base + 128 < p1) {
      rdo = l16_fetch(DO, ldo, base + 128, p1, lane);
      rq = l16_fetch(Q, ld3, base + 128, p1, lane);
      rk4 = l16_fetch(Q + hidden, ld3, base + 128, p1, lane);
      rv = l16_fetch(Q + 2 * hidden, ld3, base + 128, p1, lane);
    }
    f32x16 s = mfma16<T>(c0, l16_b<T>(dov, 0), mfma16_zero());
    s = mfma16<T>(c1, l16_b<T>(dov, 1), s);
    f32x16 tk = mfma16<T>(d0, l16_b<T>(vv, 0), mfma16_zero());
    tk = mfma16<T>(d1, l16_b<T>(vv, 1), tk);
    L16Vec ks, pk;                                        // pk = exp(k - m), ks = pk / Z
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 mk = *reinterpret_cast<const float4*>(sK + 8 * g + 4 * hh);
      const float4 iz = *reinterpret_cast<const float4*>(sK + LA_D + 8 * g + 4 * hh);
      pk.v[g][0] = la_exp(kv.v[g][0] - mk.x);
      pk.v[g][1] = la_exp(kv.v[g][1] - mk.y);
      pk.v[g][2] = la_exp(kv.v[g][2] - mk.z);
      pk.v[g][3] = la_exp(kv.v[g][3] - mk.w);
      ks.v[g][0] = pk.v[g][0] * iz.x;
      ks.v[g][1] = pk.v[g][1] * iz.y;
      ks.v[g][2] = pk.v[g][2] * iz.z;
      ks.v[g][3] = pk.v[g][3] * iz.w;
    }
    f32x16 dv = mfma16<T>(e0, l16_b<T>(FOLD ? pk : ks, 0), mfma16_zero());
    dv = mfma16<T>(e1, l16_b<T>(FOLD ? pk : ks, 1), dv);
    const L16Vec p = l16_softmax(qv);
    float dot = 0.0f;
#pragma unroll
    for (int g = 0; g < 4; ++g)
      dot += (p.v[g][0] * s[4 * g] + p.v[g][1] * s[4 * g + 1]) + (p.v[g][2] * s[4 * g + 2] + p.v[g][3] * s[4 * g + 3]);
    dot += __shfl_xor(dot, 32);
    L16Vec dq, dk, dvv;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 rkv = *reinterpret_cast<const float4*>(sK + 2 * LA_D + 8 * g + 4 * hh);
      const float rkc[4] = {rkv.x, rkv.y, rkv.z, rkv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dq.v[g][i] = scale * p.v[g][i] * (s[4 * g + i] - dot);
        dk.v[g][i] = ks.v[g][i] * (tk[4 * g + i] - rkc[i]);
        dvv.v[g][i] = dv[4 * g + i];
      }
    }
    l16_wave_sync();
    l16_give(t0, r, hh, dq);
    l16_give(t1, r, hh, dk);
    l16_wave_sync();
    l16_flush(t0, G, ld3, base, p1, lane);
    l16_flush(t1, G + hidden, ld3, base, p1, lane);
    l16_wave_sync();
    l16_give(t0, r, hh, dvv);
    l16_wave_sync();
    l16_flush(t0, G + 2 * hidden, ld3, base, p1, lane);
    l16_wave_sync();
  }
}

// ================================================================================================ host side
// One body per pass for both formats; `fn` is the entry point's name in the messages.
template <typename T>
int la16_context(const char* fn, const float* qkv, double* work, float* ctx, float* kstat, int B, int H, int W, int heads, int ld3,
                 void* stream) {
  LD_REQUIRE(la_shape_ok(B, H, W, heads) && la_strides_ok(heads, ld3, heads * LA_D),
             "%s: B=%d H=%d W=%d heads=%d ld3=%d (heads >= 1, ld3 >= 96 heads a multiple of 4)", fn, B, H, W, heads, ld3);
  LD_REQUIRE(qkv && work && ctx && kstat, "%s: null pointer", fn);
  LD_REQUIRE(dn_aligned16(qkv), "%s: qkv is not 16-byte aligned", fn);
  const long HW = (long)H * W;
  hipStream_t st = dn_st(stream);
  long ppp;
  int S;
  la_parts(B, heads, HW, ppp, S);
  const auto reduce = la16_reduce_kernel<T, true>;
  LD_LAUNCH(reduce, dim3((unsigned)S, (unsigned)heads, (unsigned)B), dim3(LA_BS), 0, st, qkv, (const float*)nullptr, work, HW,
            heads, ld3, 0, ppp, S);
  LD_LAUNCH(la_context_merge_kernel, dim3((unsigned)(B * heads)), dim3(256), 0, st, (const double*)work, ctx, kstat, S);
  LD_LAUNCH_CHECK(fn + 3);                                // (without "ld_")
  return LD_OK;
}

template <typename T>
int la16_out(const char* fn, const float* qkv, const float* ctx, float* out, int B, int H, int W, int heads, int ld3, int ldo,
             void* stream) {
  LD_REQUIRE(la_shape_ok(B, H, W, heads) && la_strides_ok(heads, ld3, ldo),
             "%s: B=%d H=%d W=%d heads=%d ld3=%d ldo=%d (heads >= 1, ld3 >= 96 heads, ldo >= 32 heads, multiples of 4)", fn, B, H, W,
             heads, ld3, ldo);
  LD_REQUIRE(qkv && ctx && out, "%s: null pointer", fn);
  LD_REQUIRE(dn_aligned16(qkv) && dn_aligned16(ctx) && dn_aligned16(out), "%s: a pointer is not 16-byte aligned", fn);
  const long HW = (long)H * W;
  const int slots = heads + (ldo - heads * LA_D + LA_D - 1) / LA_D;
  LD_REQUIRE(slots <= 65535, "%s: ldo %d", fn, ldo);
  long run;
  unsigned nrun;
  l16_runs(B, slots, HW, run, nrun);
  LD_LAUNCH(la16_out_kernel<T>, dim3(nrun, (unsigned)slots, (unsigned)B), dim3(LA_BS), 0, dn_st(stream), qkv, ctx, out, HW, heads,
            ld3, ldo, run);
  LD_LAUNCH_CHECK(fn + 3);
  return LD_OK;
}

template <typename T>
int la16_backward_reduce(const char* fn, const float* qkv, const float* dout, const float* ctx, double* work, float* dctx, float* rk,
                         int B, int H, int W, int heads, int ld3, int ldo, void* stream) {
  LD_REQUIRE(la_shape_ok(B, H, W, heads) && la_strides_ok(heads, ld3, ldo),
             "%s: B=%d H=%d W=%d heads=%d ld3=%d ldo=%d (heads >= 1, ld3 >= 96 heads, ldo >= 32 heads, multiples of 4)", fn, B, H, W,
             heads, ld3, ldo);
  LD_REQUIRE(qkv && dout && ctx && work && dctx && rk, "%s: null pointer", fn);
  LD_REQUIRE(dn_aligned16(qkv) && dn_aligned16(dout), "%s: a pointer is not 16-byte aligned", fn);
  const long HW = (long)H * W;
  hipStream_t st = dn_st(stream);
  long ppp;
  int S;
  la_parts(B, heads, HW, ppp, S);
  const auto reduce = la16_reduce_kernel<T, false>;
  LD_LAUNCH(reduce, dim3((unsigned)S, (unsigned)heads, (unsigned)B), dim3(LA_BS), 0, st, qkv, dout, work, HW, heads, ld3, ldo, ppp,
            S);
  LD_LAUNCH(la_reduce_merge_kernel, dim3((unsigned)(B * heads)), dim3(256), 0, st, (const double*)work, ctx, dctx, rk, S);
  LD_LAUNCH_CHECK(fn + 3);
  return LD_OK;
}

template <typename T>
int la16_backward_apply(const char* fn, const float* qkv, const float* dout, const float* ctx, const float* kstat, const float* dctx,
                        const float* rk, float* dqkv, int B, int H, int W, int heads, int ld3, int ldo, void* stream) {
  LD_REQUIRE(la_shape_ok(B, H, W, heads) && la_strides_ok(heads, ld3, ldo),
             "%s: B=%d H=%d W=%d heads=%d ld3=%d ldo=%d (heads >= 1, ld3 >= 96 heads, ldo >= 32 heads, multiples of 4)", fn, B, H, W,
             heads, ld3, ldo);
  LD_REQUIRE(qkv && dout && ctx && kstat && dctx && rk && dqkv, "%s: null pointer", fn);
  LD_REQUIRE(dn_aligned16(qkv) && dn_aligned16(dout) && dn_aligned16(ctx) && dn_aligned16(dctx) && dn_aligned16(dqkv),
             "%s: a pointer is not 16-byte aligned", fn);
  const long HW = (long)H * W;
  const int slots = heads + (ld3 - 3 * heads * LA_D + LA_D - 1) / LA_D;
  LD_REQUIRE(slots <= 65535, "%s: ld3 %d", fn, ld3);
  long run;
  unsigned nrun;
  l16_runs(B, slots, HW, run, nrun);
  LD_LAUNCH(la16_apply_kernel<T>, dim3(nrun, (unsigned)slots, (unsigned)B), dim3(LA_BS), 0, dn_st(stream), qkv, dout, ctx, kstat,
            dctx, rk, dqkv, HW, heads, ld3, ldo, run);
  LD_LAUNCH_CHECK(fn + 3);
  return LD_OK;
}
}  // namespace

#define LA16_ENTRY(suffix, T)                                                                                                     \
  extern "C" int ld_dn_la_context##suffix(const float* qkv, double* work, float* ctx, float* kstat, int B, int H, int W,         \
                                          int heads, int ld3, void* stream) {                                                    \
    return la16_context<T>("ld_dn_la_context" #suffix, qkv, work, ctx, kstat, B, H, W, heads, ld3, stream);                      \
  }                                                                                                                               \
  extern "C" int ld_dn_la_out##suffix(const float* qkv, const float* ctx, float* out, int B, int H, int W, int heads, int ld3,   \
                                      int ldo, void* stream) {                                                                   \
    return la16_out<T>("ld_dn_la_out" #suffix, qkv, ctx, out, B, H, W, heads, ld3, ldo, stream);                                 \
  }                                                                                                                               \
  extern "C" int ld_dn_la_backward_reduce##suffix(const float* qkv, const float* dout, const float* ctx, double* work,           \
                                                  float* dctx, float* rk, int B, int H, int W, int heads, int ld3, int ldo,      \
                                                  void* stream) {                                                                \
    return la16_backward_reduce<T>("ld_dn_la_backward_reduce" #suffix, qkv, dout, ctx, work, dctx, rk, B, H, W, heads, ld3, ldo, \
                                   stream);                                                                                      \
  }                                                                                                                               \
  extern "C" int ld_dn_la_backward_apply##suffix(const float* qkv, const float* dout, const float* ctx, const float* kstat,      \
                                                 const float* dctx, const float* rk, float* dqkv, int B, int H, int W,           \
                                                 int heads, int ld3, int ldo, void* stream) {                                    \
    return la16_backward_apply<T>("ld_dn_la_backward_apply" #suffix, qkv, dout, ctx, kstat, dctx, rk, dqkv, B, H, W, heads, ld3, \
                                  ldo, stream);                                                                                  \
  }
LA16_ENTRY(16, bf16)
LA16_ENTRY(_f16, f16)
