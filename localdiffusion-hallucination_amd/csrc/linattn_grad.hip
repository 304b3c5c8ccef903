// Training the denoiser, second slice: what a trainable LinearAttention (ddpm.py:214-251) needs besides its two 1x1
// convolutions -- RMSNorm (ddpm.py:126-132) with its backward, and the attention core with its backward.  The convolutions
// and their gradients are ld_pc_conv / ld_seg_wgrad / ld_dn_colsum launches (linattn_grad.py).
//
// fp32 throughout, the layout of denoiser_grad.hip: activations NHWC with a pixel stride >= the channel count, the
// padding never read into a sum and written as zeros.  qkv is [B, H, W, ld3] with q at channel 0, k at `hidden`, v at
// 2 * hidden, a head's 32 channels contiguous at head * 32 inside each.  Every sum over pixels is added in a fixed order
// (fp32 inside a tile of 64 pixels, fp64 across tiles, parts and samples) with no floating-point atomics, and the number
// of parts depends on the shape alone, so every result is reproducible bit for bit.  Nothing allocates.
//
// Who owns what:
//   * RMSNorm forward and its dx: the L = 1 .. 64 (a power of two) lanes of one pixel own four consecutive channels each
//     (one 16-byte access) and meet in a butterfly of shuffles for the pixel's norm or dot product; dg is the column-sum
//     pass of denoiser_grad.hip over dout x r (r = 1 / norm, saved by the forward as one float per pixel).
//   * The two reductions over pixels (context; dctx of the backward): one workgroup per (part of the pixel axis, head,
//     sample).  A tile of 64 pixels lands in LDS as P [64][32] (exp(k - m), or softmax_d(q)) and V [64][32] (v, or dO);
//     a thread owns a 2 x 4 block of the 32 x 32 product and every second pixel of the tile, so a pixel costs it one
//     8-byte and one 16-byte LDS read for 8 multiply-adds.  The parts' fp64 partials go to `work`; a second launch merges
//     them in index order.
//   * The two element-wise passes (output; dqkv of the backward): the 8 lanes of one (pixel, head) own four channels each:
//     every global access is 16 bytes per lane and 128 contiguous bytes per (pixel, head); the softmax over the head's 32
//     channels is a three-step butterfly; a 32-vector another lane holds comes by shuffles; the head's 32 x 32 ctx / dctx
//     sit in LDS, once as [d][e] and once transposed, so that both a row block and a column block are conflict-free
//     16-byte reads.
// exp is v_exp_f32 on a * log2(e): the arguments are <= 0 (a maximum is always subtracted) and the rounding of the product
// is 6e-8 |a| relative to a term that weighs e^a, i.e. at most 2.2e-8 of the largest term.
#include "common.hip.h"
#include "dn_common.hip.h"
#include "la_common.hip.h"

namespace {

// ================================================================================================ RMSNorm
inline int rms_lanes(int ldc) {
  int L = 1;
  while (L < ldc / 4 && L < 64) L <<= 1;
  return L;
}
inline unsigned rms_grid(long P, int L) {
  const long per = LA_BS / L, wgs = (P + per - 1) / per;
  return (unsigned)(wgs < 2048 ? wgs : 2048);
}

// out = x r g sqrt(C), r = 1 / max(|x_p|, 1e-12); rinv [P] = r (or NULL)
__global__ __launch_bounds__(LA_BS) void rms_forward_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                            float* __restrict__ rinv, float* __restrict__ out, long P, int C,
                                                            int ldc, int L, float scale) {
  const int li = (int)threadIdx.x & (L - 1), grp = (int)threadIdx.x / L, per = LA_BS / L;
  const int Q = ldc / 4, Qc = C / 4;
  for (long base = (long)blockIdx.x * per; base < P; base += (long)gridDim.x * per) {      // (uniform: the shuffles below)
    const long p = base + grp;
    const bool live = p < P;
    const float* src = x + (size_t)(live ? p : P - 1) * ldc;
    float4 first = make_float4(0.f, 0.f, 0.f, 0.f);
    float ss = 0.0f;
    for (int q = li; q < Qc; q += L) {
      const float4 v = ld4(src + 4 * q);
      if (q == li) first = v;
      ss += ((v.x * v.x + v.y * v.y) + v.z * v.z) + v.w * v.w;
    }
    for (int off = L >> 1; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
    const float r = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    if (!live) continue;
    if (rinv && li == 0) rinv[p] = r;
    float* dst = out + (size_t)p * ldc;
    for (int q = li; q < Q; q += L) {
      if (q >= Qc) {
        st4(dst + 4 * q, 0.f, 0.f, 0.f, 0.f);
        continue;
      }
      const float4 v = q == li ? first : ld4(src + 4 * q), gg = ld4(g + 4 * q);
      st4(dst + 4 * q, v.x * r * gg.x * scale, v.y * r * gg.y * scale, v.z * r * gg.z * scale, v.w * r * gg.w * scale);
    }
  }
}

// dx = r (e - u sum_c u_c e_c), u = x r, e = dout g sqrt(C).  dx may be dout: a lane reads what it overwrites first.
__global__ __launch_bounds__(LA_BS) void rms_dx_kernel(const float* dout, const float* __restrict__ x,
                                                       const float* __restrict__ g, const float* __restrict__ rinv, float* dx,
                                                       long P, int C, int ldc, int L, float scale) {
  const int li = (int)threadIdx.x & (L - 1), grp = (int)threadIdx.x / L, per = LA_BS / L;
  const int Q = ldc / 4, Qc = C / 4;
  for (long base = (long)blockIdx.x * per; base < P; base += (long)gridDim.x * per) {
    const long p = base + grp;
    const bool live = p < P;
    const size_t at = (size_t)(live ? p : P - 1) * ldc;
    const float r = rinv[live ? p : P - 1];
    float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), e0 = x0;
    float dot = 0.0f;
    for (int q = li; q < Qc; q += L) {
      const float4 v = ld4(x + at + 4 * q), d = ld4(dout + at + 4 * q), gg = ld4(g + 4 * q);
      const float4 e = make_float4(d.x * gg.x * scale, d.y * gg.y * scale, d.z * gg.z * scale, d.w * gg.w * scale);
      if (q == li) { x0 = v; e0 = e; }
      dot += ((v.x * e.x + v.y * e.y) + v.z * e.z) + v.w * e.w;
    }
    for (int off = L >> 1; off >= 1; off >>= 1) dot += __shfl_xor(dot, off);
    dot *= r;                                            // = sum_c u_c e_c
    if (!live) continue;
    for (int q = li; q < Q; q += L) {
      if (q >= Qc) {
        st4(dx + at + 4 * q, 0.f, 0.f, 0.f, 0.f);
        continue;
      }
      float4 v = x0, e = e0;
      if (q != li) {
        const float4 d = ld4(dout + at + 4 * q), gg = ld4(g + 4 * q);
        v = ld4(x + at + 4 * q);
        e = make_float4(d.x * gg.x * scale, d.y * gg.y * scale, d.z * gg.z * scale, d.w * gg.w * scale);
      }
      st4(dx + at + 4 * q, r * (e.x - v.x * r * dot), r * (e.y - v.y * r * dot), r * (e.z - v.z * r * dot),
          r * (e.w - v.w * r * dot));
    }
  }
}

// part [B][nchunk][C] = sum over the run of dout_c u_c
__global__ __launch_bounds__(DN_BS) void rms_dg_kernel(const float* __restrict__ dout, const float* __restrict__ x,
                                                       const float* __restrict__ rinv, double* __restrict__ part, long HW, int C,
                                                       int ldc, long ppc, int nchunk) {
  __shared__ double red[DN_BS * 4];
  const DnPos t = dn_pos(C / 4, HW, ppc);
  const int b = blockIdx.z;
  double v[4] = {0, 0, 0, 0};
  if (t.active) {
    const size_t base = ((size_t)b * HW) * ldc + 4 * t.q;
    const float* rr = rinv + (size_t)b * HW;
#pragma unroll 4
    for (long p = t.p0 + t.r; p < t.p1; p += t.R) {
      const float4 a = ld4(x + base + (size_t)p * ldc), d = ld4(dout + base + (size_t)p * ldc);
      const float r = rr[p];
      v[0] += (double)(d.x * (a.x * r));
      v[1] += (double)(d.y * (a.y * r));
      v[2] += (double)(d.z * (a.z * r));
      v[3] += (double)(d.w * (a.w * r));
    }
  }
  if (dn_block_sum<4>(t, v, red)) {
    double* dst = part + ((size_t)b * nchunk + blockIdx.x) * C + 4 * t.q;
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[i] = v[i];
  }
}
// dg [C] = sqrt(C) x the n runs added in (b, run) order
__global__ __launch_bounds__(256) void rms_dg_final_kernel(const double* __restrict__ part, float* __restrict__ dg, int n, int C,
                                                           double scale) {
  const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (c >= C) return;
  double acc = 0.0;
#pragma unroll 8
  for (int k = 0; k < n; ++k) acc += part[(size_t)k * C + c];
  dg[c] = (float)(scale * acc);
}

// ================================================================================================ attention: reductions
// (the parts, the runs, the 8-lane softmax, the two merge kernels and the shape checks: la_common.hip.h)
// One tile: acc [2][4] += sum over this thread's pixels of P[n][2 dp + i] V[n][4 eg + j], z [2] += sum of P (fp32 inside
// the tile, fp64 across tiles).
__device__ __forceinline__ void la_tile(const float* sP, const float* sV, int half, int dp, int eg, double (&acc)[8],
                                        double (&z)[2]) {
  float a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, zz[2] = {0, 0};
#pragma unroll 8
  for (int nl = half; nl < LA_TP; nl += 2) {
    const float2 p = *reinterpret_cast<const float2*>(sP + nl * LA_D + 2 * dp);
    const float4 v = *reinterpret_cast<const float4*>(sV + nl * LA_D + 4 * eg);
    a[0] += p.x * v.x; a[1] += p.x * v.y; a[2] += p.x * v.z; a[3] += p.x * v.w;
    a[4] += p.y * v.x; a[5] += p.y * v.y; a[6] += p.y * v.z; a[7] += p.y * v.w;
    zz[0] += p.x;
    zz[1] += p.y;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] += (double)a[i];
  z[0] += (double)zz[0];
  z[1] += (double)zz[1];
}
// The two halves of the workgroup (even and odd pixels) meet: threads 0..127 end with the part's sums.
__device__ __forceinline__ bool la_meet(double* comb, int half, int u, double (&acc)[8], double (&z)[2]) {
  if (half == 1) {
#pragma unroll
    for (int i = 0; i < 8; ++i) comb[u * 10 + i] = acc[i];
    comb[u * 10 + 8] = z[0];
    comb[u * 10 + 9] = z[1];
  }
  __syncthreads();
  if (half == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += comb[u * 10 + i];
    z[0] += comb[u * 10 + 8];
    z[1] += comb[u * 10 + 9];
  }
  return half == 0;
}
__device__ __forceinline__ void la_store_part(double* dst, int dp, int eg, const double (&acc)[8]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[64 + (2 * dp + i) * LA_D + 4 * eg + j] = acc[i * 4 + j];
}

// part (b, head, s) = (m, Z, ctx Z) of pixels [s ppp, (s + 1) ppp): the part's own maximum first, then the sums
__global__ __launch_bounds__(LA_BS) void la_context_kernel(const float* __restrict__ qkv, double* __restrict__ work, long HW,
                                                           int heads, int ld3, long ppp, int S) {
  __shared__ __attribute__((aligned(16))) float sP[LA_TP * LA_D];
  __shared__ __attribute__((aligned(16))) float sV[LA_TP * LA_D];
  __shared__ __attribute__((aligned(16))) float sm[LA_D];
  __shared__ double comb[128 * 10];
  const int t = threadIdx.x, h = blockIdx.y, b = blockIdx.z, hidden = heads * LA_D;
  const long p0 = (long)blockIdx.x * ppp, p1 = p0 + ppp < HW ? p0 + ppp : HW;
  const float* K = qkv + (size_t)b * HW * ld3 + hidden + h * LA_D;
  const float* V = K + hidden;
  const int r = t >> 3, l = t & 7;
  {                                                       // the part's maximum of every k channel (sP as scratch)
    float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (long n = p0 + r; n < p1; n += 32) {
      const float4 k = ld4(K + (size_t)n * ld3 + 4 * l);
      mx.x = fmaxf(mx.x, k.x); mx.y = fmaxf(mx.y, k.y); mx.z = fmaxf(mx.z, k.z); mx.w = fmaxf(mx.w, k.w);
    }
    *reinterpret_cast<float4*>(sP + r * LA_D + 4 * l) = mx;
    __syncthreads();
    if (t < LA_D) {
      float m = sP[t];
      for (int i = 1; i < 32; ++i) m = fmaxf(m, sP[i * LA_D + t]);
      sm[t] = m;                                          // (finite: a part holds at least one pixel)
    }
    __syncthreads();
  }
  const float4 mk = *reinterpret_cast<const float4*>(sm + 4 * l);
  const int half = t >> 7, u = t & 127, dp = u >> 3, eg = u & 7;
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, z[2] = {0, 0};
  for (long t0 = p0; t0 < p1; t0 += LA_TP) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nl = r + 32 * j;
      const long n = t0 + nl;
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f), v = p;
      if (n < p1) {
        const float4 k = ld4(K + (size_t)n * ld3 + 4 * l);
        v = ld4(V + (size_t)n * ld3 + 4 * l);
        p = make_float4(la_exp(k.x - mk.x), la_exp(k.y - mk.y), la_exp(k.z - mk.z), la_exp(k.w - mk.w));
      }
      *reinterpret_cast<float4*>(sP + nl * LA_D + 4 * l) = p;
      *reinterpret_cast<float4*>(sV + nl * LA_D + 4 * l) = v;
    }
    __syncthreads();
    la_tile(sP, sV, half, dp, eg, acc, z);
    __syncthreads();
  }
  if (la_meet(comb, half, u, acc, z)) {
    double* dst = work + ((size_t)(b * heads + h) * S + blockIdx.x) * LA_PART;
    la_store_part(dst, dp, eg, acc);
    if (eg == 0) {
      dst[2 * dp] = (double)sm[2 * dp];
      dst[2 * dp + 1] = (double)sm[2 * dp + 1];
      dst[32 + 2 * dp] = z[0];
      dst[32 + 2 * dp + 1] = z[1];
    }
  }
}

// part (b, head, s) [d][e] = sum over the part's pixels of softmax_d(q)[d] dO[e]
__global__ __launch_bounds__(LA_BS) void la_reduce_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                          double* __restrict__ work, long HW, int heads, int ld3, int ldo,
                                                          long ppp, int S) {
  __shared__ __attribute__((aligned(16))) float sP[LA_TP * LA_D];
  __shared__ __attribute__((aligned(16))) float sV[LA_TP * LA_D];
  __shared__ double comb[128 * 10];
  const int t = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
  const long p0 = (long)blockIdx.x * ppp, p1 = p0 + ppp < HW ? p0 + ppp : HW;
  const float* Q = qkv + (size_t)b * HW * ld3 + h * LA_D;
  const float* dO = dout + (size_t)b * HW * ldo + h * LA_D;
  const int r = t >> 3, l = t & 7;
  const int half = t >> 7, u = t & 127, dp = u >> 3, eg = u & 7;
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, z[2] = {0, 0};
  for (long t0 = p0; t0 < p1; t0 += LA_TP) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nl = r + 32 * j;
      const long n = t0 + nl;
      const bool live = n < p1;
      const size_t nc = (size_t)(live ? n : p1 - 1);       // (every lane runs the butterfly)
      float4 p = la_softmax8(ld4(Q + nc * ld3 + 4 * l)), v = ld4(dO + nc * ldo + 4 * l);
      if (!live) p = v = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(sP + nl * LA_D + 4 * l) = p;
      *reinterpret_cast<float4*>(sV + nl * LA_D + 4 * l) = v;
    }
    __syncthreads();
    la_tile(sP, sV, half, dp, eg, acc, z);
    __syncthreads();
  }
  if (la_meet(comb, half, u, acc, z)) la_store_part(work + ((size_t)(b * heads + h) * S + blockIdx.x) * LA_PART, dp, eg, acc);
}

// ================================================================================================ attention: element-wise
// component i of the float4 that lane `src` of this (pixel, head)'s 8 lanes holds
__device__ __forceinline__ float4 la_from(const float4& v, int src) {
  return make_float4(__shfl(v.x, src, 8), __shfl(v.y, src, 8), __shfl(v.z, src, 8), __shfl(v.w, src, 8));
}

// out[n][head 32 + e] = 32^-0.5 sum_d ctx[d][e] softmax_d(q)[d]; workgroup columns >= heads zero the padding
__global__ __launch_bounds__(LA_BS) void la_out_kernel(const float* __restrict__ qkv, const float* __restrict__ ctx,
                                                       float* __restrict__ out, long HW, int heads, int ld3, int ldo, long run) {
  __shared__ __attribute__((aligned(16))) float sC[LA_D * LA_D];
  const int t = threadIdx.x, h = blockIdx.y, b = blockIdx.z, l = t & 7, g = t >> 3;
  const long p0 = (long)blockIdx.x * run, p1 = p0 + run < HW ? p0 + run : HW;
  if (h >= heads) {
    const int c = h * LA_D + 4 * l;
    if (c < ldo)
      for (long n = p0 + g; n < p1; n += 32) st4(out + ((size_t)b * HW + n) * ldo + c, 0.f, 0.f, 0.f, 0.f);
    return;
  }
  *reinterpret_cast<float4*>(sC + 4 * t) = ld4(ctx + ((size_t)(b * heads + h) * LA_D * LA_D) + 4 * t);
  __syncthreads();
  const float* Q = qkv + (size_t)b * HW * ld3 + h * LA_D + 4 * l;
  const float scale = (float)LA_SCALE;
  for (long base = p0; base < p1; base += 32) {           // (uniform: the shuffles below)
    const long n = base + g;
    const bool live = n < p1;
    const float4 p = la_softmax8(ld4(Q + (size_t)(live ? n : p1 - 1) * ld3));
    float o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int src = 0; src < 8; ++src) {
      const float4 ps = la_from(p, src);
      const float pv[4] = {ps.x, ps.y, ps.z, ps.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 c = *reinterpret_cast<const float4*>(sC + (4 * src + i) * LA_D + 4 * l);
        o[0] += c.x * pv[i]; o[1] += c.y * pv[i]; o[2] += c.z * pv[i]; o[3] += c.w * pv[i];
      }
    }
    if (live) st4(out + ((size_t)b * HW + n) * ldo + h * LA_D + 4 * l, o[0] * scale, o[1] * scale, o[2] * scale, o[3] * scale);
  }
}

// dqkv of one (pixel, head) from q, k, v, dO and the head's ctx, (m, Z), dctx, rk; columns >= heads zero the padding.
// (The 96 LDS reads of a pixel are the same for every pixel; `lds0` hides that from hipcc, which would otherwise keep them
// in 384 registers: it took 274 and spilled, one wave per SIMD.  Re-read, the kernel needs about 90.)
__global__ __launch_bounds__(LA_BS) void la_apply_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                         const float* __restrict__ ctx, const float* __restrict__ kstat,
                                                         const float* __restrict__ dctx, const float* __restrict__ rk,
                                                         float* __restrict__ dqkv, long HW, int heads, int ld3, int ldo,
                                                         long run) {
  __shared__ __attribute__((aligned(16))) float sCT[LA_D * LA_D];     // ctx  [e][d]
  __shared__ __attribute__((aligned(16))) float sD[LA_D * LA_D];      // dctx [d][e]
  __shared__ __attribute__((aligned(16))) float sDT[LA_D * LA_D];     // dctx [e][d]
  __shared__ __attribute__((aligned(16))) float sK[3 * LA_D];         // m, 1 / Z, rk
  const int t = threadIdx.x, h = blockIdx.y, b = blockIdx.z, l = t & 7, g = t >> 3, hidden = heads * LA_D;
  const long p0 = (long)blockIdx.x * run, p1 = p0 + run < HW ? p0 + run : HW;
  if (h >= heads) {
    const int c = 3 * hidden + (h - heads) * LA_D + 4 * l;
    if (c < ld3)
      for (long n = p0 + g; n < p1; n += 32) st4(dqkv + ((size_t)b * HW + n) * ld3 + c, 0.f, 0.f, 0.f, 0.f);
    return;
  }
  {
    const size_t bh = (size_t)(b * heads + h);
    const float4 c = ld4(ctx + bh * LA_D * LA_D + 4 * t), dc = ld4(dctx + bh * LA_D * LA_D + 4 * t);
    const int d = t >> 3, e = 4 * (t & 7);
    *reinterpret_cast<float4*>(sD + 4 * t) = dc;
    sCT[(e + 0) * LA_D + d] = c.x; sCT[(e + 1) * LA_D + d] = c.y; sCT[(e + 2) * LA_D + d] = c.z; sCT[(e + 3) * LA_D + d] = c.w;
    sDT[(e + 0) * LA_D + d] = dc.x; sDT[(e + 1) * LA_D + d] = dc.y; sDT[(e + 2) * LA_D + d] = dc.z; sDT[(e + 3) * LA_D + d] = dc.w;
    if (t < LA_D) {
      sK[t] = kstat[(bh * LA_D + t) * 2];
      sK[LA_D + t] = 1.0f / kstat[(bh * LA_D + t) * 2 + 1];
      sK[2 * LA_D + t] = rk[bh * LA_D + t];
    }
  }
  __syncthreads();
  const float4 mk = *reinterpret_cast<const float4*>(sK + 4 * l), iz = *reinterpret_cast<const float4*>(sK + LA_D + 4 * l),
               rkv = *reinterpret_cast<const float4*>(sK + 2 * LA_D + 4 * l);
  const float* src = qkv + (size_t)b * HW * ld3 + h * LA_D + 4 * l;
  const float scale = (float)LA_SCALE;
  for (long base = p0; base < p1; base += 32) {           // (uniform: the shuffles below)
    const long n = base + g;
    const bool live = n < p1;
    const size_t nc = (size_t)(live ? n : p1 - 1);
    const float4 kv = ld4(src + nc * ld3 + hidden), vv = ld4(src + nc * ld3 + 2 * hidden);
    const float4 dov = ld4(dout + ((size_t)b * HW + nc) * ldo + h * LA_D + 4 * l);
    const float4 p = la_softmax8(ld4(src + nc * ld3));
    int lds0 = 0;
    asm volatile("" : "+v"(lds0));
    const float4 ks = make_float4(la_exp(kv.x - mk.x) * iz.x, la_exp(kv.y - mk.y) * iz.y, la_exp(kv.z - mk.z) * iz.z,
                                  la_exp(kv.w - mk.w) * iz.w);
    float dqs[4] = {0, 0, 0, 0}, tk[4] = {0, 0, 0, 0}, dv[4] = {0, 0, 0, 0};
#pragma unroll 2
    for (int s = 0; s < 8; ++s) {
      const float4 dos = la_from(dov, s), vs = la_from(vv, s), kss = la_from(ks, s);
      const float dov4[4] = {dos.x, dos.y, dos.z, dos.w}, vs4[4] = {vs.x, vs.y, vs.z, vs.w}, ks4[4] = {kss.x, kss.y, kss.z, kss.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = 4 * s + i;                          // (e for dqs and dK, d for dV)
        const float4 cT = *reinterpret_cast<const float4*>(sCT + lds0 + e * LA_D + 4 * l);
        const float4 dT = *reinterpret_cast<const float4*>(sDT + lds0 + e * LA_D + 4 * l);
        const float4 dd = *reinterpret_cast<const float4*>(sD + lds0 + e * LA_D + 4 * l);
        dqs[0] += cT.x * dov4[i]; dqs[1] += cT.y * dov4[i]; dqs[2] += cT.z * dov4[i]; dqs[3] += cT.w * dov4[i];
        tk[0] += dT.x * vs4[i]; tk[1] += dT.y * vs4[i]; tk[2] += dT.z * vs4[i]; tk[3] += dT.w * vs4[i];
        dv[0] += dd.x * ks4[i]; dv[1] += dd.y * ks4[i]; dv[2] += dd.z * ks4[i]; dv[3] += dd.w * ks4[i];
      }
    }
    float dot = (p.x * dqs[0] + p.y * dqs[1]) + (p.z * dqs[2] + p.w * dqs[3]);
    for (int off = 1; off <= 4; off <<= 1) dot += __shfl_xor(dot, off);
    if (!live) continue;
    float* dst = dqkv + ((size_t)b * HW + n) * ld3 + h * LA_D + 4 * l;
    st4(dst, scale * p.x * (dqs[0] - dot), scale * p.y * (dqs[1] - dot), scale * p.z * (dqs[2] - dot),
        scale * p.w * (dqs[3] - dot));
    st4(dst + hidden, ks.x * (tk[0] - rkv.x), ks.y * (tk[1] - rkv.y), ks.z * (tk[2] - rkv.z), ks.w * (tk[3] - rkv.w));
    st4(dst + 2 * hidden, dv[0], dv[1], dv[2], dv[3]);
  }
}

// ================================================================================================ host side
inline bool rms_shape_ok(int B, int H, int W, int C, int ldc) {
  return B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ldc >= C && ldc % 4 == 0;
}
}  // namespace

extern "C" int64_t ld_dn_rms_work_bytes(int B, int H, int W, int C) {
  if (!rms_shape_ok(B, H, W, C, C)) return 0;
  long ppc;
  int nchunk;
  dn_runs(B, (long)H * W, C / 4, ppc, nchunk);
  return (int64_t)B * nchunk * C * (int64_t)sizeof(double);
}

extern "C" int ld_dn_rms_forward(const float* x, const float* g, float* rinv, float* out, int B, int H, int W, int C, int ldc,
                                 void* stream) {
  LD_REQUIRE(rms_shape_ok(B, H, W, C, ldc), "ld_dn_rms_forward: B=%d H=%d W=%d C=%d ldc=%d (C and ldc >= C multiples of 4)", B, H,
             W, C, ldc);
  LD_REQUIRE(x && g && out, "ld_dn_rms_forward: null pointer");
  LD_REQUIRE(dn_aligned16(x) && dn_aligned16(g) && dn_aligned16(out), "ld_dn_rms_forward: a pointer is not 16-byte aligned");
  const long P = (long)B * H * W;
  const int L = rms_lanes(ldc);
  LD_LAUNCH(rms_forward_kernel, dim3(rms_grid(P, L)), dim3(LA_BS), 0, dn_st(stream), x, g, rinv, out, P, C, ldc, L,
            sqrtf((float)C));
  LD_LAUNCH_CHECK("dn_rms_forward");
  return LD_OK;
}

extern "C" int ld_dn_rms_backward(const float* dout, const float* x, const float* g, const float* rinv, double* work, float* dg,
                                  float* dx, int B, int H, int W, int C, int ldc, void* stream) {
  LD_REQUIRE(rms_shape_ok(B, H, W, C, ldc), "ld_dn_rms_backward: B=%d H=%d W=%d C=%d ldc=%d (C and ldc >= C multiples of 4)", B,
             H, W, C, ldc);
  LD_REQUIRE(dout && x && g && rinv && work && dg && dx, "ld_dn_rms_backward: null pointer");
  LD_REQUIRE(dn_aligned16(dout) && dn_aligned16(x) && dn_aligned16(g) && dn_aligned16(dx),
             "ld_dn_rms_backward: a pointer is not 16-byte aligned");
  const long HW = (long)H * W, P = (long)B * HW;
  hipStream_t st = dn_st(stream);
  long ppc;
  int nchunk;
  dn_runs(B, HW, C / 4, ppc, nchunk);
  LD_LAUNCH(rms_dg_kernel, dim3((unsigned)nchunk, (unsigned)((C / 4 + DN_LANES - 1) / DN_LANES), (unsigned)B), dim3(DN_BS), 0, st,
            dout, x, rinv, work, HW, C, ldc, ppc, nchunk);
  LD_LAUNCH(rms_dg_final_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, (const double*)work, dg, B * nchunk, C,
            sqrt((double)C));
  const int L = rms_lanes(ldc);                            // (after the sums: dx may overwrite dout)
  LD_LAUNCH(rms_dx_kernel, dim3(rms_grid(P, L)), dim3(LA_BS), 0, st, dout, x, g, rinv, dx, P, C, ldc, L, sqrtf((float)C));
  LD_LAUNCH_CHECK("dn_rms_backward");
  return LD_OK;
}

extern "C" int ld_dn_la_splits(int B, int heads, int H, int W) {
  if (!la_shape_ok(B, H, W, heads)) return 0;
  long ppp;
  int S;
  la_parts(B, heads, (long)H * W, ppp, S);
  return S;
}

extern "C" int64_t ld_dn_la_work_bytes(int B, int heads, int H, int W) {
  return (int64_t)B * heads * ld_dn_la_splits(B, heads, H, W) * LA_PART * (int64_t)sizeof(double);
}

extern "C" int ld_dn_la_context(const float* qkv, double* work, float* ctx, float* kstat, int B, int H, int W, int heads, int ld3,
                                void* stream) {
  LD_REQUIRE(la_shape_ok(B, H, W, heads) && la_strides_ok(heads, ld3, heads * LA_D),
             "ld_dn_la_context: B=%d H=%d W=%d heads=%d ld3=%d (heads >= 1, ld3 >= 96 heads a multiple of 4)", B, H, W, heads, ld3);
  LD_REQUIRE(qkv && work && ctx && kstat, "ld_dn_la_context: null pointer");
  LD_REQUIRE(dn_aligned16(qkv), "ld_dn_la_context: qkv is not 16-byte aligned");
  const long HW = (long)H * W;
  hipStream_t st = dn_st(stream);
  long ppp;
  int S;
  la_parts(B, heads, HW, ppp, S);
  LD_LAUNCH(la_context_kernel, dim3((unsigned)S, (unsigned)heads, (unsigned)B), dim3(LA_BS), 0, st, qkv, work, HW, heads, ld3, ppp,
            S);
  LD_LAUNCH(la_context_merge_kernel, dim3((unsigned)(B * heads)), dim3(256), 0, st, (const double*)work, ctx, kstat, S);
  LD_LAUNCH_CHECK("dn_la_context");
  return LD_OK;
}

extern "C" int ld_dn_la_out(const float* qkv, const float* ctx, float* out, int B, int H, int W, int heads, int ld3, int ldo,
                            void* stream) {
  LD_REQUIRE(la_shape_ok(B, H, W, heads) && la_strides_ok(heads, ld3, ldo),
             "ld_dn_la_out: B=%d H=%d W=%d heads=%d ld3=%d ldo=%d (heads >= 1, ld3 >= 96 heads, ldo >= 32 heads, multiples of 4)", B,
             H, W, heads, ld3, ldo);
  LD_REQUIRE(qkv && ctx && out, "ld_dn_la_out: null pointer");
  LD_REQUIRE(dn_aligned16(qkv) && dn_aligned16(ctx) && dn_aligned16(out), "ld_dn_la_out: a pointer is not 16-byte aligned");
  const long HW = (long)H * W;
  const int slots = heads + (ldo - heads * LA_D + LA_D - 1) / LA_D;
  LD_REQUIRE(slots <= 65535, "ld_dn_la_out: ldo %d", ldo);
  long run;
  unsigned nrun;
  la_runs(B, slots, HW, run, nrun);
  LD_LAUNCH(la_out_kernel, dim3(nrun, (unsigned)slots, (unsigned)B), dim3(LA_BS), 0, dn_st(stream), qkv, ctx, out, HW, heads, ld3,
            ldo, run);
  LD_LAUNCH_CHECK("dn_la_out");
  return LD_OK;
}

extern "C" int ld_dn_la_backward_reduce(const float* qkv, const float* dout, const float* ctx, double* work, float* dctx,
                                        float* rk, int B, int H, int W, int heads, int ld3, int ldo, void* stream) {
  LD_REQUIRE(la_shape_ok(B, H, W, heads) && la_strides_ok(heads, ld3, ldo),
             "ld_dn_la_backward_reduce: B=%d H=%d W=%d heads=%d ld3=%d ldo=%d (heads >= 1, ld3 >= 96 heads, ldo >= 32 heads, "
             "multiples of 4)", B, H, W, heads, ld3, ldo);
  LD_REQUIRE(qkv && dout && ctx && work && dctx && rk, "ld_dn_la_backward_reduce: null pointer");
  LD_REQUIRE(dn_aligned16(qkv) && dn_aligned16(dout), "ld_dn_la_backward_reduce: a pointer is not 16-byte aligned");
  const long HW = (long)H * W;
  hipStream_t st = dn_st(stream);
  long ppp;
  int S;
  la_parts(B, heads, HW, ppp, S);
  LD_LAUNCH(la_reduce_kernel, dim3((unsigned)S, (unsigned)heads, (unsigned)B), dim3(LA_BS), 0, st, qkv, dout, work, HW, heads, ld3,
            ldo, ppp, S);
  LD_LAUNCH(la_reduce_merge_kernel, dim3((unsigned)(B * heads)), dim3(256), 0, st, (const double*)work, ctx, dctx, rk, S);
  LD_LAUNCH_CHECK("dn_la_backward_reduce");
  return LD_OK;
}

extern "C" int ld_dn_la_backward_apply(const float* qkv, const float* dout, const float* ctx, const float* kstat,
                                       const float* dctx, const float* rk, float* dqkv, int B, int H, int W, int heads, int ld3,
                                       int ldo, void* stream) {
  LD_REQUIRE(la_shape_ok(B, H, W, heads) && la_strides_ok(heads, ld3, ldo),
             "ld_dn_la_backward_apply: B=%d H=%d W=%d heads=%d ld3=%d ldo=%d (heads >= 1, ld3 >= 96 heads, ldo >= 32 heads, "
             "multiples of 4)", B, H, W, heads, ld3, ldo);
  LD_REQUIRE(qkv && dout && ctx && kstat && dctx && rk && dqkv, "ld_dn_la_backward_apply: null pointer");
  LD_REQUIRE(dn_aligned16(qkv) && dn_aligned16(dout) && dn_aligned16(ctx) && dn_aligned16(dctx) && dn_aligned16(dqkv),
             "ld_dn_la_backward_apply: a pointer is not 16-byte aligned");
  const long HW = (long)H * W;
  const int slots = heads + (ld3 - 3 * heads * LA_D + LA_D - 1) / LA_D;
  LD_REQUIRE(slots <= 65535, "ld_dn_la_backward_apply: ld3 %d", ld3);
  long run;
  unsigned nrun;
  la_runs(B, slots, HW, run, nrun);
  LD_LAUNCH(la_apply_kernel, dim3(nrun, (unsigned)slots, (unsigned)B), dim3(LA_BS), 0, dn_st(stream), qkv, dout, ctx, kstat, dctx,
            rk, dqkv, HW, heads, ld3, ldo, run);
  LD_LAUNCH_CHECK("dn_la_backward_apply");
  return LD_OK;
}
