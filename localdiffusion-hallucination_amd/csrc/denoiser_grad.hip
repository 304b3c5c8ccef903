// Training the denoiser, first slice (backward half): the gradient of p_losses with respect to the denoiser's
// output, and what a trainable ResnetBlock (ddpm.py:170-212) needs besides the convolutions -- GroupNorm -> FiLM -> SiLU
// in training mode with its backward, and the time projection SiLU -> Linear with its backward.  The convolutions and
// their gradients are ld_pc_conv / ld_seg_wgrad / ld_seg_colsum launches (resblock.py).
//
// fp32, activations NHWC with a pixel stride `ldc` >= C (channels C..ldc-1 are padding: never read into a statistic or a
// gradient, written as zeros).  Every reduction adds in a fixed order with fp64 partial sums and no floating-point atomics,
// so a backward pass is reproducible bit for bit.  Nothing allocates.
//
// The two GroupNorm passes are memory-bound: a thread owns four consecutive channels (one 16-byte load / store per pixel)
// and a fixed set of pixels, so everything per channel -- gamma, beta, FiLM, the group's statistics -- sits in registers
// for the whole pass; a workgroup covers up to 256 channels x a run of pixels, and the pixel axis is cut into enough runs
// to fill the chip at the small maps.  The sums of a workgroup meet inside each wave first (where the lanes of a wave hold
// whole rows of pixels), then once through LDS.  sigma(a) is v_exp_f32 + v_rcp_f32 (1 ulp each): with libm's expf and an
// IEEE divide the passes would be VALU-bound, and the difference is two orders below the fp32 tolerance of the results.
//
// ld_dn_gn_forward_to16 and ld_dn_pack_nhwc_to16 (act_storage = "bf16") are the same passes writing bf16: the fp32 value is
// computed by the same code and rounded to nearest even on its way out (pack_bf16x2, what the bf16 convolutions' loaders do
// to an fp32 activation), so a convolution that reads the result computes what it computes from the fp32 tensor.
//
// The _from16 entry points (conv_out_storage = "bf16") are the four GroupNorm passes on a y that is bf16 in memory (same
// pixel stride in elements): the kernels are templates over y's type, a thread's four channels are one 8-byte load widened
// by a shift (exact: a bf16 is the upper half of an fp32), and the thread map and every sum's order are the same, so the
// results are bit for bit those of the fp32 kernels on y.float().
#include <type_traits>

#include "common.hip.h"
#include "dn_common.hip.h"

namespace {

// four consecutive channels of a bf16 activation: rounded to nearest even, one 8-byte store
__device__ __forceinline__ void st4(bf16* p, float a, float b, float c, float d) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
}

// four consecutive channels of y: fp32, or bf16 widened to the fp32 values they are
__device__ __forceinline__ float4 ld4y(const float* p) { return ld4(p); }
__device__ __forceinline__ float4 ld4y(const bf16* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}

__device__ __forceinline__ float dn_sigmoid(float a) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * a));
}

// ---------------------------------------------------------------- GroupNorm statistics (forward, pass 1)
// part [B][nchunk][C][2] = (sum, sum of squares) of each channel over the run.  TY: float or bf16 (here and below)
template <typename TY>
__global__ __launch_bounds__(DN_BS) void dn_gn_stats_kernel(const TY* __restrict__ y, double* __restrict__ part, long HW,
                                                            int C, int ldc, long ppc, int nchunk) {
  __shared__ double red[DN_BS * 8];
  const DnPos t = dn_pos(C / 4, HW, ppc);
  const int b = blockIdx.z;
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (t.active) {
    const TY* src = y + ((size_t)b * HW) * ldc + 4 * t.q;
#pragma unroll 4
    for (long p = t.p0 + t.r; p < t.p1; p += t.R) {
      const float4 x = ld4y(src + (size_t)p * ldc);
      const double x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w;
      v[0] += x0; v[1] = fma(x0, x0, v[1]);
      v[2] += x1; v[3] = fma(x1, x1, v[3]);
      v[4] += x2; v[5] = fma(x2, x2, v[5]);
      v[6] += x3; v[7] = fma(x3, x3, v[7]);
    }
  }
  if (dn_block_sum<8>(t, v, red)) {
    double* dst = part + (((size_t)b * nchunk + blockIdx.x) * C + 4 * t.q) * 2;
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = v[i];
  }
}

// stat [B][G][2] = (mean, 1 / sqrt(biased var + eps)) from the runs' sums, added in order
__global__ __launch_bounds__(256) void dn_gn_stats_final_kernel(const double* __restrict__ part, float* __restrict__ stat,
                                                                int nchunk, int C, int G, long HW) {
  extern __shared__ double sh[];                     // [C] sums, [C] sums of squares
  const int b = blockIdx.x, cpg = C / G;
  for (int c = threadIdx.x; c < C; c += 256) {
    double s = 0.0, ss = 0.0;
    for (int k = 0; k < nchunk; ++k) {
      const double* p = part + (((size_t)b * nchunk + k) * C + c) * 2;
      s += p[0];
      ss += p[1];
    }
    sh[c] = s;
    sh[C + c] = ss;
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 256) {
    double s = 0.0, ss = 0.0;
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) { s += sh[c]; ss += sh[C + c]; }
    const double n = (double)HW * cpg, mean = s / n;
    double var = ss / n - mean * mean;
    var = var > 0.0 ? var : 0.0;
    stat[((size_t)b * G + g) * 2] = (float)mean;
    stat[((size_t)b * G + g) * 2 + 1] = (float)(1.0 / sqrt(var + 1e-5));
  }
}

// What a thread keeps for its four channels: a = ((y - mean) rstd gamma + beta) (1 + s) + sh
struct DnCoef {
  float mean, rstd;
  float g[4], be[4], s1[4], sh[4];
};
__device__ __forceinline__ DnCoef dn_coef(const float* stat, const float* gamma, const float* beta, const float* film, int b,
                                          int c0, int C, int G) {
  DnCoef k;
  const int g = c0 / (C / G);
  k.mean = stat[((size_t)b * G + g) * 2];
  k.rstd = stat[((size_t)b * G + g) * 2 + 1];
  const float4 ga = ld4(gamma + c0), be = ld4(beta + c0);
  k.g[0] = ga.x; k.g[1] = ga.y; k.g[2] = ga.z; k.g[3] = ga.w;
  k.be[0] = be.x; k.be[1] = be.y; k.be[2] = be.z; k.be[3] = be.w;
#pragma unroll
  for (int i = 0; i < 4; ++i) { k.s1[i] = 1.0f; k.sh[i] = 0.0f; }
  if (film) {
    const float4 s = ld4(film + (size_t)b * 2 * C + c0), h = ld4(film + (size_t)b * 2 * C + C + c0);
    k.s1[0] = 1.0f + s.x; k.s1[1] = 1.0f + s.y; k.s1[2] = 1.0f + s.z; k.s1[3] = 1.0f + s.w;
    k.sh[0] = h.x; k.sh[1] = h.y; k.sh[2] = h.z; k.sh[3] = h.w;
  }
  return k;
}

// ---------------------------------------------------------------- forward, pass 2: out = silu(a) (+ residual)
// TO: float, or bf16 (out has the same pixel stride in elements)
template <typename TY, typename TO>
__global__ __launch_bounds__(DN_BS) void dn_gn_apply_kernel(const TY* __restrict__ y, const float* __restrict__ stat,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ film, const float* residual, TO* out,
                                                            long HW, int C, int ldc, int G, long ppc) {
  const DnPos t = dn_pos(ldc / 4, HW, ppc);
  if (!t.active) return;
  const int b = blockIdx.z, c0 = 4 * t.q;
  const size_t base = ((size_t)b * HW) * ldc + c0;
  if (c0 >= C) {                                      // padding: zeros
    for (long p = t.p0 + t.r; p < t.p1; p += t.R) st4(out + base + (size_t)p * ldc, 0.f, 0.f, 0.f, 0.f);
    return;
  }
  const DnCoef k = dn_coef(stat, gamma, beta, film, b, c0, C, G);
  for (long p = t.p0 + t.r; p < t.p1; p += t.R) {
    const size_t at = base + (size_t)p * ldc;
    const float4 x = ld4y(y + at);
    float4 rs = make_float4(0.f, 0.f, 0.f, 0.f);
    if (residual) rs = ld4(residual + at);
    const float xv[4] = {x.x, x.y, x.z, x.w}, rv[4] = {rs.x, rs.y, rs.z, rs.w};
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float a = ((xv[i] - k.mean) * k.rstd * k.g[i] + k.be[i]) * k.s1[i] + k.sh[i];
      o[i] = a * dn_sigmoid(a) + rv[i];
    }
    st4(out + at, o[0], o[1], o[2], o[3]);
  }
}

// ---------------------------------------------------------------- backward, pass 1: A = sum da, Q = sum da y^
__device__ __forceinline__ float dn_da(float dout, float a) {
  const float s = dn_sigmoid(a);
  return dout * s * (1.0f + a * (1.0f - s));
}
template <typename TY>
__global__ __launch_bounds__(DN_BS) void dn_gn_bwd_sums_kernel(const float* __restrict__ dout, const TY* __restrict__ y,
                                                               const float* __restrict__ stat, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ film,
                                                               double* __restrict__ part, long HW, int C, int ldc, int G,
                                                               long ppc, int nchunk) {
  __shared__ double red[DN_BS * 8];
  const DnPos t = dn_pos(C / 4, HW, ppc);
  const int b = blockIdx.z, c0 = 4 * t.q;
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (t.active) {
    const DnCoef k = dn_coef(stat, gamma, beta, film, b, c0, C, G);
    const size_t base = ((size_t)b * HW) * ldc + c0;
#pragma unroll 4
    for (long p = t.p0 + t.r; p < t.p1; p += t.R) {
      const size_t at = base + (size_t)p * ldc;
      const float4 x = ld4y(y + at), d = ld4(dout + at);
      const float xv[4] = {x.x, x.y, x.z, x.w}, dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float yh = (xv[i] - k.mean) * k.rstd;
        const float da = dn_da(dv[i], (yh * k.g[i] + k.be[i]) * k.s1[i] + k.sh[i]);
        v[2 * i] += (double)da;
        v[2 * i + 1] = fma((double)da, (double)yh, v[2 * i + 1]);
      }
    }
  }
  if (dn_block_sum<8>(t, v, red)) {
    double* dst = part + (((size_t)b * nchunk + blockIdx.x) * C + c0) * 2;
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = v[i];
  }
}

// The finalisation of one sample: dfilm, S [B][C][2] = (1 + s) (A, Q) and m [B][G][2] = the group means of gamma S.
__global__ __launch_bounds__(256) void dn_gn_bwd_final_kernel(const double* __restrict__ part, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ film,
                                                              float* __restrict__ dfilm, double* __restrict__ S,
                                                              double* __restrict__ m, int nchunk, int C, int G, long HW) {
  extern __shared__ double sh[];                     // [C] gamma S1, [C] gamma S2
  const int b = blockIdx.x, cpg = C / G;
  for (int c = threadIdx.x; c < C; c += 256) {
    double A = 0.0, Q = 0.0;
    for (int k = 0; k < nchunk; ++k) {
      const double* p = part + (((size_t)b * nchunk + k) * C + c) * 2;
      A += p[0];
      Q += p[1];
    }
    const double ga = gamma[c], be = beta[c];
    double s1 = 1.0;
    if (film) {
      s1 = (double)(1.0f + film[(size_t)b * 2 * C + c]);
      dfilm[(size_t)b * 2 * C + c] = (float)(ga * Q + be * A);
      dfilm[(size_t)b * 2 * C + C + c] = (float)A;
    }
    const double S1 = s1 * A, S2 = s1 * Q;
    S[((size_t)b * C + c) * 2] = S1;
    S[((size_t)b * C + c) * 2 + 1] = S2;
    sh[c] = ga * S1;
    sh[C + c] = ga * S2;
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 256) {
    double a = 0.0, q = 0.0;
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) { a += sh[c]; q += sh[C + c]; }
    const double n = (double)HW * cpg;
    m[((size_t)b * G + g) * 2] = a / n;
    m[((size_t)b * G + g) * 2 + 1] = q / n;
  }
}

// ---------------------------------------------------------------- backward, pass 2: dy = rstd (gamma (1 + s) da - m1 - y^ m2)
// The workgroups of run 0 of sample 0 also add S over the batch, in order: dbeta, dgamma.  dy may be dout.
template <typename TY>
__global__ __launch_bounds__(DN_BS) void dn_gn_dy_kernel(const float* dout, const TY* __restrict__ y,
                                                         const float* __restrict__ stat, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ film,
                                                         const double* __restrict__ S, const double* __restrict__ m,
                                                         float* __restrict__ dgamma, float* __restrict__ dbeta, float* dy, int B,
                                                         long HW, int C, int ldc, int G, long ppc) {
  const DnPos t = dn_pos(ldc / 4, HW, ppc);
  if (!t.active) return;
  const int b = blockIdx.z, c0 = 4 * t.q;
  const size_t base = ((size_t)b * HW) * ldc + c0;
  if (c0 >= C) {
    for (long p = t.p0 + t.r; p < t.p1; p += t.R) st4(dy + base + (size_t)p * ldc, 0.f, 0.f, 0.f, 0.f);
    return;
  }
  if (blockIdx.x == 0 && b == 0 && t.r == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double db = 0.0, dg = 0.0;
      for (int bb = 0; bb < B; ++bb) {
        db += S[((size_t)bb * C + c0 + i) * 2];
        dg += S[((size_t)bb * C + c0 + i) * 2 + 1];
      }
      dbeta[c0 + i] = (float)db;
      dgamma[c0 + i] = (float)dg;
    }
  }
  const DnCoef k = dn_coef(stat, gamma, beta, film, b, c0, C, G);
  const int g = c0 / (C / G);
  const float m1 = k.rstd * (float)m[((size_t)b * G + g) * 2], m2 = k.rstd * (float)m[((size_t)b * G + g) * 2 + 1];
  float kd[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) kd[i] = k.rstd * k.g[i] * k.s1[i];
  for (long p = t.p0 + t.r; p < t.p1; p += t.R) {
    const size_t at = base + (size_t)p * ldc;
    const float4 x = ld4y(y + at), d = ld4(dout + at);
    const float xv[4] = {x.x, x.y, x.z, x.w}, dv[4] = {d.x, d.y, d.z, d.w};
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float yh = (xv[i] - k.mean) * k.rstd;
      const float da = dn_da(dv[i], (yh * k.g[i] + k.be[i]) * k.s1[i] + k.sh[i]);
      o[i] = kd[i] * da - m1 - yh * m2;
    }
    st4(dy + at, o[0], o[1], o[2], o[3]);
  }
}

// ---------------------------------------------------------------- column sums (bias gradients)
// part [B][nchunk][C] = the sum of each channel over the run; out [C] = the runs added in (b, run) order, four contiguous
// quarters of that order at a time
__global__ __launch_bounds__(DN_BS) void dn_colsum_kernel(const float* __restrict__ x, double* __restrict__ part, long HW,
                                                          int C, int ldc, long ppc, int nchunk) {
  __shared__ double red[DN_BS * 4];
  const DnPos t = dn_pos(C / 4, HW, ppc);
  const int b = blockIdx.z;
  double v[4] = {0, 0, 0, 0};
  if (t.active) {
    const float* src = x + ((size_t)b * HW) * ldc + 4 * t.q;
#pragma unroll 4
    for (long p = t.p0 + t.r; p < t.p1; p += t.R) {
      const float4 a = ld4(src + (size_t)p * ldc);
      v[0] += (double)a.x; v[1] += (double)a.y; v[2] += (double)a.z; v[3] += (double)a.w;
    }
  }
  if (dn_block_sum<4>(t, v, red)) {
    double* dst = part + ((size_t)b * nchunk + blockIdx.x) * C + 4 * t.q;
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[i] = v[i];
  }
}
__global__ __launch_bounds__(256) void dn_colsum_final_kernel(const double* __restrict__ part, float* __restrict__ out, int n,
                                                              int C) {
  __shared__ double red[256];
  const int cl = (int)threadIdx.x & 63, j = (int)threadIdx.x >> 6, c = (int)blockIdx.x * 64 + cl;
  const int per = (n + 3) / 4, k0 = j * per, k1 = k0 + per < n ? k0 + per : n;
  double acc = 0.0;
  if (c < C) {
#pragma unroll 8
    for (int k = k0; k < k1; ++k) acc += part[(size_t)k * C + c];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (j == 0 && c < C) out[c] = (float)(((red[cl] + red[64 + cl]) + red[128 + cl]) + red[192 + cl]);
}

// ---------------------------------------------------------------- the time projection: SiLU -> Linear(T, N)
__device__ __forceinline__ double dn_wave_sum_d(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// one wave per output feature j: film[b][j] = sum_k silu(temb[b][k]) w[j][k] + bias[j]
__global__ __launch_bounds__(256) void dn_time_proj_kernel(const float* __restrict__ temb, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ film, int B,
                                                           int T, int N) {
  const int j = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  if (j >= N) return;                                 // (whole waves)
  for (int b = 0; b < B; ++b) {
    double acc = 0.0;
    for (int k = lane; k < T; k += 64) {
      const float e = temb[(size_t)b * T + k];
      acc = fma((double)(e * dn_sigmoid(e)), (double)w[(size_t)j * T + k], acc);
    }
    acc = dn_wave_sum_d(acc);
    if (lane == 0) film[(size_t)b * N + j] = (float)(acc + (double)bias[j]);
  }
}
// One launch, three kinds of workgroups: dw [N][T] = dfilm^T silu(temb) (an element per thread), dtemb [B][T] = (dfilm w)
// silu'(temb) (an element per thread), db [N] = sum_b dfilm.
__global__ __launch_bounds__(256) void dn_time_proj_bwd_kernel(const float* __restrict__ dfilm, const float* __restrict__ temb,
                                                               const float* __restrict__ w, float* __restrict__ dw,
                                                               float* __restrict__ db, float* __restrict__ dtemb, int B, int T,
                                                               int N, int wg_dw, int wg_dt) {
  int wg = blockIdx.x;
  if (wg < wg_dw) {
    const long i = (long)wg * 256 + threadIdx.x;
    if (i >= (long)N * T) return;
    const int j = (int)(i / T), k = (int)(i - (long)j * T);
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
      const float e = temb[(size_t)b * T + k];
      acc = fma((double)dfilm[(size_t)b * N + j], (double)(e * dn_sigmoid(e)), acc);
    }
    dw[i] = (float)acc;
    return;
  }
  wg -= wg_dw;
  if (wg < wg_dt) {
    const long i = (long)wg * 256 + threadIdx.x;
    if (i >= (long)B * T) return;
    const int b = (int)(i / T), k = (int)(i - (long)b * T);
    double acc = 0.0;
#pragma unroll 8                                    // (eight independent loads in flight; the additions keep their order)
    for (int j = 0; j < N; ++j) acc = fma((double)dfilm[(size_t)b * N + j], (double)w[(size_t)j * T + k], acc);
    const float e = temb[i], s = dn_sigmoid(e);
    dtemb[i] = (float)acc * (s * (1.0f + e * (1.0f - s)));
    return;
  }
  wg -= wg_dt;
  const int j = wg * 256 + (int)threadIdx.x;
  if (j >= N) return;
  double acc = 0.0;
  for (int b = 0; b < B; ++b) acc += (double)dfilm[(size_t)b * N + j];
  db[j] = (float)acc;
}

// ---------------------------------------------------------------- layouts
// out [B, H, W, ldc] (channels C..ldc-1 zero) from a tensor [B, C, H, W] of any strides
__device__ __forceinline__ float dn_nchw_at(const float* __restrict__ x, long i, int C, int H, int W, long sb, long sc, long sh,
                                            long sw, int ldc) {
  const int c = (int)(i % ldc);
  long p = i / ldc;
  const int xx = (int)(p % W);
  p /= W;
  const int yy = (int)(p % H);
  const long b = p / H;
  return c < C ? x[b * sb + c * sc + yy * sh + xx * sw] : 0.0f;
}
__global__ __launch_bounds__(256) void dn_pack_nhwc_kernel(const float* __restrict__ x, float* __restrict__ out, long n, int C,
                                                           int H, int W, long sb, long sc, long sh, long sw, int ldc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = dn_nchw_at(x, i, C, H, W, sb, sc, sh, sw, ldc);
}
// the same in bf16: one thread per pair of neighbouring channels (ldc even), n the number of pairs
__global__ __launch_bounds__(256) void dn_pack_nhwc_to16_kernel(const float* __restrict__ x, unsigned* __restrict__ out, long n,
                                                                int C, int H, int W, long sb, long sc, long sh, long sw, int ldc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = pack_bf16x2(dn_nchw_at(x, 2 * i, C, H, W, sb, sc, sh, sw, ldc), dn_nchw_at(x, 2 * i + 1, C, H, W, sb, sc, sh, sw, ldc));
}
// out [d0][d1][d2] (contiguous) from in[off + i0 s0 + i1 s1 + i2 s2]: ld_seg_permute3's inverse
__global__ __launch_bounds__(256) void dn_gather3_kernel(const float* __restrict__ in, float* __restrict__ out, long n, int d1,
                                                         int d2, long off, long s0, long s1, long s2) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int i2 = (int)(i % d2);
  const long r = i / d2;
  const int i1 = (int)(r % d1);
  const long i0 = r / d1;
  out[i] = in[off + i0 * s0 + i1 * s1 + i2 * s2];
}

// ---------------------------------------------------------------- the loss gradient
// With a trailing `const float* dev_scale` (ld_p_losses_grad_scaled) the upstream scalar is g * *dev_scale, the loss scale
// read on the device (a power of two by default, so the product is exact); without, the kernel is what it always was
template <typename... Scale>
__global__ __launch_bounds__(256) void dn_p_losses_grad_kernel(const float* __restrict__ mo, const float* __restrict__ x0,
                                                               const float* __restrict__ z, const int* __restrict__ t,
                                                               const float* __restrict__ sab, const float* __restrict__ s1mab,
                                                               const float* __restrict__ lw, float g, float* __restrict__ out,
                                                               long per, int B, int objective, Scale... dev_scale) {
  if constexpr (sizeof...(Scale) != 0) g = g * *(dev_scale, ...);
  const int b = blockIdx.y;
  const int tb = t[b];
  const float a = sab[tb], c = s1mab[tb];
  const float k = (float)((double)g * 2.0 * (double)lw[tb] / ((double)B * (double)per));
  const long base = (long)b * per;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
    const float xs = x0[base + i], nz = z[base + i];
    const float target = objective == LD_OBJ_NOISE ? nz : (objective == LD_OBJ_X0 ? xs : a * nz - c * xs);
    out[base + i] = k * (mo[base + i] - target);
  }
}

inline bool dn_gn_shape_ok(int B, int H, int W, int C, int ldc, int G) {
  return B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0 && G > 0 && C % G == 0 && (C / G) % 4 == 0 && ldc >= C && ldc % 4 == 0 &&
         C <= 4096 && ldc <= 4096;      // (the finalisations keep 2 C doubles in LDS)
}
}  // namespace

namespace {
int dn_p_losses_grad(const char* name, bool scaled, const float* model_out, const float* x_start, const float* noise, const int* t,
                     const float* sqrt_ab, const float* sqrt_1mab, const float* loss_weight, float g, const float* dev_scale,
                     float* d_model_out, int B, int64_t elems_per_sample, int objective, void* stream) {
  LD_REQUIRE(model_out && x_start && noise && t && sqrt_ab && sqrt_1mab && loss_weight && d_model_out && (dev_scale || !scaled),
             "%s: null pointer", name);
  LD_REQUIRE(B > 0 && B <= 65535 && elems_per_sample > 0, "%s: batch %d (1..65535) of %ld elements", name, B,
             (long)elems_per_sample);
  LD_REQUIRE(objective == LD_OBJ_X0 || objective == LD_OBJ_NOISE || objective == LD_OBJ_V, "%s: objective %d", name, objective);
  long wgs = ((long)elems_per_sample + 255) / 256;
  if (wgs > 1024) wgs = 1024;
  const dim3 grid((unsigned)wgs, (unsigned)B);
  if (scaled) {
    LD_LAUNCH(dn_p_losses_grad_kernel<const float*>, grid, dim3(256), 0, dn_st(stream), model_out, x_start, noise, t, sqrt_ab, sqrt_1mab,
              loss_weight, g, d_model_out, (long)elems_per_sample, B, objective, dev_scale);
  } else {
    LD_LAUNCH(dn_p_losses_grad_kernel<>, grid, dim3(256), 0, dn_st(stream), model_out, x_start, noise, t, sqrt_ab, sqrt_1mab,
              loss_weight, g, d_model_out, (long)elems_per_sample, B, objective);
  }
  LD_LAUNCH_CHECK(name + 3);
  return LD_OK;
}
}  // namespace

extern "C" int ld_p_losses_grad(const float* model_out, const float* x_start, const float* noise, const int* t,
                                const float* sqrt_ab, const float* sqrt_1mab, const float* loss_weight, float g,
                                float* d_model_out, int B, int64_t elems_per_sample, int objective, void* stream) {
  return dn_p_losses_grad("ld_p_losses_grad", false, model_out, x_start, noise, t, sqrt_ab, sqrt_1mab, loss_weight, g, nullptr,
                          d_model_out, B, elems_per_sample, objective, stream);
}

extern "C" int ld_p_losses_grad_scaled(const float* model_out, const float* x_start, const float* noise, const int* t,
                                       const float* sqrt_ab, const float* sqrt_1mab, const float* loss_weight, float g,
                                       const float* dev_scale, float* d_model_out, int B, int64_t elems_per_sample, int objective,
                                       void* stream) {
  return dn_p_losses_grad("ld_p_losses_grad_scaled", true, model_out, x_start, noise, t, sqrt_ab, sqrt_1mab, loss_weight, g,
                          dev_scale, d_model_out, B, elems_per_sample, objective, stream);
}

extern "C" int64_t ld_dn_gn_work_bytes(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4) return 0;
  long ppc;
  int nchunk;
  dn_runs(B, (long)H * W, C / 4, ppc, nchunk);
  return (int64_t)B * (nchunk + 2) * C * 2 * (int64_t)sizeof(double);
}

namespace {
// ld_dn_gn_forward (TY = TO = float), ld_dn_gn_forward_to16 (TO = bf16) and the two _from16 forms (TY = bf16)
template <typename TY, typename TO>
int dn_gn_forward(const char* name, const TY* y, const float* gamma, const float* beta, const float* film, const float* residual,
                  double* work, float* stat, TO* out, int B, int H, int W, int C, int ldc, int groups, void* stream) {
  LD_REQUIRE(dn_gn_shape_ok(B, H, W, C, ldc, groups),
             "%s: B=%d H=%d W=%d C=%d ldc=%d groups=%d (C a multiple of 4 * groups, ldc >= C a multiple of 4)", name, B, H, W, C,
             ldc, groups);
  LD_REQUIRE(y && gamma && beta && work && stat && out, "%s: null pointer", name);
  LD_REQUIRE(dn_aligned16(y) && dn_aligned16(gamma) && dn_aligned16(beta) && dn_aligned16(film) && dn_aligned16(residual) &&
                 dn_aligned16(out), "%s: a pointer is not 16-byte aligned", name);
  LD_REQUIRE((std::is_same<TO, float>::value) || static_cast<const void*>(residual) != static_cast<const void*>(out),
             "%s: residual (fp32) cannot alias out (bf16)", name);
  const long HW = (long)H * W;
  hipStream_t st = dn_st(stream);
  long ppc;
  int nchunk;
  dn_runs(B, HW, C / 4, ppc, nchunk);
  LD_LAUNCH(dn_gn_stats_kernel<TY>, dim3((unsigned)nchunk, (unsigned)((C / 4 + DN_LANES - 1) / DN_LANES), (unsigned)B), dim3(DN_BS), 0,
            st, y, work, HW, C, ldc, ppc, nchunk);
  LD_LAUNCH(dn_gn_stats_final_kernel, dim3((unsigned)B), dim3(256), 2 * (size_t)C * sizeof(double), st, (const double*)work, stat,
            nchunk, C, groups, HW);
  long ppa;
  int na;
  dn_runs(B, HW, ldc / 4, ppa, na);
  LD_LAUNCH((dn_gn_apply_kernel<TY, TO>), dim3((unsigned)na, (unsigned)((ldc / 4 + DN_LANES - 1) / DN_LANES), (unsigned)B), dim3(DN_BS),
            0, st, y, (const float*)stat, gamma, beta, film, residual, out, HW, C, ldc, groups, ppa);
  LD_LAUNCH_CHECK(name + 3);
  return LD_OK;
}
}  // namespace

extern "C" int ld_dn_gn_forward(const float* y, const float* gamma, const float* beta, const float* film, const float* residual,
                                double* work, float* stat, float* out, int B, int H, int W, int C, int ldc, int groups,
                                void* stream) {
  return dn_gn_forward<float, float>("ld_dn_gn_forward", y, gamma, beta, film, residual, work, stat, out, B, H, W, C, ldc, groups, stream);
}

extern "C" int ld_dn_gn_forward_to16(const float* y, const float* gamma, const float* beta, const float* film,
                                     const float* residual, double* work, float* stat, void* out_bf16, int B, int H, int W, int C,
                                     int ldc, int groups, void* stream) {
  return dn_gn_forward<float, bf16>("ld_dn_gn_forward_to16", y, gamma, beta, film, residual, work, stat,
                                    static_cast<bf16*>(out_bf16), B, H, W, C, ldc, groups, stream);
}

extern "C" int ld_dn_gn_forward_from16(const void* y_bf16, const float* gamma, const float* beta, const float* film,
                                       const float* residual, double* work, float* stat, float* out, int B, int H, int W, int C,
                                       int ldc, int groups, void* stream) {
  return dn_gn_forward<bf16, float>("ld_dn_gn_forward_from16", static_cast<const bf16*>(y_bf16), gamma, beta, film, residual, work,
                                    stat, out, B, H, W, C, ldc, groups, stream);
}

extern "C" int ld_dn_gn_forward_from16_to16(const void* y_bf16, const float* gamma, const float* beta, const float* film,
                                            const float* residual, double* work, float* stat, void* out_bf16, int B, int H, int W,
                                            int C, int ldc, int groups, void* stream) {
  return dn_gn_forward<bf16, bf16>("ld_dn_gn_forward_from16_to16", static_cast<const bf16*>(y_bf16), gamma, beta, film, residual,
                                   work, stat, static_cast<bf16*>(out_bf16), B, H, W, C, ldc, groups, stream);
}

namespace {
// ld_dn_gn_backward (TY = float) and ld_dn_gn_backward_from16 (TY = bf16)
template <typename TY>
int dn_gn_backward(const char* name, const float* dout, const TY* y, const float* stat, const float* gamma, const float* beta,
                   const float* film, double* work, float* dgamma, float* dbeta, float* dfilm, float* dy, int B, int H, int W, int C,
                   int ldc, int groups, void* stream) {
  LD_REQUIRE(dn_gn_shape_ok(B, H, W, C, ldc, groups),
             "%s: B=%d H=%d W=%d C=%d ldc=%d groups=%d (C a multiple of 4 * groups, ldc >= C a multiple of 4)", name, B, H, W, C,
             ldc, groups);
  LD_REQUIRE(dout && y && stat && gamma && beta && work && dgamma && dbeta && dy, "%s: null pointer", name);
  LD_REQUIRE((film == nullptr) == (dfilm == nullptr), "%s: film and dfilm go together", name);
  LD_REQUIRE(dn_aligned16(dout) && dn_aligned16(y) && dn_aligned16(gamma) && dn_aligned16(beta) && dn_aligned16(film) &&
                 dn_aligned16(dy), "%s: a pointer is not 16-byte aligned", name);
  const long HW = (long)H * W;
  hipStream_t st = dn_st(stream);
  long ppc;
  int nchunk;
  dn_runs(B, HW, C / 4, ppc, nchunk);
  double* S = work + (size_t)B * nchunk * C * 2;
  double* m = S + (size_t)B * C * 2;
  LD_LAUNCH(dn_gn_bwd_sums_kernel<TY>, dim3((unsigned)nchunk, (unsigned)((C / 4 + DN_LANES - 1) / DN_LANES), (unsigned)B), dim3(DN_BS),
            0, st, dout, y, stat, gamma, beta, film, work, HW, C, ldc, groups, ppc, nchunk);
  LD_LAUNCH(dn_gn_bwd_final_kernel, dim3((unsigned)B), dim3(256), 2 * (size_t)C * sizeof(double), st, (const double*)work, gamma,
            beta, film, dfilm, S, m, nchunk, C, groups, HW);
  long ppa;
  int na;
  dn_runs(B, HW, ldc / 4, ppa, na);
  LD_LAUNCH(dn_gn_dy_kernel<TY>, dim3((unsigned)na, (unsigned)((ldc / 4 + DN_LANES - 1) / DN_LANES), (unsigned)B), dim3(DN_BS), 0, st,
            dout, y, stat, gamma, beta, film, (const double*)S, (const double*)m, dgamma, dbeta, dy, B, HW, C, ldc, groups, ppa);
  LD_LAUNCH_CHECK(name + 3);
  return LD_OK;
}
}  // namespace

extern "C" int ld_dn_gn_backward(const float* dout, const float* y, const float* stat, const float* gamma, const float* beta,
                                 const float* film, double* work, float* dgamma, float* dbeta, float* dfilm, float* dy, int B,
                                 int H, int W, int C, int ldc, int groups, void* stream) {
  return dn_gn_backward<float>("ld_dn_gn_backward", dout, y, stat, gamma, beta, film, work, dgamma, dbeta, dfilm, dy, B, H, W, C, ldc,
                               groups, stream);
}

extern "C" int ld_dn_gn_backward_from16(const float* dout, const void* y_bf16, const float* stat, const float* gamma,
                                        const float* beta, const float* film, double* work, float* dgamma, float* dbeta,
                                        float* dfilm, float* dy, int B, int H, int W, int C, int ldc, int groups, void* stream) {
  return dn_gn_backward<bf16>("ld_dn_gn_backward_from16", dout, static_cast<const bf16*>(y_bf16), stat, gamma, beta, film, work,
                              dgamma, dbeta, dfilm, dy, B, H, W, C, ldc, groups, stream);
}

extern "C" int ld_dn_colsum(const float* x, double* work, float* out, int B, int H, int W, int C, int ldc, void* stream) {
  LD_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ldc >= C && ldc % 4 == 0,
             "ld_dn_colsum: B=%d H=%d W=%d C=%d ldc=%d (C and ldc >= C multiples of 4)", B, H, W, C, ldc);
  LD_REQUIRE(x && work && out, "ld_dn_colsum: null pointer");
  LD_REQUIRE(dn_aligned16(x), "ld_dn_colsum: x is not 16-byte aligned");
  const long HW = (long)H * W;
  hipStream_t st = dn_st(stream);
  long ppc;
  int nchunk;
  dn_runs(B, HW, C / 4, ppc, nchunk);
  LD_LAUNCH(dn_colsum_kernel, dim3((unsigned)nchunk, (unsigned)((C / 4 + DN_LANES - 1) / DN_LANES), (unsigned)B), dim3(DN_BS), 0,
            st, x, work, HW, C, ldc, ppc, nchunk);
  LD_LAUNCH(dn_colsum_final_kernel, dim3((unsigned)((C + 63) / 64)), dim3(256), 0, st, (const double*)work, out, B * nchunk, C);
  LD_LAUNCH_CHECK("dn_colsum");
  return LD_OK;
}

extern "C" int ld_dn_time_proj(const float* temb, const float* w, const float* bias, float* film, int B, int T, int N,
                               void* stream) {
  LD_REQUIRE(B > 0 && T > 0 && N > 0, "ld_dn_time_proj: shape B=%d T=%d N=%d", B, T, N);
  LD_REQUIRE(temb && w && bias && film, "ld_dn_time_proj: null pointer");
  LD_LAUNCH(dn_time_proj_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, dn_st(stream), temb, w, bias, film, B, T, N);
  LD_LAUNCH_CHECK("dn_time_proj");
  return LD_OK;
}

extern "C" int ld_dn_time_proj_backward(const float* dfilm, const float* temb, const float* w, float* dw, float* db, float* dtemb,
                                        int B, int T, int N, void* stream) {
  LD_REQUIRE(B > 0 && T > 0 && N > 0, "ld_dn_time_proj_backward: shape B=%d T=%d N=%d", B, T, N);
  LD_REQUIRE(dfilm && temb && w && dw && db && dtemb, "ld_dn_time_proj_backward: null pointer");
  const long wg_dw = ((long)N * T + 255) / 256, wg_dt = ((long)B * T + 255) / 256, wg_db = (N + 255) / 256;
  LD_REQUIRE(wg_dw + wg_dt + wg_db < (1L << 31), "ld_dn_time_proj_backward: %ld x %d weights", (long)N, T);
  LD_LAUNCH(dn_time_proj_bwd_kernel, dim3((unsigned)(wg_dw + wg_dt + wg_db)), dim3(256), 0, dn_st(stream), dfilm, temb, w, dw, db,
            dtemb, B, T, N, (int)wg_dw, (int)wg_dt);
  LD_LAUNCH_CHECK("dn_time_proj_backward");
  return LD_OK;
}

extern "C" int ld_dn_pack_nhwc(const float* x, float* out, int B, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh,
                               int64_t sw, int ldc, void* stream) {
  LD_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && ldc >= C, "ld_dn_pack_nhwc: shape B=%d C=%d H=%d W=%d ldc=%d", B, C, H, W, ldc);
  LD_REQUIRE(sb >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "ld_dn_pack_nhwc: negative stride");
  LD_REQUIRE(x && out, "ld_dn_pack_nhwc: null pointer");
  const long n = (long)B * H * W * ldc;
  LD_REQUIRE((n + 255) / 256 < (1L << 31), "ld_dn_pack_nhwc: %ld elements", n);
  LD_LAUNCH(dn_pack_nhwc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dn_st(stream), x, out, n, C, H, W, (long)sb,
            (long)sc, (long)sh, (long)sw, ldc);
  LD_LAUNCH_CHECK("dn_pack_nhwc");
  return LD_OK;
}

extern "C" int ld_dn_pack_nhwc_to16(const float* x, void* out_bf16, int B, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh,
                                    int64_t sw, int ldc, void* stream) {
  LD_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && ldc >= C, "ld_dn_pack_nhwc_to16: shape B=%d C=%d H=%d W=%d ldc=%d", B, C, H, W,
             ldc);
  LD_REQUIRE(ldc % 2 == 0, "ld_dn_pack_nhwc_to16: ldc %d (even)", ldc);
  LD_REQUIRE(sb >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "ld_dn_pack_nhwc_to16: negative stride");
  LD_REQUIRE(x && out_bf16, "ld_dn_pack_nhwc_to16: null pointer");
  LD_REQUIRE(reinterpret_cast<uintptr_t>(out_bf16) % 4 == 0, "ld_dn_pack_nhwc_to16: out must be 4-byte aligned");
  const long n = (long)B * H * W * ldc / 2;
  LD_REQUIRE((n + 255) / 256 < (1L << 31), "ld_dn_pack_nhwc_to16: %ld elements", 2 * n);
  LD_LAUNCH(dn_pack_nhwc_to16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dn_st(stream), x,
            static_cast<unsigned*>(out_bf16), n, C, H, W, (long)sb, (long)sc, (long)sh, (long)sw, ldc);
  LD_LAUNCH_CHECK("dn_pack_nhwc_to16");
  return LD_OK;
}

extern "C" int ld_dn_gather3(const float* in, float* out, int d0, int d1, int d2, int64_t off, int64_t s0, int64_t s1, int64_t s2,
                             void* stream) {
  LD_REQUIRE(d0 > 0 && d1 > 0 && d2 > 0, "ld_dn_gather3: shape %d x %d x %d", d0, d1, d2);
  LD_REQUIRE(off >= 0 && s0 >= 0 && s1 >= 0 && s2 >= 0, "ld_dn_gather3: negative offset or stride");
  LD_REQUIRE(in && out, "ld_dn_gather3: null pointer");
  const long n = (long)d0 * d1 * d2;
  LD_REQUIRE((n + 255) / 256 < (1L << 31), "ld_dn_gather3: %ld elements", n);
  LD_LAUNCH(dn_gather3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dn_st(stream), in, out, n, d1, d2, (long)off,
            (long)s0, (long)s1, (long)s2);
  LD_LAUNCH_CHECK("dn_gather3");
  return LD_OK;
}
