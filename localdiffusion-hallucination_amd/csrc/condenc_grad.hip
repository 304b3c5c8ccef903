// Training the denoiser, fifth slice: what a trainable BasicBlock of the ResUnet condition encoder (unet_model.py:8-51) needs
// besides ld_pc_conv / ld_seg_wgrad / ld_dn_colsum / ld_seg_pool -- GroupNorm in training mode at any even number of
// channels per group (16 groups of 2 at 32 channels), followed by ReLU or nothing, of one tensor or of the sum of two
// normalised tensors (the block's tail relu(GN_a(y) + GN_b(y2))), with its backward; and the im2col that turns a 3 x 3
// convolution on 1..4 image channels into a 1 x 1 convolution.
//
// fp32, activations NHWC with a pixel stride `ldc` >= C: channels C..ldc-1 are padding, never read into a statistic or a
// gradient and written as zeros.  The passes have ld_dn_gn_forward / ld_dn_gn_backward's structure (dn_common.hip.h): a
// thread owns four consecutive channels and a fixed set of pixels of its workgroup's run, a workgroup's fp64 sums meet in a
// fixed order, the runs are merged in index order by a small second launch.  No atomics, nothing allocates, every entry
// point checks its arguments before it launches.
//
// What differs from the SiLU / FiLM kernels: a thread's four channels are two PAIRS, each pair in one group (channels per
// group is even, and a pair starts at an even channel), so a thread keeps two (mean, rstd) instead of one; the backward takes
// the ReLU mask from the saved result (out > 0, ld_seg_bn_backward's rule) instead of recomputing the pre-activation; and the
// two-operand form shares that masked gradient between both GroupNorms: one pass gathers sum g, sum g y^, sum g y2^.
#include "common.hip.h"
#include "dn_common.hip.h"

namespace {

// What a thread keeps of one GroupNorm for its four channels: a = (y - mean) rstd gamma + beta, the statistics per pair
struct CeCoef {
  float mean[2], rstd[2];
  float g[4], be[4];
};
__device__ __forceinline__ CeCoef ce_coef(const float* stat, const float* gamma, const float* beta, int b, int c0, int cpg,
                                          int G) {
  CeCoef k;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int g = (c0 + 2 * h) / cpg;
    k.mean[h] = stat[((size_t)b * G + g) * 2];
    k.rstd[h] = stat[((size_t)b * G + g) * 2 + 1];
  }
  const float4 ga = ld4(gamma + c0);
  k.g[0] = ga.x; k.g[1] = ga.y; k.g[2] = ga.z; k.g[3] = ga.w;
#pragma unroll
  for (int i = 0; i < 4; ++i) k.be[i] = 0.0f;
  if (beta) {
    const float4 be = ld4(beta + c0);
    k.be[0] = be.x; k.be[1] = be.y; k.be[2] = be.z; k.be[3] = be.w;
  }
  return k;
}

// ---------------------------------------------------------------- statistics (forward, pass 1)
// part [NOP][B][nchunk][C][2] = (sum, sum of squares) of each channel over the run; blockIdx.z = op B + b
__global__ __launch_bounds__(DN_BS) void ce_gn_stats_kernel(const float* __restrict__ y, const float* __restrict__ y2,
                                                            double* __restrict__ part, int B, long HW, int C, int ldc, long ppc,
                                                            int nchunk) {
  __shared__ double red[DN_BS * 8];
  const DnPos t = dn_pos(C / 4, HW, ppc);
  const int op = (int)blockIdx.z / B, b = (int)blockIdx.z - op * B;
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (t.active) {
    const float* src = (op ? y2 : y) + ((size_t)b * HW) * ldc + 4 * t.q;
#pragma unroll 4
    for (long p = t.p0 + t.r; p < t.p1; p += t.R) {
      const float4 x = ld4(src + (size_t)p * ldc);
      const double x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w;
      v[0] += x0; v[1] = fma(x0, x0, v[1]);
      v[2] += x1; v[3] = fma(x1, x1, v[3]);
      v[4] += x2; v[5] = fma(x2, x2, v[5]);
      v[6] += x3; v[7] = fma(x3, x3, v[7]);
    }
  }
  if (dn_block_sum<8>(t, v, red)) {
    double* dst = part + ((((size_t)op * B + b) * nchunk + blockIdx.x) * C + 4 * t.q) * 2;
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = v[i];
  }
}

// stat [B][G][2] = (mean, 1 / sqrt(biased var + 1e-5)) from the runs' sums, added in order; blockIdx.y = op
__global__ __launch_bounds__(256) void ce_gn_stats_final_kernel(const double* __restrict__ part, float* __restrict__ stat,
                                                                float* __restrict__ stat2, int B, int nchunk, int C, int G,
                                                                long HW) {
  extern __shared__ double sh[];                     // [C] sums, [C] sums of squares
  const int b = blockIdx.x, op = blockIdx.y, cpg = C / G;
  const double* src = part + ((size_t)op * B + b) * nchunk * C * 2;
  float* dst = op ? stat2 : stat;
  for (int c = threadIdx.x; c < C; c += 256) {
    double s = 0.0, ss = 0.0;
    for (int k = 0; k < nchunk; ++k) {
      const double* p = src + ((size_t)k * C + c) * 2;
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
    dst[((size_t)b * G + g) * 2] = (float)mean;
    dst[((size_t)b * G + g) * 2 + 1] = (float)(1.0 / sqrt(var + 1e-5));
  }
}

// ---------------------------------------------------------------- forward, pass 2: out = act(a (+ a2))
template <int NOP>
__global__ __launch_bounds__(DN_BS) void ce_gn_apply_kernel(const float* __restrict__ y, const float* __restrict__ stat,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ y2, const float* __restrict__ stat2,
                                                            const float* __restrict__ gamma2, const float* __restrict__ beta2,
                                                            float* __restrict__ out, long HW, int C, int ldc, int G, int relu,
                                                            long ppc) {
  const DnPos t = dn_pos(ldc / 4, HW, ppc);
  if (!t.active) return;
  const int b = blockIdx.z, c0 = 4 * t.q;
  const size_t base = ((size_t)b * HW) * ldc + c0;
  if (c0 >= C) {                                      // padding: zeros
    for (long p = t.p0 + t.r; p < t.p1; p += t.R) st4(out + base + (size_t)p * ldc, 0.f, 0.f, 0.f, 0.f);
    return;
  }
  const CeCoef k = ce_coef(stat, gamma, beta, b, c0, C / G, G);
  CeCoef k2 = k;
  if (NOP == 2) k2 = ce_coef(stat2, gamma2, beta2, b, c0, C / G, G);
  for (long p = t.p0 + t.r; p < t.p1; p += t.R) {
    const size_t at = base + (size_t)p * ldc;
    const float4 x = ld4(y + at);
    const float xv[4] = {x.x, x.y, x.z, x.w};
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (xv[i] - k.mean[i >> 1]) * k.rstd[i >> 1] * k.g[i] + k.be[i];
    if (NOP == 2) {
      const float4 z = ld4(y2 + at);
      const float zv[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] += (zv[i] - k2.mean[i >> 1]) * k2.rstd[i >> 1] * k2.g[i] + k2.be[i];
    }
    if (relu) {
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = o[i] < 0.0f ? 0.0f : o[i];   // (a NaN stays a NaN)
    }
    st4(out + at, o[0], o[1], o[2], o[3]);
  }
}

// ---------------------------------------------------------------- backward, pass 1: A = sum g, Q = sum g y^ (, Q2 = sum g y2^)
// g = dout where the saved result is positive (relu) or dout; part [B][nchunk][C][1 + NOP]
template <int NOP>
__global__ __launch_bounds__(DN_BS) void ce_gn_bwd_sums_kernel(const float* __restrict__ dout, const float* __restrict__ act,
                                                               const float* __restrict__ y, const float* __restrict__ stat,
                                                               const float* __restrict__ y2, const float* __restrict__ stat2,
                                                               double* __restrict__ part, long HW, int C, int ldc, int G,
                                                               int relu, long ppc, int nchunk) {
  constexpr int NS = 1 + NOP, NV = 4 * NS;
  __shared__ double red[DN_BS * NV];
  const DnPos t = dn_pos(C / 4, HW, ppc);
  const int b = blockIdx.z, c0 = 4 * t.q, cpg = C / G;
  double v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
  if (t.active) {
    float mean[2][2], rstd[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const size_t s = ((size_t)b * G + (c0 + 2 * h) / cpg) * 2;
      mean[0][h] = stat[s];
      rstd[0][h] = stat[s + 1];
      mean[1][h] = NOP == 2 ? stat2[s] : 0.0f;
      rstd[1][h] = NOP == 2 ? stat2[s + 1] : 0.0f;
    }
    const size_t base = ((size_t)b * HW) * ldc + c0;
#pragma unroll 2
    for (long p = t.p0 + t.r; p < t.p1; p += t.R) {
      const size_t at = base + (size_t)p * ldc;
      const float4 x = ld4(y + at), d = ld4(dout + at);
      float4 a = make_float4(1.f, 1.f, 1.f, 1.f), z = make_float4(0.f, 0.f, 0.f, 0.f);
      if (relu) a = ld4(act + at);
      if (NOP == 2) z = ld4(y2 + at);
      const float xv[4] = {x.x, x.y, x.z, x.w}, dv[4] = {d.x, d.y, d.z, d.w}, av[4] = {a.x, a.y, a.z, a.w},
                  zv[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double g = (double)(av[i] > 0.0f ? dv[i] : 0.0f);
        v[NS * i] += g;
        v[NS * i + 1] = fma(g, (double)((xv[i] - mean[0][i >> 1]) * rstd[0][i >> 1]), v[NS * i + 1]);
        if (NOP == 2) v[NS * i + 2] = fma(g, (double)((zv[i] - mean[1][i >> 1]) * rstd[1][i >> 1]), v[NS * i + 2]);
      }
    }
  }
  if (dn_block_sum<NV>(t, v, red)) {
    double* dst = part + (((size_t)b * nchunk + blockIdx.x) * C + c0) * NS;
#pragma unroll
    for (int i = 0; i < NV; ++i) dst[i] = v[i];
  }
}

// The finalisation of one sample: S [B][C][1 + NOP] = (A, Q, Q2), the runs added in order, and m [NOP][B][G][2] = the group
// means of gamma A and gamma Q of each GroupNorm.
template <int NOP>
__global__ __launch_bounds__(256) void ce_gn_bwd_final_kernel(const double* __restrict__ part, const float* __restrict__ gamma,
                                                              const float* __restrict__ gamma2, double* __restrict__ S,
                                                              double* __restrict__ m, int B, int nchunk, int C, int G, long HW) {
  constexpr int NS = 1 + NOP;
  extern __shared__ double sh[];                     // [NOP][2][C]: gamma A, gamma Q
  const int b = blockIdx.x, cpg = C / G;
  for (int c = threadIdx.x; c < C; c += 256) {
    double s[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] = 0.0;
    for (int k = 0; k < nchunk; ++k) {
      const double* p = part + (((size_t)b * nchunk + k) * C + c) * NS;
#pragma unroll
      for (int j = 0; j < NS; ++j) s[j] += p[j];
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) S[((size_t)b * C + c) * NS + j] = s[j];
#pragma unroll
    for (int op = 0; op < NOP; ++op) {
      const double ga = op ? gamma2[c] : gamma[c];
      sh[(size_t)(2 * op) * C + c] = ga * s[0];
      sh[(size_t)(2 * op + 1) * C + c] = ga * s[1 + op];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NOP * G; i += 256) {
    const int op = i / G, g = i - op * G;
    double a = 0.0, q = 0.0;
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
      a += sh[(size_t)(2 * op) * C + c];
      q += sh[(size_t)(2 * op + 1) * C + c];
    }
    const double n = (double)HW * cpg;
    m[(((size_t)op * B + b) * G + g) * 2] = a / n;
    m[(((size_t)op * B + b) * G + g) * 2 + 1] = q / n;
  }
}

// ---------------------------------------------------------------- backward, pass 2: dy = rstd (gamma g - m1 - y^ m2)
// The workgroups of run 0 of sample 0 also add S over the batch, in order: dbeta (the same for both GroupNorms), dgamma.
// dy may be dout: a thread reads its 16 bytes of dout before it writes them.
template <int NOP>
__global__ __launch_bounds__(DN_BS) void ce_gn_dy_kernel(const float* dout, const float* __restrict__ act,
                                                         const float* __restrict__ y, const float* __restrict__ stat,
                                                         const float* __restrict__ gamma, const float* __restrict__ y2,
                                                         const float* __restrict__ stat2, const float* __restrict__ gamma2,
                                                         const double* __restrict__ S, const double* __restrict__ m,
                                                         float* __restrict__ dgamma, float* __restrict__ dbeta, float* dy,
                                                         float* __restrict__ dgamma2, float* __restrict__ dbeta2,
                                                         float* __restrict__ dy2, int B, long HW, int C, int ldc, int G, int relu,
                                                         long ppc) {
  constexpr int NS = 1 + NOP;
  const DnPos t = dn_pos(ldc / 4, HW, ppc);
  if (!t.active) return;
  const int b = blockIdx.z, c0 = 4 * t.q, cpg = C / G;
  const size_t base = ((size_t)b * HW) * ldc + c0;
  if (c0 >= C) {
    for (long p = t.p0 + t.r; p < t.p1; p += t.R) {
      st4(dy + base + (size_t)p * ldc, 0.f, 0.f, 0.f, 0.f);
      if (NOP == 2) st4(dy2 + base + (size_t)p * ldc, 0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  if (blockIdx.x == 0 && b == 0 && t.r == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double s[NS];
#pragma unroll
      for (int j = 0; j < NS; ++j) s[j] = 0.0;
      for (int bb = 0; bb < B; ++bb) {
#pragma unroll
        for (int j = 0; j < NS; ++j) s[j] += S[((size_t)bb * C + c0 + i) * NS + j];
      }
      dbeta[c0 + i] = (float)s[0];
      dgamma[c0 + i] = (float)s[1];
      if (NOP == 2) {
        dbeta2[c0 + i] = (float)s[0];
        dgamma2[c0 + i] = (float)s[2];
      }
    }
  }
  const CeCoef k = ce_coef(stat, gamma, nullptr, b, c0, cpg, G);
  CeCoef k2 = k;
  if (NOP == 2) k2 = ce_coef(stat2, gamma2, nullptr, b, c0, cpg, G);
  float kd[4], m1[2], m2[2], kd2[4], n1[2], n2[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const size_t s = ((size_t)b * G + (c0 + 2 * h) / cpg) * 2;
    m1[h] = k.rstd[h] * (float)m[s];
    m2[h] = k.rstd[h] * (float)m[s + 1];
    n1[h] = NOP == 2 ? k2.rstd[h] * (float)m[(size_t)B * G * 2 + s] : 0.0f;
    n2[h] = NOP == 2 ? k2.rstd[h] * (float)m[(size_t)B * G * 2 + s + 1] : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    kd[i] = k.rstd[i >> 1] * k.g[i];
    kd2[i] = k2.rstd[i >> 1] * k2.g[i];
  }
  for (long p = t.p0 + t.r; p < t.p1; p += t.R) {
    const size_t at = base + (size_t)p * ldc;
    const float4 x = ld4(y + at), d = ld4(dout + at);
    float4 a = make_float4(1.f, 1.f, 1.f, 1.f), z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (relu) a = ld4(act + at);
    if (NOP == 2) z = ld4(y2 + at);
    const float xv[4] = {x.x, x.y, x.z, x.w}, dv[4] = {d.x, d.y, d.z, d.w}, av[4] = {a.x, a.y, a.z, a.w},
                zv[4] = {z.x, z.y, z.z, z.w};
    float o[4], o2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float g = av[i] > 0.0f ? dv[i] : 0.0f;
      o[i] = kd[i] * g - m1[i >> 1] - (xv[i] - k.mean[i >> 1]) * k.rstd[i >> 1] * m2[i >> 1];
      o2[i] = kd2[i] * g - n1[i >> 1] - (zv[i] - k2.mean[i >> 1]) * k2.rstd[i >> 1] * n2[i >> 1];
    }
    st4(dy + at, o[0], o[1], o[2], o[3]);
    if (NOP == 2) st4(dy2 + at, o2[0], o2[1], o2[2], o2[3]);
  }
}

// ---------------------------------------------------------------- im2col of a 3 x 3 (padding 1) convolution on an image
// out [B, H, W, ldk], column (ci 3 + ky) 3 + kx = x[b][ci][y + ky - 1][x + kx - 1] (zero outside the image and from column
// 9 Cin on) from an image [B, Cin, H, W] of any strides; four columns per thread
__global__ __launch_bounds__(256) void ce_im2col3_kernel(const float* __restrict__ x, float* __restrict__ out, long n, int Cin,
                                                         int H, int W, long sb, long sc, long sh, long sw, int ldk) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int Q = ldk / 4;
  const int q = (int)(i % Q);
  long r = i / Q;
  const int xx = (int)(r % W);
  r /= W;
  const int yy = (int)(r % H);
  const long b = r / H;
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = 4 * q + k;
    const int ci = j / 9, t = j - ci * 9, ky = t / 3, kx = t - ky * 3;
    const int sy = yy + ky - 1, sx = xx + kx - 1;
    const bool in = ci < Cin && sy >= 0 && sy < H && sx >= 0 && sx < W;
    v[k] = in ? x[b * sb + ci * sc + sy * sh + sx * sw] : 0.0f;
  }
  st4(out + 4 * i, v[0], v[1], v[2], v[3]);
}

constexpr long CE_MAX_PIXELS = 1L << 36;      // batch included: with ldc <= 4096 no count below leaves int64
constexpr int CE_MAX_C = 2048;                // the two-operand backward's finalisation keeps 4 C doubles in LDS (64 KB)
constexpr int CE_MAX_LDC = 4096;
constexpr int CE_MAX_B = 32767;               // the statistics pass has 2 B workgroup layers

inline bool ce_map_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && H <= (1 << 20) && W <= (1 << 20) && (long)H * W <= CE_MAX_PIXELS / B;
}
// C a multiple of 4 (a thread's four channels) and of 2 groups (a pair of channels lies in one group)
inline bool ce_gn_shape_ok(int B, int H, int W, int C, int ldc, int G) {
  return ce_map_ok(B, H, W) && B <= CE_MAX_B && C > 0 && G > 0 && C % 4 == 0 && C % G == 0 && (C / G) % 2 == 0 && ldc >= C &&
         ldc % 4 == 0 && C <= CE_MAX_C && ldc <= CE_MAX_LDC;
}
inline bool ce_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
}  // namespace

extern "C" int64_t ld_dn_gnr_work_bytes(int B, int H, int W, int C, int groups) {
  if (!ce_gn_shape_ok(B, H, W, C, C, groups)) return 0;
  long ppc;
  int nchunk;
  dn_runs(B, (long)H * W, C / 4, ppc, nchunk);
  const int64_t runs = (int64_t)B * nchunk * C;
  const int64_t fwd = 2 * runs * 2;                                                       // [2][B][nchunk][C][2]
  const int64_t bwd = runs * 3 + (int64_t)B * C * 3 + 2 * (int64_t)B * groups * 2;        // part, S, m
  return (fwd > bwd ? fwd : bwd) * (int64_t)sizeof(double);
}

extern "C" int ld_dn_gnr_forward(const float* y, const float* gamma, const float* beta, const float* y2, const float* gamma2,
                                 const float* beta2, double* work, float* stat, float* stat2, float* out, int B, int H, int W,
                                 int C, int ldc, int groups, int relu, void* stream) {
  LD_REQUIRE(ce_gn_shape_ok(B, H, W, C, ldc, groups),
             "ld_dn_gnr_forward: B=%d H=%d W=%d C=%d ldc=%d groups=%d (C a multiple of 4 and of 2 * groups, ldc >= C a multiple of "
             "4, C <= 2048, ldc <= 4096, B <= 32767)", B, H, W, C, ldc, groups);
  LD_REQUIRE(y && gamma && beta && work && stat && out, "ld_dn_gnr_forward: null pointer");
  LD_REQUIRE(y2 ? (gamma2 && beta2 && stat2) : (!gamma2 && !beta2 && !stat2),
             "ld_dn_gnr_forward: y2, gamma2, beta2 and stat2 go together (null pointer)");
  LD_REQUIRE(dn_aligned16(y) && dn_aligned16(gamma) && dn_aligned16(beta) && dn_aligned16(y2) && dn_aligned16(gamma2) &&
                 dn_aligned16(beta2) && dn_aligned16(out) && ce_aligned8(work),
             "ld_dn_gnr_forward: a pointer is not 16-byte aligned (work: 8-byte)");
  const long HW = (long)H * W;
  const int nop = y2 ? 2 : 1;
  hipStream_t st = dn_st(stream);
  long ppc;
  int nchunk;
  dn_runs(B, HW, C / 4, ppc, nchunk);
  LD_LAUNCH(ce_gn_stats_kernel, dim3((unsigned)nchunk, (unsigned)((C / 4 + DN_LANES - 1) / DN_LANES), (unsigned)(nop * B)),
            dim3(DN_BS), 0, st, y, y2, work, B, HW, C, ldc, ppc, nchunk);
  LD_LAUNCH(ce_gn_stats_final_kernel, dim3((unsigned)B, (unsigned)nop), dim3(256), 2 * (size_t)C * sizeof(double), st,
            (const double*)work, stat, stat2, B, nchunk, C, groups, HW);
  long ppa;
  int na;
  dn_runs(B, HW, ldc / 4, ppa, na);
  const dim3 grid((unsigned)na, (unsigned)((ldc / 4 + DN_LANES - 1) / DN_LANES), (unsigned)B);
  if (nop == 2)
    LD_LAUNCH(ce_gn_apply_kernel<2>, grid, dim3(DN_BS), 0, st, y, (const float*)stat, gamma, beta, y2, (const float*)stat2, gamma2,
              beta2, out, HW, C, ldc, groups, relu, ppa);
  else
    LD_LAUNCH(ce_gn_apply_kernel<1>, grid, dim3(DN_BS), 0, st, y, (const float*)stat, gamma, beta, y2, (const float*)stat2, gamma2,
              beta2, out, HW, C, ldc, groups, relu, ppa);
  LD_LAUNCH_CHECK("dn_gnr_forward");
  return LD_OK;
}

extern "C" int ld_dn_gnr_backward(const float* dout, const float* act, const float* y, const float* stat, const float* gamma,
                                  const float* y2, const float* stat2, const float* gamma2, double* work, float* dgamma,
                                  float* dbeta, float* dy, float* dgamma2, float* dbeta2, float* dy2, int B, int H, int W, int C,
                                  int ldc, int groups, int relu, void* stream) {
  LD_REQUIRE(ce_gn_shape_ok(B, H, W, C, ldc, groups),
             "ld_dn_gnr_backward: B=%d H=%d W=%d C=%d ldc=%d groups=%d (C a multiple of 4 and of 2 * groups, ldc >= C a multiple "
             "of 4, C <= 2048, ldc <= 4096, B <= 32767)", B, H, W, C, ldc, groups);
  LD_REQUIRE(dout && y && stat && gamma && work && dgamma && dbeta && dy, "ld_dn_gnr_backward: null pointer");
  LD_REQUIRE(!relu || act, "ld_dn_gnr_backward: relu needs the saved result (null pointer)");
  LD_REQUIRE(y2 ? (stat2 && gamma2 && dgamma2 && dbeta2 && dy2) : (!stat2 && !gamma2 && !dgamma2 && !dbeta2 && !dy2),
             "ld_dn_gnr_backward: y2, stat2, gamma2, dgamma2, dbeta2 and dy2 go together (null pointer)");
  LD_REQUIRE(dn_aligned16(dout) && dn_aligned16(act) && dn_aligned16(y) && dn_aligned16(gamma) && dn_aligned16(y2) &&
                 dn_aligned16(gamma2) && dn_aligned16(dy) && dn_aligned16(dy2) && ce_aligned8(work),
             "ld_dn_gnr_backward: a pointer is not 16-byte aligned (work: 8-byte)");
  LD_REQUIRE(dy2 == nullptr || (dy2 != dy && dy2 != dout), "ld_dn_gnr_backward: dy2 must be a buffer of its own");
  const long HW = (long)H * W;
  const int nop = y2 ? 2 : 1, ns = 1 + nop;
  hipStream_t st = dn_st(stream);
  long ppc;
  int nchunk;
  dn_runs(B, HW, C / 4, ppc, nchunk);
  double* S = work + (size_t)B * nchunk * C * ns;
  double* m = S + (size_t)B * C * ns;
  long ppa;
  int na;
  dn_runs(B, HW, ldc / 4, ppa, na);
  const dim3 gs((unsigned)nchunk, (unsigned)((C / 4 + DN_LANES - 1) / DN_LANES), (unsigned)B);
  const dim3 ga((unsigned)na, (unsigned)((ldc / 4 + DN_LANES - 1) / DN_LANES), (unsigned)B);
  const size_t lds = 2 * (size_t)nop * C * sizeof(double);
#define CE_BWD(N)                                                                                                                \
  do {                                                                                                                           \
    LD_LAUNCH(ce_gn_bwd_sums_kernel<N>, gs, dim3(DN_BS), 0, st, dout, act, y, stat, y2, stat2, work, HW, C, ldc, groups, relu,   \
              ppc, nchunk);                                                                                                      \
    LD_LAUNCH(ce_gn_bwd_final_kernel<N>, dim3((unsigned)B), dim3(256), lds, st, (const double*)work, gamma, gamma2, S, m, B,     \
              nchunk, C, groups, HW);                                                                                            \
    LD_LAUNCH(ce_gn_dy_kernel<N>, ga, dim3(DN_BS), 0, st, dout, act, y, stat, gamma, y2, stat2, gamma2, (const double*)S,        \
              (const double*)m, dgamma, dbeta, dy, dgamma2, dbeta2, dy2, B, HW, C, ldc, groups, relu, ppa);                      \
  } while (0)
  if (nop == 2)
    CE_BWD(2);
  else
    CE_BWD(1);
#undef CE_BWD
  LD_LAUNCH_CHECK("dn_gnr_backward");
  return LD_OK;
}

extern "C" int ld_dn_im2col3(const float* x, float* out, int B, int Cin, int H, int W, int64_t sb, int64_t sc, int64_t sh,
                              int64_t sw, int ldk, void* stream) {
  LD_REQUIRE(ce_map_ok(B, H, W) && Cin >= 1 && Cin <= 4 && ldk >= 9 * Cin && ldk % 4 == 0 && ldk <= CE_MAX_LDC,
             "ld_dn_im2col3: B=%d Cin=%d H=%d W=%d ldk=%d (Cin 1..4, ldk >= 9 Cin a multiple of 4, <= 4096)", B, Cin, H, W, ldk);
  LD_REQUIRE(sb >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "ld_dn_im2col3: negative stride");
  LD_REQUIRE(x && out, "ld_dn_im2col3: null pointer");
  LD_REQUIRE(dn_aligned16(out), "ld_dn_im2col3: out is not 16-byte aligned");
  const long n = (long)B * H * W * (ldk / 4);
  LD_REQUIRE((n + 255) / 256 < (1L << 31), "ld_dn_im2col3: %ld pieces", n);
  LD_LAUNCH(ce_im2col3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dn_st(stream), x, out, n, Cin, H, W, (long)sb,
            (long)sc, (long)sh, (long)sw, ldk);
  LD_LAUNCH_CHECK("dn_im2col3");
  return LD_OK;
}
