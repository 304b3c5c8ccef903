// Training step of the segmentation U-Net (train_seg.py:78-95 on unet_model.UNet, bilinear=False), fp32 NHWC like
// patchcore.hip.  The training-mode forward and the data gradient of every convolution are ld_pc_conv launches (exact-f32
// MFMA implicit GEMM; the data gradient is the same convolution with the weight flipped in (ky, kx) and transposed in
// (Cout, Cin), which ld_seg_permute3 makes).  This file holds what is new:
//
//   * seg_wgrad_kernel: the weight gradient dW[co][tap][ci] = sum_p dY[p][co] * A[p + tap][ci] as an implicit GEMM on
//     v_mfma_f32_32x32x2_f32 (rows = output channels, columns = input channels, K = pixels in chunks of 32, both operands
//     channel-contiguous, so the chunks go to LDS as they sit in memory).  The pixel axis is split over workgroups; each
//     split writes its own slab and seg_wgrad_reduce_kernel adds the slabs in index order (no floating-point atomics:
//     a step is reproducible bit for bit).  ksize 1 gives the ConvTranspose2d(2, 2) weight gradient;
//   * per-channel reductions (BatchNorm batch statistics, BatchNorm backward's sum g / sum g x^, the ConvTranspose2d bias
//     gradient, the head's weight / bias gradient): one stage-1 kernel with fp64 accumulators over a fixed slab of rows per
//     workgroup, and a stage-2 kernel per use that adds the slabs in order.  They are bandwidth kernels, fp64 adds are free;
//   * the element-wise passes: BatchNorm normalise + affine + ReLU, its backward, the 2x2 max-pool and its backward (first
//     maximum in row-major order, ATen's rule) fused with the add of the skip gradient, the concat with depth-to-space and
//     its split, the loss (BCE-with-logits with pos_weight + one dice term per batch) and dz, the head's dX, Adam.
#include "common.hip.h"
#include "adam.hip.h"

namespace {
typedef __attribute__((ext_vector_type(16))) float sg_f32x16;
constexpr int SG_T = 64;        // weight-gradient tile: 64 output channels x 64 input channels per workgroup
constexpr int SG_KC = 32;       // pixels per K-chunk
constexpr int SG_RED_MAX_WG = 2048;                         // stage-1 workgroups of a per-channel reduction, at most
static_assert((long)SG_RED_MAX_WG * 2 * 64 * 8 == LD_SEG_RED_WORK_BYTES, "the reductions' scratch: [slabs][2][C] doubles");
constexpr int SG_LOSS_MAX_WG = 1024;

// ------------------------------------------------------------------------------------------------ weight gradient
struct SgWgradDev {
  const float* dy; const float* a; float* work;
  long M, nchunks;
  int H, W, Cin, Cout, ks, chunks_per_split;
};

__global__ __launch_bounds__(256) void seg_wgrad_kernel(SgWgradDev d) {
  __shared__ __attribute__((aligned(16))) float sa[SG_KC][SG_T + 4];   // [pixel][output channel]
  __shared__ __attribute__((aligned(16))) float sb[SG_KC][SG_T + 4];   // [pixel][input channel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int nci = d.Cin / SG_T;
  const int co0 = ((int)blockIdx.x / nci) * SG_T, ci0 = ((int)blockIdx.x % nci) * SG_T;
  const int tap = blockIdx.y, taps = d.ks * d.ks;
  const int oy = d.ks == 3 ? tap / 3 - 1 : 0, ox = d.ks == 3 ? tap % 3 - 1 : 0;
  const long c0 = (long)blockIdx.z * d.chunks_per_split;
  const long c1 = c0 + d.chunks_per_split < d.nchunks ? c0 + d.chunks_per_split : d.nchunks;
  const int lk = tid >> 4, lc = (tid & 15) * 4;               // loader: pixels lk and lk + 16 of the chunk, 4 channels
  float4 ra[2], rb[2];
  auto fetch = [&](long q) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long p = q * SG_KC + lk + 16 * u;
      ra[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      rb[u] = ra[u];
      if (p < d.M) {
        ra[u] = *reinterpret_cast<const float4*>(d.dy + p * d.Cout + co0 + lc);
        const int x = (int)(p % d.W), y = (int)((p / d.W) % d.H);
        const int yy = y + oy, xx = x + ox;
        if (yy >= 0 && yy < d.H && xx >= 0 && xx < d.W)        // same image: the shifted pixel is p + oy * W + ox
          rb[u] = *reinterpret_cast<const float4*>(d.a + (p + (long)oy * d.W + ox) * d.Cin + ci0 + lc);
      }
    }
  };
  sg_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  if (c0 < c1) fetch(c0);
  const int kh = lane >> 5, c = lane & 31;
  for (long q = c0; q < c1; ++q) {
    __syncthreads();                                          // the previous chunk's reads of the tiles are done
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      *reinterpret_cast<float4*>(&sa[lk + 16 * u][lc]) = ra[u];
      *reinterpret_cast<float4*>(&sb[lk + 16 * u][lc]) = rb[u];
    }
    __syncthreads();
    if (q + 1 < c1) fetch(q + 1);
#pragma unroll
    for (int kk = 0; kk < SG_KC; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[kk + kh][wm * 32 + c], sb[kk + kh][wn * 32 + c], acc, 0, 0, 0);
  }
  // C/D layout of 32x32x2f32: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* slab = d.work + (long)blockIdx.z * d.Cout * taps * d.Cin;
  const int ci = ci0 + wn * 32 + c;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
    slab[((long)co * taps + tap) * d.Cin + ci] = acc[r];
  }
}

__global__ void seg_wgrad_reduce_kernel(const float* __restrict__ work, float* dw, long n, int splits) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = work[i];
  for (int k = 1; k < splits; ++k) s += work[(long)k * n + i];
  dw[i] = s;
}

// ------------------------------------------------------------------------------------------------ per-channel reductions
enum { SG_RED_STATS = 0, SG_RED_BN_BWD = 1, SG_RED_SUM = 2, SG_RED_HEAD = 3 };
struct SgRedDev {
  const float* x;        // STATS: y; BN_BWD: dA; SUM: x; HEAD: x (the head's input)
  const float* act;      // BN_BWD: the saved activation A (ReLU mask A > 0)
  const float* y;        // BN_BWD: the saved convolution output
  const float* stat;     // BN_BWD: [3][C] mean, biased variance, invstd
  const float* dz;       // HEAD: [M]
  double* part;          // [slabs][2][C]
  long M, rows_per_slab;
  int C;
};

template <int MODE>
__global__ __launch_bounds__(256) void seg_colred_kernel(SgRedDev d) {
  __shared__ double red[2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + lane;
  const long r0 = (long)blockIdx.x * d.rows_per_slab;
  const long r1 = r0 + d.rows_per_slab < d.M ? r0 + d.rows_per_slab : d.M;
  double s0 = 0.0, s1 = 0.0;
  float mean = 0.0f, invstd = 0.0f;
  if constexpr (MODE == SG_RED_BN_BWD) { mean = d.stat[c]; invstd = d.stat[2 * d.C + c]; }
  for (long r = r0 + wave; r < r1; r += 4) {
    const long i = r * d.C + c;
    if constexpr (MODE == SG_RED_STATS) {
      const float v = d.x[i];
      s0 += (double)v;
      s1 += (double)v * (double)v;
    } else if constexpr (MODE == SG_RED_BN_BWD) {
      const float g = d.act[i] > 0.0f ? d.x[i] : 0.0f;
      const float xh = (d.y[i] - mean) * invstd;
      s0 += (double)g;
      s1 += (double)g * (double)xh;
    } else if constexpr (MODE == SG_RED_SUM) {
      s0 += (double)d.x[i];
    } else {
      const float z = d.dz[r];
      s0 += (double)z * (double)d.x[i];
      s1 += (double)z;
    }
  }
  red[0][wave][lane] = s0;
  red[1][wave][lane] = s1;
  __syncthreads();
  if (wave == 0) {
    double* p = d.part + (long)blockIdx.x * 2 * d.C;
    p[c] = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
    p[d.C + c] = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
  }
}

__device__ __forceinline__ double sg_slab_sum(const double* part, int slabs, int C, int q, int c) {
  double s = 0.0;
  for (int k = 0; k < slabs; ++k) s += part[((long)k * 2 + q) * C + c];
  return s;
}

// BatchNorm2d (train): mean, biased variance, invstd; running statistics as nn.BatchNorm2d updates them (unbiased variance)
__global__ void seg_bn_stats_final_kernel(const double* __restrict__ part, int slabs, int C, long n, float eps, float momentum,
                                          float* stat, float* running_mean, float* running_var) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double mean = sg_slab_sum(part, slabs, C, 0, c) / (double)n;
  double var = sg_slab_sum(part, slabs, C, 1, c) / (double)n - mean * mean;
  if (var < 0.0) var = 0.0;
  stat[c] = (float)mean;
  stat[C + c] = (float)var;
  stat[2 * C + c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * (float)mean;
  if (running_var) {
    const float unbiased = (float)(var * ((double)n / (double)(n > 1 ? n - 1 : 1)));
    running_var[c] = (1.0f - momentum) * running_var[c] + momentum * unbiased;
  }
}

__global__ void seg_bn_bwd_final_kernel(const double* __restrict__ part, int slabs, int C, float* dgamma, float* dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  dbeta[c] = (float)sg_slab_sum(part, slabs, C, 0, c);
  dgamma[c] = (float)sg_slab_sum(part, slabs, C, 1, c);
}

// out[c] = sum over the `fold` channel groups of Cf = C / fold channels (the (p1, p2) positions of a ConvTranspose2d)
__global__ void seg_colsum_final_kernel(const double* __restrict__ part, int slabs, int C, int fold, float* out) {
  const int Cf = C / fold;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= Cf) return;
  double s = 0.0;
  for (int f = 0; f < fold; ++f) s += sg_slab_sum(part, slabs, C, 0, f * Cf + c);
  out[c] = (float)s;
}

__global__ void seg_head_bwd_final_kernel(const double* __restrict__ part, int slabs, int C, float* dw, float* db) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  dw[c] = (float)sg_slab_sum(part, slabs, C, 0, c);
  if (c == 0) db[0] = (float)sg_slab_sum(part, slabs, C, 1, 0);
}

// ------------------------------------------------------------------------------------------------ element-wise passes
__global__ void seg_bn_apply_kernel(const float* __restrict__ y, const float* __restrict__ stat, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, float* out, long total4, int C) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int c = (int)((i * 4) % C);
  const float4 v = reinterpret_cast<const float4*>(y)[i];
  const float in[4] = {v.x, v.y, v.z, v.w};
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = fmaxf(((in[j] - stat[c + j]) * stat[2 * C + c + j]) * gamma[c + j] + beta[c + j], 0.0f);
  reinterpret_cast<float4*>(out)[i] = make_float4(o[0], o[1], o[2], o[3]);
}

// dY = gamma * invstd * (g - sum(g) / n - x^ * sum(g x^) / n), g = dA * (A > 0); dy may be da itself
__global__ void seg_bn_dy_kernel(const float* da, const float* __restrict__ act, const float* __restrict__ y,
                                 const float* __restrict__ stat, const float* __restrict__ gamma,
                                 const float* __restrict__ dgamma, const float* __restrict__ dbeta, float* dy, long total4,
                                 int C, float inv_n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int c = (int)((i * 4) % C);
  const float4 g4 = reinterpret_cast<const float4*>(da)[i], a4 = reinterpret_cast<const float4*>(act)[i];
  const float4 y4 = reinterpret_cast<const float4*>(y)[i];
  const float g[4] = {g4.x, g4.y, g4.z, g4.w}, a[4] = {a4.x, a4.y, a4.z, a4.w}, yv[4] = {y4.x, y4.y, y4.z, y4.w};
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float invstd = stat[2 * C + c + j];
    const float xh = (yv[j] - stat[c + j]) * invstd;
    const float gj = a[j] > 0.0f ? g[j] : 0.0f;
    o[j] = (gamma[c + j] * invstd) * ((gj - dbeta[c + j] * inv_n) - xh * (dgamma[c + j] * inv_n));
  }
  reinterpret_cast<float4*>(dy)[i] = make_float4(o[0], o[1], o[2], o[3]);
}

// MaxPool2d(2): x [B, 2H, 2W, C] -> out [B, H, W, C]; one thread per (output pixel, 4 channels)
__global__ void seg_pool_kernel(const float* __restrict__ x, float* out, long total, int H, int W, int C) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int C4 = C / 4;
  const int c = (int)(i % C4) * 4;
  const long p = i / C4;
  const int ox = (int)(p % W);
  const long r = p / W;                                       // b * H + oy
  const float* s = x + ((r * 2) * (2L * W) + 2 * ox) * C + c;
  const float4 v0 = *reinterpret_cast<const float4*>(s), v1 = *reinterpret_cast<const float4*>(s + C);
  const float4 v2 = *reinterpret_cast<const float4*>(s + 2L * W * C), v3 = *reinterpret_cast<const float4*>(s + (2L * W + 1) * C);
  float4 m;
  m.x = fmaxf(fmaxf(v0.x, v1.x), fmaxf(v2.x, v3.x));
  m.y = fmaxf(fmaxf(v0.y, v1.y), fmaxf(v2.y, v3.y));
  m.z = fmaxf(fmaxf(v0.z, v1.z), fmaxf(v2.z, v3.z));
  m.w = fmaxf(fmaxf(v0.w, v1.w), fmaxf(v2.w, v3.w));
  *reinterpret_cast<float4*>(out + p * C + c) = m;
}

// dx [B, 2H, 2W, C] = dskip (or 0) + dpool routed to the first maximum of each window in row-major order
__global__ void seg_pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dpool, const float* __restrict__ dskip,
                                    float* dx, long total, int H, int W, int C) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int C4 = C / 4;
  const int c = (int)(i % C4) * 4;
  const long p = i / C4;
  const int ox = (int)(p % W);
  const long r = p / W;
  const long base = ((r * 2) * (2L * W) + 2 * ox) * C + c;
  const long off[4] = {0, C, 2L * W * C, (2L * W + 1) * C};
  float v[4][4], o[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float4 t = *reinterpret_cast<const float4*>(x + base + off[k]);
    v[k][0] = t.x; v[k][1] = t.y; v[k][2] = t.z; v[k][3] = t.w;
    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (dskip) s = *reinterpret_cast<const float4*>(dskip + base + off[k]);
    o[k][0] = s.x; o[k][1] = s.y; o[k][2] = s.z; o[k][3] = s.w;
  }
  const float4 g4 = *reinterpret_cast<const float4*>(dpool + p * C + c);
  const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int best = 0;
    float m = v[0][j];
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (v[k][j] > m) { m = v[k][j]; best = k; }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k == best) o[k][j] += g[j];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    *reinterpret_cast<float4*>(dx + base + off[k]) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
}

// cat([skip [B, H, W, C0], depth_to_space(low [B, H/2, W/2, 4*C1])]) <-> its parts.  BWD = 0: out = cat; BWD = 1: split
template <int BWD>
__global__ void seg_cat_kernel(float* skip, float* low, float* cat, long total, int H, int W, int C0, int C1) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int Cc = C0 + C1, C4 = Cc / 4;
  const int c = (int)(i % C4) * 4;
  const long p = i / C4;
  const int x = (int)(p % W);
  const long r = p / W;
  const int y = (int)(r % H);
  const long b = r / H;
  float* part;
  if (c < C0) {
    part = skip + p * C0 + c;
  } else {
    const long pl = (b * (H >> 1) + (y >> 1)) * (W >> 1) + (x >> 1);
    part = low + pl * 4 * C1 + (((y & 1) << 1) | (x & 1)) * C1 + (c - C0);
  }
  float* whole = cat + p * Cc + c;
  if constexpr (BWD) *reinterpret_cast<float4*>(part) = *reinterpret_cast<const float4*>(whole);
  else *reinterpret_cast<float4*>(whole) = *reinterpret_cast<const float4*>(part);
}

// ------------------------------------------------------------------------------------------------ loss
__device__ __forceinline__ float sg_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// partial sums per workgroup: sum p t, sum p, sum t, sum bce (fp64), p = sigmoid(z)
__global__ __launch_bounds__(256) void seg_loss_partial_kernel(const float* __restrict__ z, const float* __restrict__ t, long M,
                                                               float pos_weight, double* part) {
  __shared__ double red[4][256];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long)gridDim.x * 256) {
    const float zi = z[i], ti = t[i];
    const float p = sg_sigmoid(zi);
    // F.binary_cross_entropy_with_logits: (1 - t) z + (1 + (pw - 1) t) (log1p(exp(-|z|)) + max(-z, 0))
    const float lw = 1.0f + (pos_weight - 1.0f) * ti;
    const float l = (1.0f - ti) * zi + lw * (log1pf(expf(-fabsf(zi))) + fmaxf(-zi, 0.0f));
    s[0] += (double)p * (double)ti;
    s[1] += (double)p;
    s[2] += (double)ti;
    s[3] += (double)l;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[q][threadIdx.x] = s[q];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x < 4) part[(long)blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0];
}

// sums [4] (fp64, behind the partials) and out = {loss, bce, dice loss}
__global__ void seg_loss_final_kernel(double* part, int nblk, long M, float dice_eps, float* out) {
  __shared__ double s[4];
  if (threadIdx.x < 4) {
    double a = 0.0;
    for (int k = 0; k < nblk; ++k) a += part[(long)k * 4 + threadIdx.x];
    s[threadIdx.x] = a;
    part[(long)nblk * 4 + threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double bce = s[3] / (double)M;
    const double dice = 1.0 - (2.0 * s[0] + (double)dice_eps) / (s[1] + s[2] + (double)dice_eps);
    out[0] = (float)(bce + dice);
    out[1] = (float)bce;
    out[2] = (float)dice;
  }
}

__global__ void seg_loss_dz_kernel(const float* __restrict__ z, const float* __restrict__ t, long M, float pos_weight,
                                   float dice_eps, const double* __restrict__ sums, float* dz) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const double N = 2.0 * sums[0] + (double)dice_eps, D = sums[1] + sums[2] + (double)dice_eps;
  const float a = (float)(2.0 / D), bq = (float)(N / (D * D)), inv_m = (float)(1.0 / (double)M);
  const float zi = z[i], ti = t[i];
  const float p = sg_sigmoid(zi);
  const float lw = 1.0f + (pos_weight - 1.0f) * ti;
  const float dbce = ((1.0f - ti) - lw * (1.0f - p)) * inv_m;
  const float ddice = (bq - a * ti) * (p * (1.0f - p));       // d(1 - N / D) / dp_i = N / D^2 - 2 t_i / D
  dz[i] = dbce + ddice;
}

__global__ void seg_head_dx_kernel(const float* __restrict__ dz, const float* __restrict__ w, float* dx, long total4, int C) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int c = (int)((i * 4) % C);
  const float g = dz[(i * 4) / C];
  reinterpret_cast<float4*>(dx)[i] = make_float4(g * w[c], g * w[c + 1], g * w[c + 2], g * w[c + 3]);
}

// ------------------------------------------------------------------------------------------------ optimiser, layouts
// torch.optim.Adam (ld_adam_update) over a group of tensors, the table by value as the kernel argument.  Tensor k owns
// elements [start[k], start[k + 1]) of the launch; its gradient is read through the strides of the weight-gradient layout
// and the updated value also goes to the mirrors (the kernel-layout copies), both in seg_permute3_kernel's index arithmetic
struct SgAdamDev {
  ld_seg_adam_tensor t[LD_SEG_ADAM_GROUP];
  long start[LD_SEG_ADAM_GROUP + 1];
  int count;
  float omb1, beta2, omb2, eps, step_size, bc2_sqrt;
};
static_assert(sizeof(SgAdamDev) <= 4096, "a group's table travels by value: the kernel-argument block holds 4 KB");

__global__ void seg_adam_kernel(SgAdamDev d) {
  const long gi = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= d.start[d.count]) return;
  int k = 0;
  while (gi >= d.start[k + 1]) ++k;
  const ld_seg_adam_tensor& t = d.t[k];
  const long i = gi - d.start[k];
  const long i2 = i % t.d2, r = i / t.d2, i0 = r / t.d1, i1 = r % t.d1;
  float p = t.param[i], m = t.m[i], v = t.v[i];
  ld_adam_update(p, t.grad[i0 * t.gs0 + i1 * t.gs1 + i2 * t.gs2], m, v, d.omb1, d.beta2, d.omb2, d.eps, d.step_size, d.bc2_sqrt);
  t.m[i] = m; t.v[i] = v; t.param[i] = p;
  if (t.mirror0) t.mirror0[t.m0_off + i0 * t.m0_s0 + i1 * t.m0_s1 + i2 * t.m0_s2] = p;
  if (t.mirror1) t.mirror1[t.m1_off + i0 * t.m1_s0 + i1 * t.m1_s1 + i2 * t.m1_s2] = p;
}

// out[off + i0 s0 + i1 s1 + i2 s2] = in[(i0 d1 + i1) d2 + i2]
__global__ void seg_permute3_kernel(const float* __restrict__ in, float* out, long n, int d1, int d2, long off, long s0, long s1,
                                    long s2) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long i2 = i % d2, r = i / d2;
  out[off + (r / d1) * s0 + (r % d1) * s1 + i2 * s2] = in[i];
}

inline unsigned sg_blocks(long n) { return (unsigned)((n + 255) / 256); }

// rows per slab / slabs of a per-channel reduction over x [M][C]: about SG_RED_MAX_WG workgroups, at least 32 rows each
inline void sg_red_shape(long M, int C, long& rows_per_slab, int& slabs) {
  long want = SG_RED_MAX_WG / (C / 64);
  if (want < 1) want = 1;
  const long most = (M + 31) / 32;
  if (want > most) want = most;
  rows_per_slab = (M + want - 1) / want;
  slabs = (int)((M + rows_per_slab - 1) / rows_per_slab);
}

template <int MODE>
void sg_red_launch(SgRedDev& d, int& slabs, hipStream_t st) {
  sg_red_shape(d.M, d.C, d.rows_per_slab, slabs);
  LD_LAUNCH((seg_colred_kernel<MODE>), dim3((unsigned)slabs, (unsigned)(d.C / 64)), dim3(256), 0, st, d);
}

inline bool sg_red_ok(long M, int C) { return M > 0 && C > 0 && C % 64 == 0 && C / 64 <= SG_RED_MAX_WG && M * C / 4 / 256 < (1L << 31); }
}  // namespace

extern "C" int ld_seg_wgrad_splits(int B, int H, int W, int Cin, int Cout, int ksize) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin % SG_T || Cout % SG_T || (ksize != 1 && ksize != 3)) return 0;
  const long nchunks = ((long)B * H * W + SG_KC - 1) / SG_KC;
  const long tiles = (long)(Cin / SG_T) * (Cout / SG_T) * ksize * ksize;
  long splits = (2048 + tiles - 1) / tiles;                  // about eight workgroups per CU in all
  if (splits > nchunks) splits = nchunks;
  if (splits > 1024) splits = 1024;
  const long per = (nchunks + splits - 1) / splits;
  return (int)((nchunks + per - 1) / per);
}

extern "C" int ld_seg_wgrad(const float* dy, const float* a, float* work, float* dw, int B, int H, int W, int Cin, int Cout,
                            int ksize, int splits, void* stream) {
  LD_REQUIRE(ksize == 1 || ksize == 3, "ld_seg_wgrad: ksize %d (1 or 3)", ksize);
  LD_REQUIRE(B > 0 && H > 0 && W > 0, "ld_seg_wgrad: empty shape B=%d H=%d W=%d", B, H, W);
  LD_REQUIRE(Cin > 0 && Cin % SG_T == 0, "ld_seg_wgrad: Cin %d (a multiple of 64)", Cin);
  LD_REQUIRE(Cout > 0 && Cout % SG_T == 0, "ld_seg_wgrad: Cout %d (a multiple of 64)", Cout);
  const long M = (long)B * H * W, nchunks = (M + SG_KC - 1) / SG_KC;
  LD_REQUIRE(splits >= 1 && splits <= nchunks && splits <= 65535, "ld_seg_wgrad: splits %d (1..min(%ld, 65535))", splits,
             nchunks);
  const long tiles = (long)(Cin / SG_T) * (Cout / SG_T);
  LD_REQUIRE(tiles < (1L << 31), "ld_seg_wgrad: %ld tiles", tiles);
  LD_REQUIRE(dy && a && work && dw, "ld_seg_wgrad: null pointer");
  const long per = (nchunks + splits - 1) / splits;
  SgWgradDev d{dy, a, work, M, nchunks, H, W, Cin, Cout, ksize, (int)per};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(seg_wgrad_kernel, dim3((unsigned)tiles, (unsigned)(ksize * ksize), (unsigned)splits), dim3(256), 0, st, d);
  const long n = (long)Cout * ksize * ksize * Cin;
  LD_LAUNCH(seg_wgrad_reduce_kernel, dim3(sg_blocks(n)), dim3(256), 0, st, work, dw, n, splits);
  LD_LAUNCH_CHECK("seg_wgrad");
  return LD_OK;
}

extern "C" int ld_seg_bn_train(const float* y, const float* gamma, const float* beta, double* work, float* stat,
                               float* running_mean, float* running_var, float momentum, float eps, float* out, int64_t M,
                               int C, void* stream) {
  LD_REQUIRE(sg_red_ok((long)M, C), "ld_seg_bn_train: M %ld C %d (C a multiple of 64)", (long)M, C);
  LD_REQUIRE(M >= 2, "ld_seg_bn_train: %ld values per channel (BatchNorm in training mode needs two)", (long)M);
  LD_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "ld_seg_bn_train: one running statistic without the other");
  LD_REQUIRE(y && gamma && beta && work && stat && out, "ld_seg_bn_train: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SgRedDev d{y, nullptr, nullptr, nullptr, nullptr, work, (long)M, 0, C};
  int slabs = 0;
  sg_red_launch<SG_RED_STATS>(d, slabs, st);
  LD_LAUNCH(seg_bn_stats_final_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, (const double*)work, slabs, C, (long)M,
            eps, momentum, stat, running_mean, running_var);
  const long total4 = (long)M * C / 4;
  LD_LAUNCH(seg_bn_apply_kernel, dim3(sg_blocks(total4)), dim3(256), 0, st, y, (const float*)stat, gamma, beta, out, total4, C);
  LD_LAUNCH_CHECK("seg_bn_train");
  return LD_OK;
}

extern "C" int ld_seg_bn_backward(const float* da, const float* act, const float* y, const float* gamma, const float* stat,
                                  double* work, float* dgamma, float* dbeta, float* dy, int64_t M, int C, void* stream) {
  LD_REQUIRE(sg_red_ok((long)M, C), "ld_seg_bn_backward: M %ld C %d (C a multiple of 64)", (long)M, C);
  LD_REQUIRE(da && act && y && gamma && stat && work && dgamma && dbeta && dy, "ld_seg_bn_backward: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SgRedDev d{da, act, y, stat, nullptr, work, (long)M, 0, C};
  int slabs = 0;
  sg_red_launch<SG_RED_BN_BWD>(d, slabs, st);
  LD_LAUNCH(seg_bn_bwd_final_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, (const double*)work, slabs, C, dgamma,
            dbeta);
  const long total4 = (long)M * C / 4;
  LD_LAUNCH(seg_bn_dy_kernel, dim3(sg_blocks(total4)), dim3(256), 0, st, da, act, y, stat, gamma, (const float*)dgamma,
            (const float*)dbeta, dy, total4, C, (float)(1.0 / (double)M));
  LD_LAUNCH_CHECK("seg_bn_backward");
  return LD_OK;
}

extern "C" int ld_seg_colsum(const float* x, double* work, float* out, int64_t M, int C, int fold, void* stream) {
  LD_REQUIRE(sg_red_ok((long)M, C), "ld_seg_colsum: M %ld C %d (C a multiple of 64)", (long)M, C);
  LD_REQUIRE(fold >= 1 && C % fold == 0, "ld_seg_colsum: fold %d does not divide C %d", fold, C);
  LD_REQUIRE(x && work && out, "ld_seg_colsum: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SgRedDev d{x, nullptr, nullptr, nullptr, nullptr, work, (long)M, 0, C};
  int slabs = 0;
  sg_red_launch<SG_RED_SUM>(d, slabs, st);
  LD_LAUNCH(seg_colsum_final_kernel, dim3((unsigned)((C / fold + 63) / 64)), dim3(64), 0, st, (const double*)work, slabs, C,
            fold, out);
  LD_LAUNCH_CHECK("seg_colsum");
  return LD_OK;
}

extern "C" int ld_seg_pool(const float* x, float* out, int B, int H, int W, int C, void* stream) {
  LD_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "ld_seg_pool: shape B=%d H=%d W=%d C=%d (C a multiple of 4)", B, H,
             W, C);
  LD_REQUIRE(x && out, "ld_seg_pool: null pointer");
  const long total = (long)B * H * W * (C / 4);
  LD_REQUIRE((total + 255) / 256 < (1L << 31), "ld_seg_pool: %ld elements", total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(seg_pool_kernel, dim3(sg_blocks(total)), dim3(256), 0, st, x, out, total, H, W, C);
  LD_LAUNCH_CHECK("seg_pool");
  return LD_OK;
}

extern "C" int ld_seg_pool_backward(const float* x, const float* dpool, const float* dskip, float* dx, int B, int H, int W,
                                    int C, void* stream) {
  LD_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0,
             "ld_seg_pool_backward: shape B=%d H=%d W=%d C=%d (C a multiple of 4)", B, H, W, C);
  LD_REQUIRE(x && dpool && dx, "ld_seg_pool_backward: null pointer");
  const long total = (long)B * H * W * (C / 4);
  LD_REQUIRE((total + 255) / 256 < (1L << 31), "ld_seg_pool_backward: %ld elements", total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(seg_pool_bwd_kernel, dim3(sg_blocks(total)), dim3(256), 0, st, x, dpool, dskip, dx, total, H, W, C);
  LD_LAUNCH_CHECK("seg_pool_backward");
  return LD_OK;
}

static int sg_cat(int bwd, float* skip, float* low, float* cat, int B, int H, int W, int C0, int C1, void* stream,
                  const char* name) {
  LD_REQUIRE(B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "%s: shape B=%d H=%d W=%d (H, W even)", name, B, H, W);
  LD_REQUIRE(C0 > 0 && C1 > 0 && C0 % 4 == 0 && C1 % 4 == 0, "%s: C0 %d C1 %d (multiples of 4)", name, C0, C1);
  LD_REQUIRE(skip && low && cat, "%s: null pointer", name);
  const long total = (long)B * H * W * ((C0 + C1) / 4);
  LD_REQUIRE((total + 255) / 256 < (1L << 31), "%s: %ld elements", name, total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (bwd)
    LD_LAUNCH(seg_cat_kernel<1>, dim3(sg_blocks(total)), dim3(256), 0, st, skip, low, cat, total, H, W, C0, C1);
  else
    LD_LAUNCH(seg_cat_kernel<0>, dim3(sg_blocks(total)), dim3(256), 0, st, skip, low, cat, total, H, W, C0, C1);
  LD_LAUNCH_CHECK(name);
  return LD_OK;
}

extern "C" int ld_seg_cat_d2s(const float* skip, const float* low, float* out, int B, int H, int W, int C0, int C1,
                              void* stream) {
  return sg_cat(0, const_cast<float*>(skip), const_cast<float*>(low), out, B, H, W, C0, C1, stream, "ld_seg_cat_d2s");
}

extern "C" int ld_seg_cat_d2s_backward(const float* dcat, float* dskip, float* dlow, int B, int H, int W, int C0, int C1,
                                       void* stream) {
  return sg_cat(1, dskip, dlow, const_cast<float*>(dcat), B, H, W, C0, C1, stream, "ld_seg_cat_d2s_backward");
}

extern "C" int ld_seg_loss(const float* logits, const float* target, double* work, float* out, float* dz, int64_t M,
                           float pos_weight, float dice_eps, void* stream) {
  LD_REQUIRE(M > 0 && (M + 255) / 256 < (1L << 31), "ld_seg_loss: %ld logits", (long)M);
  LD_REQUIRE(logits && target && work && out, "ld_seg_loss: null pointer");
  int nblk = (int)(((long)M + 255) / 256 < SG_LOSS_MAX_WG ? ((long)M + 255) / 256 : SG_LOSS_MAX_WG);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(seg_loss_partial_kernel, dim3((unsigned)nblk), dim3(256), 0, st, logits, target, (long)M, pos_weight, work);
  LD_LAUNCH(seg_loss_final_kernel, dim3(1), dim3(64), 0, st, work, nblk, (long)M, dice_eps, out);
  if (dz)
    LD_LAUNCH(seg_loss_dz_kernel, dim3(sg_blocks((long)M)), dim3(256), 0, st, logits, target, (long)M, pos_weight, dice_eps,
              (const double*)(work + (long)nblk * 4), dz);
  LD_LAUNCH_CHECK("seg_loss");
  return LD_OK;
}

extern "C" int ld_seg_head_backward(const float* dz, const float* x, const float* w, double* work, float* dw, float* db,
                                    float* dx, int64_t M, int C, void* stream) {
  LD_REQUIRE(sg_red_ok((long)M, C), "ld_seg_head_backward: M %ld C %d (C a multiple of 64)", (long)M, C);
  LD_REQUIRE(dz && x && w && work && dw && db && dx, "ld_seg_head_backward: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SgRedDev d{x, nullptr, nullptr, nullptr, dz, work, (long)M, 0, C};
  int slabs = 0;
  sg_red_launch<SG_RED_HEAD>(d, slabs, st);
  LD_LAUNCH(seg_head_bwd_final_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, (const double*)work, slabs, C, dw, db);
  const long total4 = (long)M * C / 4;
  LD_LAUNCH(seg_head_dx_kernel, dim3(sg_blocks(total4)), dim3(256), 0, st, dz, w, dx, total4, C);
  LD_LAUNCH_CHECK("seg_head_backward");
  return LD_OK;
}

extern "C" int ld_seg_adam(const ld_seg_adam_tensor* tensors, int count, double beta1, double beta2, double eps, double step_size,
                           double bc2_sqrt, void* stream) {
  LD_REQUIRE(tensors && count >= 1 && count <= LD_SEG_ADAM_MAX, "ld_seg_adam: %d tensors (1..%d)", count, LD_SEG_ADAM_MAX);
  LD_REQUIRE(bc2_sqrt > 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
             "ld_seg_adam: betas / bias correction: beta1 %g beta2 %g eps %g sqrt(1 - beta2^t) %g", beta1, beta2, eps, bc2_sqrt);
  for (int k = 0; k < count; ++k) {                            // the whole table first: a refused call has changed nothing
    const ld_seg_adam_tensor& t = tensors[k];
    LD_REQUIRE(t.d0 > 0 && t.d1 > 0 && t.d2 > 0, "ld_seg_adam: tensor %d has an empty shape", k);
    LD_REQUIRE(t.param && t.grad && t.m && t.v, "ld_seg_adam: tensor %d has a null pointer", k);
    LD_REQUIRE(t.gs0 >= 0 && t.gs1 >= 0 && t.gs2 >= 0, "ld_seg_adam: tensor %d has a negative gradient stride", k);
    auto lowest = [&](int64_t off, int64_t s0, int64_t s1, int64_t s2) {
      return off + (s0 < 0 ? s0 * (t.d0 - 1) : 0) + (s1 < 0 ? s1 * (t.d1 - 1) : 0) + (s2 < 0 ? s2 * (t.d2 - 1) : 0);
    };
    LD_REQUIRE(!t.mirror0 || lowest(t.m0_off, t.m0_s0, t.m0_s1, t.m0_s2) >= 0, "ld_seg_adam: tensor %d: mirror0 index below 0", k);
    LD_REQUIRE(!t.mirror1 || lowest(t.m1_off, t.m1_s0, t.m1_s1, t.m1_s2) >= 0, "ld_seg_adam: tensor %d: mirror1 index below 0", k);
    LD_REQUIRE((long)t.d0 * t.d1 <= ((1L << 31) / LD_SEG_ADAM_GROUP - 1) * 256 / t.d2,     // a group fits the grid's 2^31
               "ld_seg_adam: tensor %d: %d x %d x %d elements", k, t.d0, t.d1, t.d2);
  }
  SgAdamDev d;
  d.omb1 = (float)(1.0 - beta1); d.beta2 = (float)beta2; d.omb2 = (float)(1.0 - beta2);
  d.eps = (float)eps; d.step_size = (float)step_size; d.bc2_sqrt = (float)bc2_sqrt;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int k0 = 0; k0 < count; k0 += LD_SEG_ADAM_GROUP) {
    d.count = count - k0 < LD_SEG_ADAM_GROUP ? count - k0 : LD_SEG_ADAM_GROUP;
    d.start[0] = 0;
    for (int k = 0; k < d.count; ++k) {
      d.t[k] = tensors[k0 + k];
      d.start[k + 1] = d.start[k] + (long)d.t[k].d0 * d.t[k].d1 * d.t[k].d2;
    }
    LD_LAUNCH(seg_adam_kernel, dim3(sg_blocks(d.start[d.count])), dim3(256), 0, st, d);
  }
  LD_LAUNCH_CHECK("seg_adam");
  return LD_OK;
}

extern "C" int ld_seg_permute3(const float* in, float* out, int d0, int d1, int d2, int64_t off, int64_t s0, int64_t s1,
                               int64_t s2, void* stream) {
  LD_REQUIRE(d0 > 0 && d1 > 0 && d2 > 0, "ld_seg_permute3: shape %d x %d x %d", d0, d1, d2);
  // every output index is in [lo, hi]: the caller's buffer must hold it, and it must not be negative
  const long lo = off + (s0 < 0 ? s0 * (d0 - 1) : 0) + (s1 < 0 ? s1 * (d1 - 1) : 0) + (s2 < 0 ? s2 * (d2 - 1) : 0);
  LD_REQUIRE(lo >= 0, "ld_seg_permute3: lowest output index %ld is negative", lo);
  LD_REQUIRE(in && out, "ld_seg_permute3: null pointer");
  const long n = (long)d0 * d1 * d2;
  LD_REQUIRE((n + 255) / 256 < (1L << 31), "ld_seg_permute3: %ld elements", n);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(seg_permute3_kernel, dim3(sg_blocks(n)), dim3(256), 0, st, in, out, n, d1, d2, (long)off, (long)s0, (long)s1,
            (long)s2);
  LD_LAUNCH_CHECK("seg_permute3");
  return LD_OK;
}
