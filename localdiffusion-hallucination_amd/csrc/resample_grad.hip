// Training the denoiser, fourth slice: what the layers between the blocks of the U-Net need besides ld_pc_conv /
// ld_seg_wgrad / ld_dn_colsum -- Downsample's rearrangement (ddpm.py:120-124) and its inverse, Upsample's nearest x2
// (ddpm.py:114-118) and its backward (the sum of each 2 x 2 window), the im2col that turns the 7 x 7 stem on 1..4 image
// channels into a 1 x 1 convolution, and the head (final_conv: C -> 1..8 channels) with its backward.
//
// fp32, activations NHWC with a pixel stride `ldc` >= C: channels C..ldc-1 are padding, never read and written as zeros.
// The layout kernels move 16 bytes per thread and add nothing (the window sum adds its four terms in one order); the head's
// weight and bias gradients are fp64 partial sums per workgroup, merged in index order by a second launch.  No atomics,
// nothing allocates, every entry point checks its arguments before it launches.
//
// The head kernels are memory-bound and built around the pixel stride: eight lanes share a pixel, lane l owns channels
// 32 j + 4 l .. + 3 of every 32-channel chunk j, so a wave's load is eight pixels x 128 contiguous bytes.  The forward walks
// the chunks with the weights in LDS and meets the eight lanes by three xor-shuffles per output; the backward gives each
// chunk a row of workgroups of its own (dout, O / C of the traffic, is read once per chunk), so a lane keeps O x 4 weights
// and O x 5 sums in registers whatever C is.
#include "common.hip.h"
#include "dn_common.hip.h"

namespace {

constexpr int RS_HEAD_MAX_O = 8;
constexpr int RS_HEAD_GROUPS = DN_BS / 8;        // pixels a workgroup of the head kernels holds at a time
constexpr int RS_HEAD_MAX_PARTS = 512;

__device__ __forceinline__ void st4z(float* p) { st4(p, 0.0f, 0.0f, 0.0f, 0.0f); }

// ---------------------------------------------------------------- Downsample: 'b c (h p1) (w p2) -> b (p1 p2 c) h w'
// out [B, H, W, 4 C], channel (p1 2 + p2) C + c, from x [B, 2 H, 2 W, ldc]; one 16-byte copy per thread
__global__ __launch_bounds__(256) void rs_space_to_depth_kernel(const float* __restrict__ x, float* __restrict__ out, long n,
                                                                int H, int W, int C, int ldc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int Q = C / 4;
  const int q = (int)(i % Q);
  long r = i / Q;
  const int p = (int)(r & 3);
  r >>= 2;
  const int xx = (int)(r % W);
  r /= W;
  const int yy = (int)(r % H);
  const long b = r / H;
  const float4 v = ld4(x + ((b * 2 * H + 2 * yy + (p >> 1)) * 2 * W + 2 * xx + (p & 1)) * ldc + 4 * q);
  st4(out + 4 * i, v.x, v.y, v.z, v.w);
}
// dx [B, 2 H, 2 W, ldc] (channels C..ldc-1 zero) from g [B, H, W, 4 C]: the inverse
__global__ __launch_bounds__(256) void rs_depth_to_space_kernel(const float* __restrict__ g, float* __restrict__ dx, long n, int H,
                                                                int W, int C, int ldc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int Q = ldc / 4;
  const int q = (int)(i % Q);
  long r = i / Q;
  const int xx = (int)(r % (2 * W));
  r /= 2 * W;
  const int yy = (int)(r % (2 * H));
  const long b = r / (2 * H);
  if (4 * q >= C) {
    st4z(dx + 4 * i);
    return;
  }
  const int p = (yy & 1) * 2 + (xx & 1);
  const float4 v = ld4(g + (((b * H + (yy >> 1)) * W + (xx >> 1)) * 4 + p) * C + 4 * q);
  st4(dx + 4 * i, v.x, v.y, v.z, v.w);
}

// ---------------------------------------------------------------- Upsample: nearest x 2
// out [B, 2 H, 2 W, ldc] (padding zero) from x [B, H, W, ldc]
__global__ __launch_bounds__(256) void rs_upsample2x_kernel(const float* __restrict__ x, float* __restrict__ out, long n, int H,
                                                            int W, int C, int ldc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int Q = ldc / 4;
  const int q = (int)(i % Q);
  long r = i / Q;
  const int xx = (int)(r % (2 * W));
  r /= 2 * W;
  const int yy = (int)(r % (2 * H));
  const long b = r / (2 * H);
  if (4 * q >= C) {
    st4z(out + 4 * i);
    return;
  }
  const float4 v = ld4(x + ((b * H + (yy >> 1)) * W + (xx >> 1)) * ldc + 4 * q);
  st4(out + 4 * i, v.x, v.y, v.z, v.w);
}
// dx [B, H, W, ldc] = ((g[2h][2w] + g[2h][2w+1]) + g[2h+1][2w]) + g[2h+1][2w+1] from g [B, 2 H, 2 W, ldc]; padding zero
__global__ __launch_bounds__(256) void rs_upsample2x_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx, long n, int H,
                                                                int W, int C, int ldc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int Q = ldc / 4;
  const int q = (int)(i % Q);
  long r = i / Q;
  const int xx = (int)(r % W);
  r /= W;
  const int yy = (int)(r % H);
  const long b = r / H;
  if (4 * q >= C) {
    st4z(dx + 4 * i);
    return;
  }
  const float* s = g + ((b * 2 * H + 2 * yy) * 2 * W + 2 * xx) * ldc + 4 * q;
  const float4 a = ld4(s), c = ld4(s + ldc), d = ld4(s + (size_t)2 * W * ldc), e = ld4(s + (size_t)2 * W * ldc + ldc);
  st4(dx + 4 * i, ((a.x + c.x) + d.x) + e.x, ((a.y + c.y) + d.y) + e.y, ((a.z + c.z) + d.z) + e.z, ((a.w + c.w) + d.w) + e.w);
}

// ---------------------------------------------------------------- the stem's im2col (7 x 7, padding 3)
// out [B, H, W, ldk], column (ci 7 + ky) 7 + kx = x[b][ci][y + ky - 3][x + kx - 3] (zero outside the image and from column
// 49 Cin on) from an image [B, Cin, H, W] of any strides; four columns per thread
__global__ __launch_bounds__(256) void rs_im2col_kernel(const float* __restrict__ x, float* __restrict__ out, long n, int Cin,
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
    const int ci = j / 49, t = j - ci * 49, ky = t / 7, kx = t - ky * 7;
    const int sy = yy + ky - 3, sx = xx + kx - 3;
    const bool in = ci < Cin && sy >= 0 && sy < H && sx >= 0 && sx < W;
    v[k] = in ? x[b * sb + ci * sc + sy * sh + sx * sw] : 0.0f;
  }
  st4(out + 4 * i, v[0], v[1], v[2], v[3]);
}

// ---------------------------------------------------------------- the head: Conv2d(C, O, 1), O <= 8, NCHW result
// where a thread works: lane l of the eight of pixel group g; the workgroup walks pixels [p0, p1) of the B H W, 32 at a time
struct RsHeadPos {
  int l, g;
  long p0, p1;
};
__device__ __forceinline__ RsHeadPos rs_head_pos(long M, long ppp) {
  RsHeadPos t;
  t.l = (int)threadIdx.x & 7;
  t.g = (int)threadIdx.x >> 3;
  t.p0 = (long)blockIdx.x * ppp;
  t.p1 = t.p0 + ppp < M ? t.p0 + ppp : M;
  return t;
}

// out [B, O, H, W] = sum_c x[p][c] w[o][c] + bias[o]: the workgroup copies w [O][C] to LDS once; every lane adds its four
// channels of each chunk in chunk order, the eight lanes of a pixel meet by xor-shuffles (4, 2, 1), lane o stores output o
template <int O>
__global__ __launch_bounds__(DN_BS) void rs_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ out, long M,
                                                            long HW, int C, int ldc, long ppp) {
  extern __shared__ float4 rs_w[];                               // [O][C / 4]
  const RsHeadPos t = rs_head_pos(M, ppp);
  const int nj = C / 32, Q = C / 4;
  for (int i = (int)threadIdx.x; i < O * Q; i += DN_BS) rs_w[i] = ld4(w + 4 * (size_t)i);
  __syncthreads();
  for (long p = t.p0 + t.g; p < t.p1; p += RS_HEAD_GROUPS) {     // (a pixel's eight lanes leave together: whole shuffles)
    const float* src = x + (size_t)p * ldc + 4 * t.l;
    float acc[O];
#pragma unroll
    for (int o = 0; o < O; ++o) acc[o] = 0.0f;
    for (int j = 0; j < nj; ++j) {
      const float4 a = ld4(src + 32 * j);
#pragma unroll
      for (int o = 0; o < O; ++o) {
        const float4 k = rs_w[o * Q + 8 * j + t.l];
        acc[o] += ((a.x * k.x + a.y * k.y) + a.z * k.z) + a.w * k.w;
      }
    }
#pragma unroll
    for (int o = 0; o < O; ++o) {
      acc[o] += __shfl_xor(acc[o], 4);
      acc[o] += __shfl_xor(acc[o], 2);
      acc[o] += __shfl_xor(acc[o], 1);
    }
    const long b = p / HW;
#pragma unroll
    for (int o = 0; o < O; ++o) {
      if (t.l == o) out[(b * O + o) * HW + (p - b * HW)] = acc[o] + bias[o];
    }
  }
}

// One row of workgroups per 32-channel chunk j = blockIdx.y of the padded pixel.  dx [p][32 j + 4 l ..] = sum_o dout[o][p]
// w[o][..] in o order (a padding chunk: zeros); part [blockIdx.x][o][C + 1] = this run's fp64 sums of dout[o][p] x[p][c]
// and, in the last column (chunk 0 writes it), of dout[o][p].
template <int O>
__global__ __launch_bounds__(DN_BS) void rs_head_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ x,
                                                            const float* __restrict__ w, double* __restrict__ part,
                                                            float* __restrict__ dx, long M, long HW, int C, int ldc, long ppp) {
  __shared__ double red[DN_BS / 64][8][O * 5];
  const RsHeadPos t = rs_head_pos(M, ppp);
  const int c0 = 32 * (int)blockIdx.y + 4 * t.l;
  if (c0 >= C) {                                                 // (uniform over the workgroup: C is a multiple of 32)
    for (long p = t.p0 + t.g; p < t.p1; p += RS_HEAD_GROUPS) st4z(dx + (size_t)p * ldc + c0);
    return;
  }
  float4 k[O];
#pragma unroll
  for (int o = 0; o < O; ++o) k[o] = ld4(w + (size_t)o * C + c0);
  double v[O * 5];
#pragma unroll
  for (int i = 0; i < O * 5; ++i) v[i] = 0.0;
  for (long p = t.p0 + t.g; p < t.p1; p += RS_HEAD_GROUPS) {
    const long b = p / HW;
    const float* dz = dout + b * O * HW + (p - b * HW);
    const float4 a = ld4(x + (size_t)p * ldc + c0);
    float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int o = 0; o < O; ++o) {
      const float z = dz[(size_t)o * HW];
      d.x += z * k[o].x; d.y += z * k[o].y; d.z += z * k[o].z; d.w += z * k[o].w;
      const double zd = (double)z;
      v[o * 5 + 0] += zd * (double)a.x; v[o * 5 + 1] += zd * (double)a.y;
      v[o * 5 + 2] += zd * (double)a.z; v[o * 5 + 3] += zd * (double)a.w;
      v[o * 5 + 4] += zd;
    }
    st4(dx + (size_t)p * ldc + c0, d.x, d.y, d.z, d.w);
  }
  // the eight pixel groups of a wave (same l: lanes 8 apart), then the four waves in order
#pragma unroll
  for (int i = 0; i < O * 5; ++i) {
    v[i] += __shfl_xor(v[i], 8);
    v[i] += __shfl_xor(v[i], 16);
    v[i] += __shfl_xor(v[i], 32);
  }
  const int wave = (int)threadIdx.x >> 6;
  if (((int)threadIdx.x & 63) < 8) {
#pragma unroll
    for (int i = 0; i < O * 5; ++i) red[wave][t.l][i] = v[i];
  }
  __syncthreads();
  if ((int)threadIdx.x < 8) {
    double* dst = part + (size_t)blockIdx.x * O * (C + 1);
#pragma unroll
    for (int o = 0; o < O; ++o) {
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int e = o * 5 + i;
        const double s = ((red[0][t.l][e] + red[1][t.l][e]) + red[2][t.l][e]) + red[3][t.l][e];
        if (i < 4) dst[(size_t)o * (C + 1) + c0 + i] = s;
        else if (blockIdx.y == 0 && t.l == 0) dst[(size_t)o * (C + 1) + C] = s;
      }
    }
  }
}
// dw [O][C], db [O] = the parts added in index order, four contiguous quarters of that order at a time
__global__ __launch_bounds__(256) void rs_head_bwd_final_kernel(const double* __restrict__ part, float* __restrict__ dw,
                                                                float* __restrict__ db, int nparts, int C, int O) {
  __shared__ double red[256];
  const int el = (int)threadIdx.x & 63, j = (int)threadIdx.x >> 6, e = (int)blockIdx.x * 64 + el, N = O * (C + 1);
  const int per = (nparts + 3) / 4, k0 = j * per, k1 = k0 + per < nparts ? k0 + per : nparts;
  double acc = 0.0;
  if (e < N) {
#pragma unroll 8
    for (int k = k0; k < k1; ++k) acc += part[(size_t)k * N + e];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (j == 0 && e < N) {
    const float s = (float)(((red[el] + red[64 + el]) + red[128 + el]) + red[192 + el]);
    const int o = e / (C + 1), c = e - o * (C + 1);
    if (c < C) dw[(size_t)o * C + c] = s;
    else db[o] = s;
  }
}

// pixels per part (a multiple of the 32 a workgroup holds) and the number of parts of M pixels
inline void rs_head_parts(long M, long& ppp, int& nparts) {
  ppp = (M + RS_HEAD_MAX_PARTS - 1) / RS_HEAD_MAX_PARTS;
  ppp = (ppp + RS_HEAD_GROUPS - 1) / RS_HEAD_GROUPS * RS_HEAD_GROUPS;
  nparts = (int)((M + ppp - 1) / ppp);
}
constexpr long RS_MAX_PIXELS = 1L << 36;      // of the small map, batch included: with ldc <= 2^16 no count below leaves int64
constexpr int RS_MAX_LDC = 1 << 16;
constexpr int RS_HEAD_MAX_C = 2048;           // the forward keeps w [O][C] in LDS: 64 KB at O = 8
inline bool rs_map_ok(int B, int H, int W, int C, int ldc) {
  return B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ldc >= C && ldc % 4 == 0 && ldc <= RS_MAX_LDC && H <= (1 << 20) &&
         W <= (1 << 20) && (long)H * W <= RS_MAX_PIXELS / B;
}
inline bool rs_head_ok(int B, int H, int W, int C, int ldc, int O) {
  return rs_map_ok(B, H, W, C, ldc) && C % 32 == 0 && ldc % 32 == 0 && C <= RS_HEAD_MAX_C && O >= 1 && O <= RS_HEAD_MAX_O;
}
inline unsigned rs_blocks(long n) { return (unsigned)((n + 255) / 256); }

#define RS_HEAD_DISPATCH(O, LAUNCH) \
  switch (O) {                      \
    case 1: LAUNCH(1); break;       \
    case 2: LAUNCH(2); break;       \
    case 3: LAUNCH(3); break;       \
    case 4: LAUNCH(4); break;       \
    case 5: LAUNCH(5); break;       \
    case 6: LAUNCH(6); break;       \
    case 7: LAUNCH(7); break;       \
    default: LAUNCH(8); break;      \
  }
}  // namespace

extern "C" int ld_dn_space_to_depth(const float* x, float* out, int B, int H, int W, int C, int ldc, void* stream) {
  LD_REQUIRE(rs_map_ok(B, H, W, C, ldc), "ld_dn_space_to_depth: B=%d H=%d W=%d C=%d ldc=%d (the output map; C and ldc >= C "
             "multiples of 4)", B, H, W, C, ldc);
  LD_REQUIRE(x && out, "ld_dn_space_to_depth: null pointer");
  LD_REQUIRE(dn_aligned16(x) && dn_aligned16(out), "ld_dn_space_to_depth: a pointer is not 16-byte aligned");
  const long n = (long)B * H * W * C;                      // 16-byte pieces of the output: 4 C / 4 per pixel
  LD_REQUIRE((n + 255) / 256 < (1L << 31), "ld_dn_space_to_depth: %ld pieces", n);
  LD_LAUNCH(rs_space_to_depth_kernel, dim3(rs_blocks(n)), dim3(256), 0, dn_st(stream), x, out, n, H, W, C, ldc);
  LD_LAUNCH_CHECK("dn_space_to_depth");
  return LD_OK;
}

extern "C" int ld_dn_depth_to_space(const float* g, float* dx, int B, int H, int W, int C, int ldc, void* stream) {
  LD_REQUIRE(rs_map_ok(B, H, W, C, ldc), "ld_dn_depth_to_space: B=%d H=%d W=%d C=%d ldc=%d (the input map; C and ldc >= C "
             "multiples of 4)", B, H, W, C, ldc);
  LD_REQUIRE(g && dx, "ld_dn_depth_to_space: null pointer");
  LD_REQUIRE(dn_aligned16(g) && dn_aligned16(dx), "ld_dn_depth_to_space: a pointer is not 16-byte aligned");
  const long n = (long)B * H * W * ldc;                    // 4 pixels of ldc / 4 pieces each
  LD_REQUIRE((n + 255) / 256 < (1L << 31), "ld_dn_depth_to_space: %ld pieces", n);
  LD_LAUNCH(rs_depth_to_space_kernel, dim3(rs_blocks(n)), dim3(256), 0, dn_st(stream), g, dx, n, H, W, C, ldc);
  LD_LAUNCH_CHECK("dn_depth_to_space");
  return LD_OK;
}

extern "C" int ld_dn_upsample2x(const float* x, float* out, int B, int H, int W, int C, int ldc, void* stream) {
  LD_REQUIRE(rs_map_ok(B, H, W, C, ldc), "ld_dn_upsample2x: B=%d H=%d W=%d C=%d ldc=%d (the input map; C and ldc >= C "
             "multiples of 4)", B, H, W, C, ldc);
  LD_REQUIRE(x && out, "ld_dn_upsample2x: null pointer");
  LD_REQUIRE(dn_aligned16(x) && dn_aligned16(out), "ld_dn_upsample2x: a pointer is not 16-byte aligned");
  const long n = (long)B * H * W * ldc;
  LD_REQUIRE((n + 255) / 256 < (1L << 31), "ld_dn_upsample2x: %ld pieces", n);
  LD_LAUNCH(rs_upsample2x_kernel, dim3(rs_blocks(n)), dim3(256), 0, dn_st(stream), x, out, n, H, W, C, ldc);
  LD_LAUNCH_CHECK("dn_upsample2x");
  return LD_OK;
}

extern "C" int ld_dn_upsample2x_backward(const float* g, float* dx, int B, int H, int W, int C, int ldc, void* stream) {
  LD_REQUIRE(rs_map_ok(B, H, W, C, ldc), "ld_dn_upsample2x_backward: B=%d H=%d W=%d C=%d ldc=%d (the map of dx; C and ldc >= C "
             "multiples of 4)", B, H, W, C, ldc);
  LD_REQUIRE(g && dx, "ld_dn_upsample2x_backward: null pointer");
  LD_REQUIRE(dn_aligned16(g) && dn_aligned16(dx), "ld_dn_upsample2x_backward: a pointer is not 16-byte aligned");
  const long n = (long)B * H * W * (ldc / 4);
  LD_REQUIRE((n + 255) / 256 < (1L << 31), "ld_dn_upsample2x_backward: %ld pieces", n);
  LD_LAUNCH(rs_upsample2x_bwd_kernel, dim3(rs_blocks(n)), dim3(256), 0, dn_st(stream), g, dx, n, H, W, C, ldc);
  LD_LAUNCH_CHECK("dn_upsample2x_backward");
  return LD_OK;
}

extern "C" int ld_dn_im2col(const float* x, float* out, int B, int Cin, int H, int W, int64_t sb, int64_t sc, int64_t sh,
                            int64_t sw, int ldk, void* stream) {
  LD_REQUIRE(B > 0 && H > 0 && W > 0 && Cin >= 1 && Cin <= 4 && ldk >= 49 * Cin && ldk % 4 == 0 && ldk <= RS_MAX_LDC &&
                 H <= (1 << 20) && W <= (1 << 20) && (long)H * W <= RS_MAX_PIXELS / B,
             "ld_dn_im2col: B=%d Cin=%d H=%d W=%d ldk=%d (Cin 1..4, ldk >= 49 Cin a multiple of 4)", B, Cin, H, W, ldk);
  LD_REQUIRE(sb >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "ld_dn_im2col: negative stride");
  LD_REQUIRE(x && out, "ld_dn_im2col: null pointer");
  LD_REQUIRE(dn_aligned16(out), "ld_dn_im2col: out is not 16-byte aligned");
  const long n = (long)B * H * W * (ldk / 4);
  LD_REQUIRE((n + 255) / 256 < (1L << 31), "ld_dn_im2col: %ld pieces", n);
  LD_LAUNCH(rs_im2col_kernel, dim3(rs_blocks(n)), dim3(256), 0, dn_st(stream), x, out, n, Cin, H, W, (long)sb, (long)sc, (long)sh,
            (long)sw, ldk);
  LD_LAUNCH_CHECK("dn_im2col");
  return LD_OK;
}

extern "C" int ld_dn_head_splits(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  long ppp;
  int nparts;
  rs_head_parts((long)B * H * W, ppp, nparts);
  return nparts;
}

extern "C" int64_t ld_dn_head_work_bytes(int B, int H, int W, int C, int O) {
  if (!rs_head_ok(B, H, W, C, C, O)) return 0;
  return (int64_t)ld_dn_head_splits(B, H, W) * O * (C + 1) * (int64_t)sizeof(double);
}

extern "C" int ld_dn_head_forward(const float* x, const float* w, const float* bias, float* out, int B, int H, int W, int C,
                                  int ldc, int O, void* stream) {
  LD_REQUIRE(rs_head_ok(B, H, W, C, ldc, O), "ld_dn_head_forward: B=%d H=%d W=%d C=%d ldc=%d O=%d (C and ldc >= C multiples of "
             "32, C <= 2048, O 1..8)", B, H, W, C, ldc, O);
  LD_REQUIRE(x && w && bias && out, "ld_dn_head_forward: null pointer");
  LD_REQUIRE(dn_aligned16(x) && dn_aligned16(w), "ld_dn_head_forward: x or w is not 16-byte aligned");
  const long HW = (long)H * W, M = (long)B * HW, ppp = 8 * RS_HEAD_GROUPS;
  LD_REQUIRE((M + ppp - 1) / ppp < (1L << 31), "ld_dn_head_forward: %ld pixels", M);
  const dim3 grid((unsigned)((M + ppp - 1) / ppp));
#define RS_FWD(N) \
  LD_LAUNCH(rs_head_fwd_kernel<N>, grid, dim3(DN_BS), (size_t)N * C * sizeof(float), dn_st(stream), x, w, bias, out, M, HW, C, ldc, ppp)
  RS_HEAD_DISPATCH(O, RS_FWD)
#undef RS_FWD
  LD_LAUNCH_CHECK("dn_head_forward");
  return LD_OK;
}

extern "C" int ld_dn_head_backward(const float* dout, const float* x, const float* w, double* work, float* dw, float* db,
                                   float* dx, int B, int H, int W, int C, int ldc, int O, void* stream) {
  LD_REQUIRE(rs_head_ok(B, H, W, C, ldc, O), "ld_dn_head_backward: B=%d H=%d W=%d C=%d ldc=%d O=%d (C and ldc >= C multiples of "
             "32, C <= 2048, O 1..8)", B, H, W, C, ldc, O);
  LD_REQUIRE(dout && x && w && work && dw && db && dx, "ld_dn_head_backward: null pointer");
  LD_REQUIRE(dn_aligned16(x) && dn_aligned16(w) && dn_aligned16(dx) && (reinterpret_cast<uintptr_t>(work) & 7) == 0,
             "ld_dn_head_backward: x, w or dx is not 16-byte aligned, or work not 8-byte aligned");
  const long HW = (long)H * W, M = (long)B * HW;
  long ppp;
  int nparts;
  rs_head_parts(M, ppp, nparts);
  hipStream_t st = dn_st(stream);
  const dim3 grid((unsigned)nparts, (unsigned)(ldc / 32));
#define RS_BWD(N) LD_LAUNCH(rs_head_bwd_kernel<N>, grid, dim3(DN_BS), 0, st, dout, x, w, work, dx, M, HW, C, ldc, ppp)
  RS_HEAD_DISPATCH(O, RS_BWD)
#undef RS_BWD
  LD_LAUNCH(rs_head_bwd_final_kernel, dim3((unsigned)((O * (C + 1) + 63) / 64)), dim3(256), 0, st, (const double*)work, dw, db,
            nparts, C, O);
  LD_LAUNCH_CHECK("dn_head_backward");
  return LD_OK;
}
