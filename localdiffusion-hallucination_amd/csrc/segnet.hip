// Segmentation U-Net (unet_model.py:140-243, bilinear=False): the OOD-mask producer that test.py:214-221, 284-289 runs on
// the conditioning image before sample(..., mask=...).  Every DoubleConv convolution is conv3x3 (no bias) -> BatchNorm2d
// (eval) -> ReLU; the BatchNorm is an fp32 epilogue on the fp32 accumulator, out = relu(acc * s[c] + t[c]) with
// s = gamma / sqrt(var + eps), t = beta - mean * s made by the host from the running statistics (the weights are NOT
// scaled: the reference applies BN after the convolution).  Every stored tensor is post-activation, so the consumers
// need no normalising prologue:
//   * Down (unet_model.py:170-180): the first convolution reads its input through a 2x2 max-pool (exact in every type);
//   * Up (:183-206): ConvTranspose2d(k=2, s=2) is a 1x1 GEMM to 4*Cout channels in (p1, p2, c) order, and the first
//     convolution of the DoubleConv reads cat([skip, depth_to_space(that)]) directly;
//   * inc (:224): a direct 3x3 convolution from the NCHW fp32 image (Cin 1 or 3) to 64 channels;
//   * outc (:209-215): a 1x1 convolution to one class, NCHW fp32 logits and optionally sigmoid / (p > 0.5).
// This file is separate from the diffusion path's convolutions: none of their kernels or routing is involved.
//
// ld_seg_conv is an implicit GEMM on the vector ALU in fp32: M = pixels (64 per workgroup), N = output channels (64 per
// workgroup), K = taps x input channels in chunks of 32.  256 threads, each owning a 4-pixel x 4-channel block of the
// tile; the next chunk's global loads are issued before the current chunk's FMAs.  Activations are NHWC in the storage
// dtype, converted to fp32 on load; weights are fp32 [tap][Cin][Cout] (ld_seg_pack_weight / ld_seg_pack_convt).
#include "common.hip.h"

namespace {
constexpr int SEG_TM = 64;      // pixels per workgroup
constexpr int SEG_TN = 64;      // output channels per workgroup
constexpr int SEG_KC = 32;      // input channels per K-chunk

struct SegConvDev {
  const void* src0; const void* src1;
  const float* weight; const float* scale; const float* shift;
  void* out;
  int C0, C1, B, H, W, Cout, relu;
};

// 8 consecutive channels as they sit in memory (one 16-byte load per 16 bytes): loaded from an always-valid address and
// converted only where the value is written to LDS, so the loads of the next chunk are in flight during this chunk's FMAs
// (a conversion inside the `if (in range)` branch would wait for the load right there).
template <typename T> struct Raw8 { uint4 r[sizeof(T) / 2]; };
template <typename T>
__device__ __forceinline__ void load_raw8(const T* p, Raw8<T>& o) {
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 2); ++i) o.r[i] = reinterpret_cast<const uint4*>(p)[i];
}
template <typename T>
__device__ __forceinline__ void unpack8(const Raw8<T>& o, float* v) {
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 2); ++i) unpack16<T>(o.r[i], v + i * DT<T>::E);
}

// Address of channels [c, c+8) of the logical input at pixel (b, y, x), in range; for the pooled source the first of the
// four stored pixels (the others are +C0, +2W*C0, +(2W+1)*C0)
template <typename T, int MODE>
__device__ __forceinline__ const T* src_addr(const SegConvDev& a, int b, int y, int x, int c) {
  if constexpr (MODE == LD_SEG_SRC_PLAIN) {
    return static_cast<const T*>(a.src0) + (((long)b * a.H + y) * a.W + x) * a.C0 + c;
  } else if constexpr (MODE == LD_SEG_SRC_POOL) {             // src0 is [B, 2H, 2W, C0]
    return static_cast<const T*>(a.src0) + (((long)b * 2 * a.H + 2 * y) * (2L * a.W) + 2 * x) * a.C0 + c;
  } else {                                                    // LD_SEG_SRC_CAT_D2S: cat([src0, depth_to_space(src1)])
    if (c < a.C0) return static_cast<const T*>(a.src0) + (((long)b * a.H + y) * a.W + x) * a.C0 + c;
    const int Hl = a.H >> 1, Wl = a.W >> 1;                   // src1 is [B, H/2, W/2, 4*C1], channel (p1, p2, c) order
    const long pix = ((long)b * Hl + (y >> 1)) * Wl + (x >> 1);
    const int ch = (((y & 1) << 1) | (x & 1)) * a.C1 + (c - a.C0);
    return static_cast<const T*>(a.src1) + pix * 4 * a.C1 + ch;
  }
}

template <typename T, int KS, int MODE>
__global__ __launch_bounds__(256) void seg_conv_kernel(SegConvDev a) {
  __shared__ __attribute__((aligned(16))) float As[SEG_KC][SEG_TM + 4];   // [k][pixel]
  __shared__ __attribute__((aligned(16))) float Bs[SEG_KC][SEG_TN];       // [k][output channel]
  const int tid = threadIdx.x;
  const long M = (long)a.B * a.H * a.W;
  const long p0 = (long)blockIdx.x * SEG_TM;
  const int n0 = blockIdx.y * SEG_TN;
  const int Cin = a.C0 + a.C1, nch = Cin / SEG_KC, nq = KS * KS * nch;
  // loader roles: activations -- pixel lp, channels [lc, lc+8); weights -- row wk, columns [wn, wn+8)
  const int lp = tid >> 2, lc = (tid & 3) * 8;
  const int wk = tid >> 3, wn = (tid & 7) * 8;
  const long gp = p0 + lp;
  const bool pvalid = gp < M;
  int b = 0, y = 0, x = 0;
  if (pvalid) {
    x = (int)(gp % a.W);
    const long r = gp / a.W;
    y = (int)(r % a.H);
    b = (int)(r / a.H);
  }
  constexpr int NP = MODE == LD_SEG_SRC_POOL ? 4 : 1;        // stored pixels per logical input pixel
  Raw8<T> araw[NP];
  bool aval = false;
  float bv[8];
  auto fetch = [&](int q) {
    const int tap = q / nch, c0 = (q - tap * nch) * SEG_KC;
    const int yy = y + (KS == 3 ? tap / 3 - 1 : 0), xx = x + (KS == 3 ? tap % 3 - 1 : 0);
    aval = pvalid && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
    const T* p = src_addr<T, MODE>(a, b, aval ? yy : 0, aval ? xx : 0, c0 + lc);
    load_raw8<T>(p, araw[0]);
    if constexpr (NP == 4) {
      const long W2 = 2L * a.W;
      load_raw8<T>(p + a.C0, araw[1]);
      load_raw8<T>(p + W2 * a.C0, araw[2]);
      load_raw8<T>(p + (W2 + 1) * a.C0, araw[3]);
    }
    const float* wp = a.weight + ((long)tap * Cin + c0 + wk) * a.Cout + n0 + wn;
    const float4 w0 = *reinterpret_cast<const float4*>(wp), w1 = *reinterpret_cast<const float4*>(wp + 4);
    bv[0] = w0.x; bv[1] = w0.y; bv[2] = w0.z; bv[3] = w0.w;
    bv[4] = w1.x; bv[5] = w1.y; bv[6] = w1.z; bv[7] = w1.w;
  };
  // compute role: pixels [ty*4, ty*4+4), output channels [tx*4, tx*4+4) of the tile
  const int tx = tid & 15, ty = tid >> 4;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
  fetch(0);
  for (int q = 0; q < nq; ++q) {
    __syncthreads();                                          // the previous chunk's reads of As / Bs are done
    float av[8];
    unpack8<T>(araw[0], av);
#pragma unroll
    for (int k = 1; k < NP; ++k) {                            // 2x2 max-pool: exact in every storage type
      float o[8];
      unpack8<T>(araw[k], o);
#pragma unroll
      for (int i = 0; i < 8; ++i) av[i] = fmaxf(av[i], o[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) As[lc + i][lp] = aval ? av[i] : 0.0f;
    *reinterpret_cast<float4*>(&Bs[wk][wn]) = make_float4(bv[0], bv[1], bv[2], bv[3]);
    *reinterpret_cast<float4*>(&Bs[wk][wn + 4]) = make_float4(bv[4], bv[5], bv[6], bv[7]);
    __syncthreads();
    if (q + 1 < nq) fetch(q + 1);
#pragma unroll 8
    for (int k = 0; k < SEG_KC; ++k) {
      const float4 pa = *reinterpret_cast<const float4*>(&As[k][ty * 4]);
      const float4 pb = *reinterpret_cast<const float4*>(&Bs[k][tx * 4]);
      const float ra[4] = {pa.x, pa.y, pa.z, pa.w}, rb[4] = {pb.x, pb.y, pb.z, pb.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ra[i], rb[j], acc[i][j]);
    }
  }
  const int co = n0 + tx * 4;
  float s[4], t[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s[j] = a.scale ? a.scale[co + j] : 1.0f;
    t[j] = a.shift ? a.shift[co + j] : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long p = p0 + ty * 4 + i;
    if (p >= M) break;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = (a.scale ? acc[i][j] * s[j] : acc[i][j]) + t[j];
      if (a.relu) v[j] = fmaxf(v[j], 0.0f);
    }
    store4<T>(static_cast<T*>(a.out) + p * a.Cout + co, v);
  }
}

// inc's first convolution: NCHW fp32 image [B, Cin <= 3, H, W] -> NHWC [B, H, W, 64], BN + ReLU epilogue.
// One thread per pixel; the 64 x Cin x 9 weights sit in LDS as [Cin*9][64].
template <typename T>
__global__ __launch_bounds__(256) void seg_conv_image_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             T* out, int B, int Cin, int H, int W) {
  __shared__ __attribute__((aligned(16))) float ws[3 * 9][64];
  for (int i = threadIdx.x; i < 64 * Cin * 9; i += blockDim.x) {
    const int co = i / (Cin * 9), k = i - co * Cin * 9;     // w is OIHW: [co][ci][ky][kx] = [co][k]
    ws[k][co] = w[i];
  }
  __syncthreads();
  const long M = (long)B * H * W;
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= M) return;
  const int xx = (int)(p % W);
  const long r = p / W;
  const int yy = (int)(r % H), b = (int)(r / H);
  float acc[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) acc[c] = 0.0f;
  for (int ci = 0; ci < Cin; ++ci) {
    const float* xp = x + ((long)b * Cin + ci) * H * W;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int sy = yy + tap / 3 - 1, sx = xx + tap % 3 - 1;
      const float v = (sy >= 0 && sy < H && sx >= 0 && sx < W) ? xp[(long)sy * W + sx] : 0.0f;
      const float* wr = ws[ci * 9 + tap];
#pragma unroll
      for (int c = 0; c < 64; c += 4) {
        const float4 wv = *reinterpret_cast<const float4*>(wr + c);
        acc[c] = fmaf(v, wv.x, acc[c]);
        acc[c + 1] = fmaf(v, wv.y, acc[c + 1]);
        acc[c + 2] = fmaf(v, wv.z, acc[c + 2]);
        acc[c + 3] = fmaf(v, wv.w, acc[c + 3]);
      }
    }
  }
  T* op = out + p * 64;
#pragma unroll
  for (int c = 0; c < 64; c += 4) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaxf(acc[c + j] * scale[c + j] + shift[c + j], 0.0f);
    store4<T>(op + c, v);
  }
}

// outc: NHWC [B, H, W, C] -> logits [B, 1, H, W] fp32 (= pixel order), optional sigmoid and (p > 0.5) as nn.Sigmoid / test.py:287
template <typename T>
__global__ __launch_bounds__(256) void seg_head_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* logits, float* prob,
                                                       float* mask, long M, int C) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= M) return;
  const T* xp = x + p * C;
  float acc = 0.0f;
  for (int c = 0; c < C; c += 4) {
    float v[4];
    load4<T>(xp + c, v);
    const float4 wv = *reinterpret_cast<const float4*>(w + c);
    acc = fmaf(v[0], wv.x, acc);
    acc = fmaf(v[1], wv.y, acc);
    acc = fmaf(v[2], wv.z, acc);
    acc = fmaf(v[3], wv.w, acc);
  }
  const float l = acc + bias[0];
  if (logits) logits[p] = l;
  const float s = 1.0f / (1.0f + expf(-l));
  if (prob) prob[p] = s;
  if (mask) mask[p] = s > 0.5f ? 1.0f : 0.0f;
}

__global__ void seg_pack_weight_kernel(const float* __restrict__ w, float* out, int cout, int cin, int taps) {
  const long total = (long)cout * cin * taps;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int co = (int)(i % cout);                           // out [tap][ci][co] <- w [co][ci][tap]
  const long r = i / cout;
  const int ci = (int)(r % cin), tap = (int)(r / cin);
  out[i] = w[((long)co * cin + ci) * taps + tap];
}

__global__ void seg_pack_convt_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* w_out,
                                      float* bias_out, int cin, int cout) {
  const long total = (long)cin * 4 * cout;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int n = (int)(i % (4 * cout)), ci = (int)(i / (4 * cout));
  const int pp = n / cout, c = n - pp * cout;              // w_out [ci][(p1, p2, c)] <- w [ci][c][p1][p2]
  w_out[i] = w[((long)ci * cout + c) * 4 + pp];
  if (ci == 0) bias_out[n] = bias ? bias[c] : 0.0f;
}

template <typename T, int KS, int MODE>
int launch_seg_conv(const SegConvDev& d, hipStream_t st) {
  const long M = (long)d.B * d.H * d.W;
  const dim3 grid((unsigned)((M + SEG_TM - 1) / SEG_TM), (unsigned)(d.Cout / SEG_TN));
  LD_LAUNCH((seg_conv_kernel<T, KS, MODE>), grid, dim3(256), 0, st, d);
  return 0;
}
}  // namespace

extern "C" int ld_seg_conv(const ld_seg_conv_args* a, void* stream) {
  LD_REQUIRE(a, "ld_seg_conv: null args");
  LD_REQUIRE(ld_dtype_ok(a->dtype), "ld_seg_conv: bad dtype %d", a->dtype);
  LD_REQUIRE(a->ksize == 1 || a->ksize == 3, "ld_seg_conv: ksize %d (1 or 3)", a->ksize);
  LD_REQUIRE(a->mode == LD_SEG_SRC_PLAIN || a->mode == LD_SEG_SRC_POOL || a->mode == LD_SEG_SRC_CAT_D2S,
             "ld_seg_conv: source mode %d", a->mode);
  LD_REQUIRE(a->ksize == 3 || a->mode == LD_SEG_SRC_PLAIN, "ld_seg_conv: ksize 1 takes a plain source only");
  LD_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "ld_seg_conv: empty shape B=%d H=%d W=%d", a->B, a->H, a->W);
  LD_REQUIRE(a->mode != LD_SEG_SRC_CAT_D2S || (a->H % 2 == 0 && a->W % 2 == 0),
             "ld_seg_conv: depth-to-space source needs even H, W (%d, %d)", a->H, a->W);
  LD_REQUIRE(a->Cout > 0 && a->Cout % SEG_TN == 0, "ld_seg_conv: Cout %d (a multiple of 64)", a->Cout);
  LD_REQUIRE(a->C0 > 0 && a->C0 % SEG_KC == 0, "ld_seg_conv: C0 %d (a multiple of 32)", a->C0);
  LD_REQUIRE(a->mode == LD_SEG_SRC_CAT_D2S ? (a->C1 > 0 && a->C1 % SEG_KC == 0) : a->C1 == 0,
             "ld_seg_conv: C1 %d (a multiple of 32 with the concatenated source, else 0)", a->C1);
  LD_REQUIRE(a->src0 && a->weight && a->out && (a->mode != LD_SEG_SRC_CAT_D2S || a->src1), "ld_seg_conv: null pointer");
  const long M = (long)a->B * a->H * a->W;
  LD_REQUIRE((M + SEG_TM - 1) / SEG_TM < (1L << 31), "ld_seg_conv: %ld pixels", M);
  SegConvDev d{a->src0, a->src1, a->weight, a->scale, a->shift, a->out, a->C0, a->C1, a->B, a->H, a->W, a->Cout,
               a->relu ? 1 : 0};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_DISPATCH(a->dtype, [&] {
    if (a->ksize == 1) return launch_seg_conv<T, 1, LD_SEG_SRC_PLAIN>(d, st);
    if (a->mode == LD_SEG_SRC_POOL) return launch_seg_conv<T, 3, LD_SEG_SRC_POOL>(d, st);
    if (a->mode == LD_SEG_SRC_CAT_D2S) return launch_seg_conv<T, 3, LD_SEG_SRC_CAT_D2S>(d, st);
    return launch_seg_conv<T, 3, LD_SEG_SRC_PLAIN>(d, st);
  }());
  LD_LAUNCH_CHECK("seg_conv");
  return LD_OK;
}

extern "C" int ld_seg_conv_image(const float* x_nchw, const float* w_oihw, const float* scale, const float* shift, void* out,
                                 int B, int Cin, int H, int W, int dtype, void* stream) {
  LD_REQUIRE(ld_dtype_ok(dtype), "ld_seg_conv_image: bad dtype %d", dtype);
  LD_REQUIRE(Cin == 1 || Cin == 3, "ld_seg_conv_image: Cin %d (1 or 3)", Cin);
  LD_REQUIRE(B > 0 && H > 0 && W > 0, "ld_seg_conv_image: empty shape B=%d H=%d W=%d", B, H, W);
  LD_REQUIRE(x_nchw && w_oihw && scale && shift && out, "ld_seg_conv_image: null pointer");
  const long M = (long)B * H * W;
  LD_REQUIRE((M + 255) / 256 < (1L << 31), "ld_seg_conv_image: %ld pixels", M);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_DISPATCH(dtype, [&] {
    LD_LAUNCH(seg_conv_image_kernel<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, x_nchw, w_oihw, scale, shift,
              (T*)out, B, Cin, H, W);
    return 0;
  }());
  LD_LAUNCH_CHECK("seg_conv_image");
  return LD_OK;
}

extern "C" int ld_seg_head(const void* x, const float* w, const float* bias, float* logits, float* prob, float* mask,
                           int B, int H, int W, int C, int dtype, void* stream) {
  LD_REQUIRE(ld_dtype_ok(dtype), "ld_seg_head: bad dtype %d", dtype);
  LD_REQUIRE(C > 0 && C % 4 == 0, "ld_seg_head: C %d (a multiple of 4)", C);
  LD_REQUIRE(B > 0 && H > 0 && W > 0, "ld_seg_head: empty shape B=%d H=%d W=%d", B, H, W);
  LD_REQUIRE(x && w && bias && (logits || prob || mask), "ld_seg_head: null pointer");
  const long M = (long)B * H * W;
  LD_REQUIRE((M + 255) / 256 < (1L << 31), "ld_seg_head: %ld pixels", M);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_DISPATCH(dtype, [&] {
    LD_LAUNCH(seg_head_kernel<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (const T*)x, w, bias, logits, prob,
              mask, M, C);
    return 0;
  }());
  LD_LAUNCH_CHECK("seg_head");
  return LD_OK;
}

extern "C" int ld_seg_pack_weight(const float* w_oihw, float* out, int cout, int cin, int ksize, void* stream) {
  LD_REQUIRE(w_oihw && out, "ld_seg_pack_weight: null pointer");
  LD_REQUIRE(ksize == 1 || ksize == 3, "ld_seg_pack_weight: ksize %d", ksize);
  LD_REQUIRE(cout > 0 && cin > 0, "ld_seg_pack_weight: cout %d cin %d", cout, cin);
  const long total = (long)cout * cin * ksize * ksize;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(seg_pack_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w_oihw, out, cout, cin,
            ksize * ksize);
  LD_LAUNCH_CHECK("seg_pack_weight");
  return LD_OK;
}

extern "C" int ld_seg_pack_convt(const float* w, const float* bias, float* w_out, float* bias_out, int cin, int cout,
                                 void* stream) {
  LD_REQUIRE(w && w_out && bias_out, "ld_seg_pack_convt: null pointer");
  LD_REQUIRE(cout > 0 && cin > 0, "ld_seg_pack_convt: cout %d cin %d", cout, cin);
  const long total = (long)cin * 4 * cout;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(seg_pack_convt_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, bias, w_out, bias_out, cin,
            cout);
  LD_LAUNCH_CHECK("seg_pack_convt");
  return LD_OK;
}
