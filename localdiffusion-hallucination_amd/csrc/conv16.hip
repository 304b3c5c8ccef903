// The denoiser's training convolutions on the bf16 matrix cores (conv_precision = "bf16" of trainable.py): the three
// launches every trainable module's convolutions go through, with both operands of every product rounded to bf16
// (round-to-nearest-even, v_cvt_pk_bf16_f32) and multiplied by v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  What
// sits in memory does not change: activations and gradients are fp32 NHWC, the weight gradient is fp32.
//
//   * dn_conv16_kernel: ld_pc_conv's implicit GEMM (M = output pixels, N = output channels, K = taps x input channels;
//     stride 1) with a bf16 OHWI weight.  The fp32 activation tile is rounded on its way into LDS, the weight tile is
//     copied as it is; both are K-contiguous, so the LDS image is [row][32 k] bf16 and a lane's fragment (8 consecutive k
//     of row lane & 31, k offset 8 (lane >> 5)) is one ds_read_b128.  Rows are padded to 80 bytes: the 16 rows a
//     ds_read_b128 serves at a time start in 16 different 16-byte bank groups.  A 32-channel K-chunk is two MFMAs per
//     32 x 32 block; the next chunk's global loads sit in registers while the current one is multiplied (pc_gemm's
//     shape).  The data gradient is the same kernel on the flipped, transposed weight.
//   * dn_wgrad16_kernel: ld_seg_wgrad's implicit GEMM (rows = output channels, columns = input channels, K = pixels in
//     chunks of 32).  Both operands are channel-contiguous in memory and K is the pixel axis, so the loader writes the
//     tiles transposed, [channel][32 pixels] bf16: a thread loads four channels of two neighbouring pixels and stores
//     the four rounded pairs.  One slab of fp32 partial sums per split, added in index order by a second kernel (no
//     floating-point atomics: a step is reproducible bit for bit); a split without chunks writes a zero slab.
//   * dn_pack_conv16_kernel: an OIHW fp32 parameter to the two bf16 layouts in one launch, zero in the padded channels.
//
// The _from16 entry points (act_storage = "bf16") run the same two kernels on an activation that is ALREADY bf16 in memory
// (same NHWC shape, same pixel stride in elements): the loader copies where the fp32 one rounds, and everything behind it
// -- the LDS image, the MFMA order, the epilogue, the slabs -- is the same code, so the result is bit for bit that of the
// fp32 tensor which rounds to this one.  The convolution's loader takes 8 bf16 (16 bytes) of one pixel per thread, four
// threads a pixel's 32-channel chunk, and stores them with one ds_write_b128 (the weight tile's shape); the weight gradient's
// keeps its thread map (four channels of two neighbouring pixels, now two 8-byte loads) and pairs the halves of the two
// pixels' dwords for the same four transposed ds_write_b32.
//
// The _to16 entry points (conv_out_storage = "bf16") run the convolution with a bf16 OUTPUT (same NHWC shape, same pixel
// stride in elements): loader, LDS image, MFMA order and the epilogue's fp32 arithmetic are the same code, and the value is
// rounded to nearest even on its way out (pack_bf16x2), so the result is the fp32 kernel's, rounded.  In the 32x32x16 C/D
// layout a lane holds one channel of 16 pixels and its neighbour lane ^ 1 the next channel of the same pixels; the two swap
// eight values (one DPP quad_perm move each), so that the even lane holds both channels of its even rows and the odd lane
// both channels of its odd rows, and each stores eight dwords: half the store instructions of sixteen 2-byte stores, 64
// contiguous bytes per pixel row and half-wave parity either way.
//
// The _f16 entry points (amp = "fp16" of trainable.py) are the same three kernels with the operand format as a template
// parameter: the loader rounds to fp16 (pack_f16x2: v_cvt_pk_f16_f32, round-to-nearest-even; a value beyond 65504 becomes
// inf, it is NOT saturated -- the loss scaler of denoiser_opt.hip finds its overflows that way), the packed weights are fp16
// and the product is v_mfma_f32_32x32x16_f16.  Tiles, LDS image, chunk pipeline, epilogue and slab order are the code above;
// only the fp32-in / fp32-out forms exist.
#include <type_traits>

#include "common.hip.h"

namespace {
constexpr int CV_T = 64;        // tile: 64 rows x 64 columns per workgroup (4 waves, 2 x 2, 32 x 32 each)
constexpr int CV_KC = 32;       // K per chunk
constexpr int CV_LD = CV_KC + 8;   // bf16 per LDS row (80 bytes)
typedef __attribute__((ext_vector_type(16))) float cv_f32x16;
typedef unsigned short cv_bf16;    // the bits of a 16-bit operand (bf16, or fp16 in the F = f16 kernels)

// the operand format F of a kernel: how two fp32 values are rounded to a packed pair, and the MFMA that multiplies them
template <typename F> __device__ __forceinline__ unsigned cv_pack(float lo, float hi);
template <> __device__ __forceinline__ unsigned cv_pack<bf16>(float lo, float hi) { return pack_bf16x2(lo, hi); }
template <> __device__ __forceinline__ unsigned cv_pack<f16>(float lo, float hi) { return pack_f16x2(lo, hi); }
template <typename F> __device__ __forceinline__ cv_f32x16 cv_mfma(bf16x8 a, bf16x8 b, cv_f32x16 acc);
template <> __device__ __forceinline__ cv_f32x16 cv_mfma<bf16>(bf16x8 a, bf16x8 b, cv_f32x16 acc) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}
template <> __device__ __forceinline__ cv_f32x16 cv_mfma<f16>(bf16x8 a, bf16x8 b, cv_f32x16 acc) {   // (the same 16 bytes, read as fp16)
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
}

// the lane's fragment of K-step s (16 k) of a [row][CV_LD] image: 8 consecutive k of row `row`
__device__ __forceinline__ bf16x8 cv_frag(const cv_bf16 (*img)[CV_LD], int row, int s, int kh) {
  return *reinterpret_cast<const bf16x8*>(&img[row][s * 16 + 8 * kh]);
}

// ------------------------------------------------------------------------------------------------ convolution
// A16: a.src points at bf16 (8 per thread and chunk, one row) instead of fp32 (4 per thread and chunk, two rows)
// O16: a.out points at bf16; the epilogue's fp32 value is rounded to nearest even
// F: the operand format (bf16 or f16); A16 and O16 are bf16 storage and exist for F = bf16 only
template <typename F, bool A16, bool O16>
__global__ __launch_bounds__(256) void dn_conv16_kernel(ld_pc_conv_args a, const cv_bf16* __restrict__ w) {
  static_assert(std::is_same_v<F, bf16> || (!A16 && !O16), "16-bit storage is bf16");
  __shared__ __attribute__((aligned(16))) cv_bf16 sa[CV_T][CV_LD];   // [pixel][k]
  __shared__ __attribute__((aligned(16))) cv_bf16 sb[CV_T][CV_LD];   // [output channel][k]
  constexpr int UA = A16 ? 1 : CV_T / 32;
  using RA = std::conditional_t<A16, uint4, float4>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const long M = (long)a.B * a.Ho * a.Wo;
  const long p0 = (long)blockIdx.x * CV_T;
  const int n0 = blockIdx.y * CV_T;
  const int ks = a.ksize, pad = ks == 3 ? 1 : 0, nch = a.Cin / CV_KC, K = ks * ks * a.Cin;
  // activations: rows lr and lr + 32, 4 floats at k offset lk; in bf16 row lr, 8 bf16 at k offset lk
  const int lr = A16 ? tid >> 2 : tid >> 3, lk = A16 ? (tid & 3) * 8 : (tid & 7) * 4;
  const int wr = tid >> 2, wk = (tid & 3) * 8;       // weights: row wr, 8 bf16 at k offset wk
  int pb[UA], py[UA], px[UA];
  bool pv[UA];
#pragma unroll
  for (int u = 0; u < UA; ++u) {
    const long p = p0 + lr + 32 * u;
    pv[u] = p < M;
    const long pc = pv[u] ? p : 0;
    px[u] = (int)(pc % a.Wo);
    const long r = pc / a.Wo;
    py[u] = (int)(r % a.Ho);
    pb[u] = (int)(r / a.Ho);
  }
  auto fa = [&](int q, int u) {
    const int tap = q / nch, c0 = (q - tap * nch) * CV_KC;
    const int iy = py[u] - pad + tap / ks, ix = px[u] - pad + tap % ks;
    if constexpr (A16) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (pv[u] && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi)
        v = *reinterpret_cast<const uint4*>(reinterpret_cast<const cv_bf16*>(a.src) +
                                            (((long)pb[u] * a.Hi + iy) * a.Wi + ix) * a.Cin + c0 + lk);
      return v;
    } else {
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (pv[u] && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi)
        v = *reinterpret_cast<const float4*>(a.src + (((long)pb[u] * a.Hi + iy) * a.Wi + ix) * a.Cin + c0 + lk);
      return v;
    }
  };
  auto fb = [&](int q) { return *reinterpret_cast<const uint4*>(w + (long)(n0 + wr) * K + q * CV_KC + wk); };
  cv_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  RA ra[UA];
  uint4 rb;
#pragma unroll
  for (int u = 0; u < UA; ++u) ra[u] = fa(0, u);
  rb = fb(0);
  const int nq = ks * ks * nch;
  const int kh = lane >> 5, c = lane & 31;
  for (int q = 0; q < nq; ++q) {
    __syncthreads();                                  // the previous chunk's reads of the tiles are done
#pragma unroll
    for (int u = 0; u < UA; ++u) {
      if constexpr (A16) *reinterpret_cast<uint4*>(&sa[lr][lk]) = ra[u];
      else *reinterpret_cast<uint2*>(&sa[lr + 32 * u][lk]) = make_uint2(cv_pack<F>(ra[u].x, ra[u].y), cv_pack<F>(ra[u].z, ra[u].w));
    }
    *reinterpret_cast<uint4*>(&sb[wr][wk]) = rb;
    __syncthreads();
    if (q + 1 < nq) {
#pragma unroll
      for (int u = 0; u < UA; ++u) ra[u] = fa(q + 1, u);
      rb = fb(q + 1);
    }
#pragma unroll
    for (int s = 0; s < CV_KC / 16; ++s)
      acc = cv_mfma<F>(cv_frag(sa, wm * 32 + c, s, kh), cv_frag(sb, wn * 32 + c, s, kh), acc);
  }
  // C/D layout of 32x32x16: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int co = n0 + wn * 32 + c;
  const float sc = a.scale[co], t = a.shift[co];
  auto epi = [&](int r, long p) {                     // (p < M)
    float v = acc[r] * sc + t;
    if (a.residual) v += a.residual[p * a.Cout + co];
    if (a.relu) v = fmaxf(v, 0.0f);
    return v;
  };
  if constexpr (O16) {
    // rows 2 j and 2 j + 1 are neighbouring pixels: the even lane keeps 2 j, the odd lane 2 j + 1, each gets the other's
    // value of the row it keeps (every lane takes part in the exchange; only the loads and stores look at p < M)
    cv_bf16* out16 = reinterpret_cast<cv_bf16*>(a.out);
    const int odd = c & 1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long pe = p0 + wm * 32 + ((2 * j) & 3) + 8 * (j >> 1) + 4 * kh;      // row 2 j's pixel; row 2 j + 1's is pe + 1
      const float ve = pe < M ? epi(2 * j, pe) : 0.0f, vo = pe + 1 < M ? epi(2 * j + 1, pe + 1) : 0.0f;
      const float mine = odd ? vo : ve;
      const float theirs = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(odd ? ve : vo), 0xB1, 0xF, 0xF, true));
      const long p = pe + odd;
      if (p < M)
        *reinterpret_cast<unsigned*>(out16 + p * a.Cout + (co & ~1)) = odd ? pack_bf16x2(theirs, mine) : pack_bf16x2(mine, theirs);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long p = p0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
      if (p >= M) continue;
      a.out[p * a.Cout + co] = epi(r, p);
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct CvWgradDev {
  const float* dy; const void* a; float* work;      // a: fp32, or bf16 for the A16 kernel
  long M, nchunks;
  int H, W, Cin, Cout, ks, chunks_per_split;
};

// A16: d.a points at bf16; rb then holds the four channels of a pixel as two dwords of bf16 pairs (F = bf16 only)
template <typename F, bool A16>
__global__ __launch_bounds__(256) void dn_wgrad16_kernel(CvWgradDev d) {
  static_assert(std::is_same_v<F, bf16> || !A16, "16-bit storage is bf16");
  __shared__ __attribute__((aligned(16))) cv_bf16 sa[CV_T][CV_LD];   // [output channel][pixel of the chunk]
  __shared__ __attribute__((aligned(16))) cv_bf16 sb[CV_T][CV_LD];   // [input channel][pixel of the chunk]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int nci = d.Cin / CV_T;
  const int co0 = ((int)blockIdx.x / nci) * CV_T, ci0 = ((int)blockIdx.x % nci) * CV_T;
  const int tap = blockIdx.y, taps = d.ks * d.ks;
  const int oy = d.ks == 3 ? tap / 3 - 1 : 0, ox = d.ks == 3 ? tap % 3 - 1 : 0;
  const long c0 = (long)blockIdx.z * d.chunks_per_split;
  const long c1 = c0 + d.chunks_per_split < d.nchunks ? c0 + d.chunks_per_split : d.nchunks;
  const int lp = (tid >> 4) * 2, lc = (tid & 15) * 4;         // loader: pixels lp and lp + 1 of the chunk, 4 channels
  using RB = std::conditional_t<A16, uint2, float4>;
  float4 ra[2];
  RB rb[2];
  auto fetch = [&](long q) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long p = q * CV_KC + lp + u;
      ra[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if constexpr (A16) rb[u] = make_uint2(0u, 0u);
      else rb[u] = ra[u];
      if (p < d.M) {
        ra[u] = *reinterpret_cast<const float4*>(d.dy + p * d.Cout + co0 + lc);
        const int x = (int)(p % d.W), y = (int)((p / d.W) % d.H);
        const int yy = y + oy, xx = x + ox;
        if (yy >= 0 && yy < d.H && xx >= 0 && xx < d.W)        // same image: the shifted pixel is p + oy * W + ox
          rb[u] = *reinterpret_cast<const RB*>(static_cast<const std::conditional_t<A16, cv_bf16, float>*>(d.a) +
                                               (p + (long)oy * d.W + ox) * d.Cin + ci0 + lc);
      }
    }
  };
  cv_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  if (c0 < c1) fetch(c0);
  const int kh = lane >> 5, c = lane & 31;
  for (long q = c0; q < c1; ++q) {
    __syncthreads();                                          // the previous chunk's reads of the tiles are done
    *reinterpret_cast<unsigned*>(&sa[lc][lp]) = cv_pack<F>(ra[0].x, ra[1].x);
    *reinterpret_cast<unsigned*>(&sa[lc + 1][lp]) = cv_pack<F>(ra[0].y, ra[1].y);
    *reinterpret_cast<unsigned*>(&sa[lc + 2][lp]) = cv_pack<F>(ra[0].z, ra[1].z);
    *reinterpret_cast<unsigned*>(&sa[lc + 3][lp]) = cv_pack<F>(ra[0].w, ra[1].w);
    if constexpr (A16) {                                      // (low half: the even channel, and the first pixel of a pair)
      *reinterpret_cast<unsigned*>(&sb[lc][lp]) = (rb[0].x & 0xffffu) | (rb[1].x << 16);
      *reinterpret_cast<unsigned*>(&sb[lc + 1][lp]) = (rb[0].x >> 16) | (rb[1].x & 0xffff0000u);
      *reinterpret_cast<unsigned*>(&sb[lc + 2][lp]) = (rb[0].y & 0xffffu) | (rb[1].y << 16);
      *reinterpret_cast<unsigned*>(&sb[lc + 3][lp]) = (rb[0].y >> 16) | (rb[1].y & 0xffff0000u);
    } else {
      *reinterpret_cast<unsigned*>(&sb[lc][lp]) = cv_pack<F>(rb[0].x, rb[1].x);
      *reinterpret_cast<unsigned*>(&sb[lc + 1][lp]) = cv_pack<F>(rb[0].y, rb[1].y);
      *reinterpret_cast<unsigned*>(&sb[lc + 2][lp]) = cv_pack<F>(rb[0].z, rb[1].z);
      *reinterpret_cast<unsigned*>(&sb[lc + 3][lp]) = cv_pack<F>(rb[0].w, rb[1].w);
    }
    __syncthreads();
    if (q + 1 < c1) fetch(q + 1);
#pragma unroll
    for (int s = 0; s < CV_KC / 16; ++s)
      acc = cv_mfma<F>(cv_frag(sa, wm * 32 + c, s, kh), cv_frag(sb, wn * 32 + c, s, kh), acc);
  }
  // C/D layout of 32x32x16: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* slab = d.work + (long)blockIdx.z * d.Cout * taps * d.Cin;
  const int ci = ci0 + wn * 32 + c;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
    slab[((long)co * taps + tap) * d.Cin + ci] = acc[r];
  }
}

__global__ void dn_wgrad16_reduce_kernel(const float* __restrict__ work, float* dw, long n, int splits) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = work[i];
  for (int k = 1; k < splits; ++k) s += work[(long)k * n + i];
  dw[i] = s;
}

// ------------------------------------------------------------------------------------------------ weight packing
// One thread per pair of neighbouring elements of fwd [cop][kk][cip] (the first `half` threads) or of dgr [cip][kk][cop]
// with the taps flipped; w is OIHW [co][ci][kk].
template <typename F>
__global__ void dn_pack_conv16_kernel(const float* __restrict__ w, unsigned* fwd, unsigned* dgr, long half, int co, int cop, int ci,
                                      int cip, int kk) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * half) return;
  float v[2];
  if (i < half) {
    const long e = 2 * i;
    const int c = (int)(e % cip), t = (int)((e / cip) % kk), o = (int)(e / ((long)cip * kk));
#pragma unroll
    for (int j = 0; j < 2; ++j) v[j] = (o < co && c + j < ci) ? w[((long)o * ci + c + j) * kk + t] : 0.0f;
    fwd[i] = cv_pack<F>(v[0], v[1]);
  } else {
    const long e = 2 * (i - half);
    const int o = (int)(e % cop), t = kk - 1 - (int)((e / cop) % kk), c = (int)(e / ((long)cop * kk));
#pragma unroll
    for (int j = 0; j < 2; ++j) v[j] = (o + j < co && c < ci) ? w[((long)(o + j) * ci + c) * kk + t] : 0.0f;
    dgr[i - half] = cv_pack<F>(v[0], v[1]);
  }
}
}  // namespace

namespace {
// ld_dn_conv16 and its _from16 / _to16 forms: `name` is the entry point's, `a16` says what args->src points at, `o16` what
// args->out does, `fp16` the operand format (ld_dn_conv_f16: fp32 in, fp32 out only)
int cv_conv(const char* name, bool fp16, bool a16, bool o16, const ld_pc_conv_args* a, const void* weight_bf16, void* stream) {
  LD_REQUIRE(a, "%s: null args", name);
  LD_REQUIRE(a->ksize == 1 || a->ksize == 3, "%s: ksize %d (1 or 3)", name, a->ksize);
  LD_REQUIRE(a->stride == 1, "%s: stride %d (1 only)", name, a->stride);
  LD_REQUIRE(a->B > 0 && a->Hi > 0 && a->Wi > 0, "%s: empty input B=%d H=%d W=%d", name, a->B, a->Hi, a->Wi);
  LD_REQUIRE(a->Ho == a->Hi && a->Wo == a->Wi, "%s: output %dx%d does not match input %dx%d at stride 1", name, a->Ho, a->Wo,
             a->Hi, a->Wi);
  LD_REQUIRE(a->Cin > 0 && a->Cin % CV_KC == 0, "%s: Cin %d (a multiple of 32)", name, a->Cin);
  LD_REQUIRE(a->Cout > 0 && a->Cout % CV_T == 0, "%s: Cout %d (a multiple of 64)", name, a->Cout);
  LD_REQUIRE(a->src && weight_bf16 && a->scale && a->shift && a->out, "%s: null pointer", name);
  LD_REQUIRE(((uintptr_t)a->src | (uintptr_t)weight_bf16) % 16 == 0, "%s: src%s and weight must be 16-byte aligned", name,
             a16 ? " (bf16)" : "");
  if (o16) {                                          // the epilogue stores pairs of channels, and reads the residual after
    LD_REQUIRE((uintptr_t)a->out % 4 == 0, "%s: out (bf16) must be 4-byte aligned", name);
    LD_REQUIRE(static_cast<const void*>(a->residual) != static_cast<const void*>(a->out),
               "%s: residual (fp32) cannot alias out (bf16)", name);
  }
  const long M = (long)a->B * a->Ho * a->Wo;
  LD_REQUIRE((M + CV_T - 1) / CV_T < (1L << 31), "%s: %ld pixels", name, M);
  LD_REQUIRE((long)a->ksize * a->ksize * a->Cin < (1L << 31), "%s: K %ld", name, (long)a->ksize * a->ksize * a->Cin);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((M + CV_T - 1) / CV_T), (unsigned)(a->Cout / CV_T));
  const cv_bf16* w = reinterpret_cast<const cv_bf16*>(weight_bf16);
  if (fp16) {
    LD_LAUNCH((dn_conv16_kernel<f16, false, false>), grid, dim3(256), 0, st, *a, w);
  } else if (a16 && o16) {
    LD_LAUNCH((dn_conv16_kernel<bf16, true, true>), grid, dim3(256), 0, st, *a, w);
  } else if (a16) {
    LD_LAUNCH((dn_conv16_kernel<bf16, true, false>), grid, dim3(256), 0, st, *a, w);
  } else if (o16) {
    LD_LAUNCH((dn_conv16_kernel<bf16, false, true>), grid, dim3(256), 0, st, *a, w);
  } else {
    LD_LAUNCH((dn_conv16_kernel<bf16, false, false>), grid, dim3(256), 0, st, *a, w);
  }
  LD_LAUNCH_CHECK(name + 3);
  return LD_OK;
}

int cv_wgrad(const char* name, bool fp16, bool a16, const float* dy, const void* a, float* work, float* dw, int B, int H, int W, int Cin,
             int Cout, int ksize, int splits, void* stream) {
  LD_REQUIRE(ksize == 1 || ksize == 3, "%s: ksize %d (1 or 3)", name, ksize);
  LD_REQUIRE(B > 0 && H > 0 && W > 0, "%s: empty shape B=%d H=%d W=%d", name, B, H, W);
  LD_REQUIRE(Cin > 0 && Cin % CV_T == 0, "%s: Cin %d (a multiple of 64)", name, Cin);
  LD_REQUIRE(Cout > 0 && Cout % CV_T == 0, "%s: Cout %d (a multiple of 64)", name, Cout);
  const long M = (long)B * H * W, nchunks = (M + CV_KC - 1) / CV_KC;
  LD_REQUIRE(splits >= 1 && splits <= nchunks && splits <= 65535, "%s: splits %d (1..min(%ld, 65535))", name, splits, nchunks);
  const long tiles = (long)(Cin / CV_T) * (Cout / CV_T);
  LD_REQUIRE(tiles < (1L << 31), "%s: %ld tiles", name, tiles);
  LD_REQUIRE(dy && a && work && dw, "%s: null pointer", name);
  LD_REQUIRE(((uintptr_t)dy | (uintptr_t)a) % 16 == 0, "%s: dy and a%s must be 16-byte aligned", name, a16 ? " (bf16)" : "");
  const long per = (nchunks + splits - 1) / splits;
  CvWgradDev d{dy, a, work, M, nchunks, H, W, Cin, Cout, ksize, (int)per};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)tiles, (unsigned)(ksize * ksize), (unsigned)splits);
  if (fp16) {
    LD_LAUNCH((dn_wgrad16_kernel<f16, false>), grid, dim3(256), 0, st, d);
  } else if (a16) {
    LD_LAUNCH((dn_wgrad16_kernel<bf16, true>), grid, dim3(256), 0, st, d);
  } else {
    LD_LAUNCH((dn_wgrad16_kernel<bf16, false>), grid, dim3(256), 0, st, d);
  }
  const long n = (long)Cout * ksize * ksize * Cin;
  LD_LAUNCH(dn_wgrad16_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, work, dw, n, splits);
  LD_LAUNCH_CHECK(name + 3);
  return LD_OK;
}
}  // namespace

extern "C" int ld_dn_conv16(const ld_pc_conv_args* a, const void* weight_bf16, void* stream) {
  return cv_conv("ld_dn_conv16", false, false, false, a, weight_bf16, stream);
}

extern "C" int ld_dn_conv16_from16(const ld_pc_conv_args* a, const void* weight_bf16, void* stream) {
  return cv_conv("ld_dn_conv16_from16", false, true, false, a, weight_bf16, stream);
}

extern "C" int ld_dn_conv16_to16(const ld_pc_conv_args* a, const void* weight_bf16, void* stream) {
  return cv_conv("ld_dn_conv16_to16", false, false, true, a, weight_bf16, stream);
}

extern "C" int ld_dn_conv16_from16_to16(const ld_pc_conv_args* a, const void* weight_bf16, void* stream) {
  return cv_conv("ld_dn_conv16_from16_to16", false, true, true, a, weight_bf16, stream);
}

extern "C" int ld_dn_wgrad16(const float* dy, const float* a, float* work, float* dw, int B, int H, int W, int Cin, int Cout,
                             int ksize, int splits, void* stream) {
  return cv_wgrad("ld_dn_wgrad16", false, false, dy, a, work, dw, B, H, W, Cin, Cout, ksize, splits, stream);
}

extern "C" int ld_dn_wgrad16_from16(const float* dy, const void* a_bf16, float* work, float* dw, int B, int H, int W, int Cin,
                                    int Cout, int ksize, int splits, void* stream) {
  return cv_wgrad("ld_dn_wgrad16_from16", false, true, dy, a_bf16, work, dw, B, H, W, Cin, Cout, ksize, splits, stream);
}

namespace {
int cv_pack_conv(const char* name, bool fp16, const float* w_oihw, void* fwd16, void* dgr16, int co, int cop, int ci, int cip, int k,
                 void* stream) {
  LD_REQUIRE(k == 1 || k == 3, "%s: ksize %d (1 or 3)", name, k);
  LD_REQUIRE(co > 0 && ci > 0 && cop >= co && cip >= ci, "%s: co %d of %d, ci %d of %d", name, co, cop, ci, cip);
  LD_REQUIRE(cop % 2 == 0 && cip % 2 == 0, "%s: padded channels %d, %d (even)", name, cop, cip);
  LD_REQUIRE(w_oihw && fwd16 && dgr16, "%s: null pointer", name);
  LD_REQUIRE(((uintptr_t)fwd16 | (uintptr_t)dgr16) % 4 == 0, "%s: outputs must be 4-byte aligned", name);
  const long half = (long)cop * k * k * cip / 2;
  LD_REQUIRE((2 * half + 255) / 256 < (1L << 31), "%s: %ld elements", name, 2 * half);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((2 * half + 255) / 256));
  unsigned* fwd = reinterpret_cast<unsigned*>(fwd16);
  unsigned* dgr = reinterpret_cast<unsigned*>(dgr16);
  if (fp16) {
    LD_LAUNCH(dn_pack_conv16_kernel<f16>, grid, dim3(256), 0, st, w_oihw, fwd, dgr, half, co, cop, ci, cip, k * k);
  } else {
    LD_LAUNCH(dn_pack_conv16_kernel<bf16>, grid, dim3(256), 0, st, w_oihw, fwd, dgr, half, co, cop, ci, cip, k * k);
  }
  LD_LAUNCH_CHECK(name + 3);
  return LD_OK;
}
}  // namespace

extern "C" int ld_dn_pack_conv16(const float* w_oihw, void* fwd_bf16, void* dgr_bf16, int co, int cop, int ci, int cip, int k,
                                 void* stream) {
  return cv_pack_conv("ld_dn_pack_conv16", false, w_oihw, fwd_bf16, dgr_bf16, co, cop, ci, cip, k, stream);
}

// ------------------------------------------------------------------------------------------------ fp16 operands (amp = "fp16")
extern "C" int ld_dn_conv_f16(const ld_pc_conv_args* a, const void* weight_f16, void* stream) {
  return cv_conv("ld_dn_conv_f16", true, false, false, a, weight_f16, stream);
}

extern "C" int ld_dn_wgrad_f16(const float* dy, const float* a, float* work, float* dw, int B, int H, int W, int Cin, int Cout,
                               int ksize, int splits, void* stream) {
  return cv_wgrad("ld_dn_wgrad_f16", true, false, dy, a, work, dw, B, H, W, Cin, Cout, ksize, splits, stream);
}

extern "C" int ld_dn_pack_conv_f16(const float* w_oihw, void* fwd_f16, void* dgr_f16, int co, int cop, int ci, int cip, int k,
                                   void* stream) {
  return cv_pack_conv("ld_dn_pack_conv_f16", true, w_oihw, fwd_f16, dgr_f16, co, cop, ci, cip, k, stream);
}
