// The real / hallucinated gate of fusion() (Classifier_PatchCore, models.py:257-430): what surrounds PatchCore when it
// scores the fused x0 inside the reverse loop.  Three small memory-bound kernels replace the five eager ops and the two
// host round trips (`hr.max() > 1.0`, `pred_score > threshold`) of models.py:404-430:
//
//   * clf_max_kernel: the max of the whole tensor (or of each sample), wave64 shuffles -> LDS -> one atomicMax per
//     workgroup on an order-preserving uint32 code (enc_max; 0 is the identity), left in device memory;
//   * clf_resize_kernel: torch's bilinear resize (align_corners=False, no antialiasing) of an NCHW fp32 tensor with an
//     optional input transform (halving decided by that max, or the MRI de-normalisation), a C = 1 input read three
//     times instead of repeated, and the ImageNet Normalize per output channel: x0 -> ld_pc_stem's input in one launch.
//     The same kernel without transforms resizes the anomaly map back to the image size;
//   * the decision pred_score[b] > threshold -> int32, on its own (clf_decide_kernel) or in workgroup 0 of the resize.
//
// The max word is never zeroed by a launch of its own: a plan owns two sets of words, call i accumulates into set
// i & 1 and its resize launch zeroes the other set, which the resize of call i - 1 (earlier on the same stream) was
// the last to read.
//
// Arithmetic follows torch op by op (no contraction: -ffp-contract=off), so the distance to an exact evaluation is the
// reference's own: the source coordinate scale * (dst + 0.5) - 0.5 in fp32, h0 * (w0 * p00 + w1 * p01) + h1 * (...),
// (v - mean) / std with an IEEE division.
#include "common.hip.h"

namespace {
constexpr int CLF_MAX_WGS = 64;      // workgroups per reduced group at most: 3 * 256^2 floats = 48 float4 per thread

// torch's bilinear source index (align_corners=False): i0, i1 and the weights l0, l1 of output index o
__device__ __forceinline__ void clf_lin(int o, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
  float real = scale * ((float)o + 0.5f) - 0.5f;
  if (real < 0.0f) real = 0.0f;
  i0 = min((int)real, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = real - (float)i0;
  l0 = 1.0f - l1;
}

// max over group g = blockIdx.y of x [groups, n]; words[g] holds enc_max of it after the last workgroup
__global__ __launch_bounds__(256) void clf_max_kernel(const float* __restrict__ x, long n, unsigned* words) {
  __shared__ float part[4];
  const float* p = x + (long)blockIdx.y * n;
  const long stride = (long)gridDim.x * blockDim.x;
  float m = -INFINITY;
  if ((reinterpret_cast<size_t>(p) & 15) == 0) {                 // (uniform) 16-byte loads; the tail one by one
    const long n4 = n >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(p);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      const float4 v = p4[i];
      m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) m = fmaxf(m, p[i]);
  } else {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) m = fmaxf(m, p[i]);
  }
  for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomic_max_enc(&words[blockIdx.y], fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3])));
}

struct ClfResize {
  const float* x;            // [B, Cin, Hi, Wi]
  float* out;                // [B, Cout, Ho, Wo]
  int B, Cin, Cout, Hi, Wi, Ho, Wo;
  int mode;                  // LD_CLF_PLAIN / LD_CLF_HALVE / LD_CLF_AFFINE
  const unsigned* max_words; // HALVE: enc_max words, one per sample (per_sample) or one for the tensor
  int per_sample;
  unsigned* zero_words;      // words to zero for the next call, or NULL
  int n_zero;
  float sub, mul, add, div;  // AFFINE: ((v - sub) * mul + add) / div
  int normalize;             // (v - mean[c]) / std[c] per output channel
  float mean[3], std[3];
  const float* pred;         // decision: pred[b] > threshold -> decision[b]; or NULL
  float threshold;
  int32_t* decision;
  int n_decision;
};

// one thread per 4 consecutive output pixels of a row (the last group of a row may be shorter)
__global__ __launch_bounds__(256) void clf_resize_kernel(const ClfResize a) {
  if (blockIdx.x == 0) {                                          // (uniform) the side jobs of the launch
    for (int i = threadIdx.x; i < a.n_zero; i += blockDim.x) a.zero_words[i] = 0u;
    if (a.pred)
      for (int i = threadIdx.x; i < a.n_decision; i += blockDim.x) a.decision[i] = a.pred[i] > a.threshold ? 1 : 0;
  }
  const int wq = (a.Wo + 3) >> 2;
  const long total = (long)a.B * a.Cout * a.Ho * wq;
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= total) return;
  const int xq = (int)(id % wq);
  const int y = (int)((id / wq) % a.Ho);
  const int c = (int)((id / ((long)wq * a.Ho)) % a.Cout);
  const int b = (int)(id / ((long)wq * a.Ho * a.Cout));
  const float* src = a.x + ((long)b * a.Cin + (a.Cin == 1 ? 0 : c)) * a.Hi * a.Wi;
  float halve = 1.0f;
  if (a.mode == LD_CLF_HALVE) halve = dec_max(a.max_words[a.per_sample ? b : 0]) > 1.0f ? 0.5f : 1.0f;
  const float sy = (float)a.Hi / (float)a.Ho, sx = (float)a.Wi / (float)a.Wo;
  int y0, y1;
  float hy0, hy1;
  clf_lin(y, a.Hi, sy, y0, y1, hy0, hy1);
  const float* r0 = src + (long)y0 * a.Wi;
  const float* r1 = src + (long)y1 * a.Wi;
  const int xb = xq * 4;
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int x = min(xb + e, a.Wo - 1);                          // (a short last group recomputes the last pixel)
    int x0, x1;
    float wx0, wx1;
    clf_lin(x, a.Wi, sx, x0, x1, wx0, wx1);
    float p00 = r0[x0], p01 = r0[x1], p10 = r1[x0], p11 = r1[x1];
    if (a.mode == LD_CLF_AFFINE) {
      p00 = ((p00 - a.sub) * a.mul + a.add) / a.div;
      p01 = ((p01 - a.sub) * a.mul + a.add) / a.div;
      p10 = ((p10 - a.sub) * a.mul + a.add) / a.div;
      p11 = ((p11 - a.sub) * a.mul + a.add) / a.div;
    }
    float r = hy0 * (wx0 * p00 + wx1 * p01) + hy1 * (wx0 * p10 + wx1 * p11);
    r *= halve;                                                   // (a power of two: commutes with the interpolation)
    if (a.normalize) r = (r - a.mean[c]) / a.std[c];
    v[e] = r;
  }
  float* dst = a.out + (((long)b * a.Cout + c) * a.Ho + y) * a.Wo + xb;
  if ((a.Wo & 3) == 0 && (reinterpret_cast<size_t>(a.out) & 15) == 0) {
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (xb + e < a.Wo) dst[e] = v[e];
  }
}

__global__ __launch_bounds__(64) void clf_decide_kernel(const float* __restrict__ pred, float threshold, int32_t* decision,
                                                        int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) decision[i] = pred[i] > threshold ? 1 : 0;
}
}  // namespace

extern "C" int ld_clf_max(const float* x, int groups, int64_t n, uint32_t* words, void* stream) {
  LD_REQUIRE(x && words, "ld_clf_max: null pointer");
  LD_REQUIRE(groups >= 1 && groups <= 65535 && n >= 1, "ld_clf_max: groups %d n %ld", groups, (long)n);
  const long per_wg = 256 * 4 * 8;                                // at least 8 float4 per thread before another workgroup
  const unsigned wgs = (unsigned)std::min<long>(CLF_MAX_WGS, (n + per_wg - 1) / per_wg);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(clf_max_kernel, dim3(wgs, (unsigned)groups), dim3(256), 0, st, x, (long)n, words);
  LD_LAUNCH_CHECK("clf_max");
  return LD_OK;
}

extern "C" int ld_clf_resize(const ld_clf_resize_args* p, void* stream) {
  LD_REQUIRE(p, "ld_clf_resize: null args");
  LD_REQUIRE(p->x && p->out, "ld_clf_resize: null pointer");
  LD_REQUIRE(p->B >= 1 && p->Hi >= 1 && p->Wi >= 1 && p->Ho >= 1 && p->Wo >= 1, "ld_clf_resize: sizes B=%d %dx%d -> %dx%d",
             p->B, p->Hi, p->Wi, p->Ho, p->Wo);
  LD_REQUIRE(p->Cout >= 1 && (p->Cin == p->Cout || p->Cin == 1), "ld_clf_resize: channels %d -> %d (equal, or 1 read "
             "for every output channel)", p->Cin, p->Cout);
  LD_REQUIRE(p->mode == LD_CLF_PLAIN || p->mode == LD_CLF_HALVE || p->mode == LD_CLF_AFFINE, "ld_clf_resize: mode %d", p->mode);
  LD_REQUIRE(p->mode != LD_CLF_HALVE || p->max_words, "ld_clf_resize: halving needs the max words");
  LD_REQUIRE(p->mode != LD_CLF_AFFINE || p->div != 0.0f, "ld_clf_resize: affine divisor 0");
  LD_REQUIRE(!p->normalize || p->Cout == 3, "ld_clf_resize: Normalize needs 3 output channels, not %d", p->Cout);
  LD_REQUIRE(p->n_zero >= 0 && (p->n_zero == 0 || p->zero_words), "ld_clf_resize: n_zero %d without words", p->n_zero);
  LD_REQUIRE(!p->pred || (p->decision && p->n_decision >= 1), "ld_clf_resize: decision output missing");
  if (p->normalize)
    for (int c = 0; c < 3; ++c) LD_REQUIRE(p->std[c] != 0.0f, "ld_clf_resize: std[%d] = 0", c);
  ClfResize a;
  a.x = p->x; a.out = p->out;
  a.B = p->B; a.Cin = p->Cin; a.Cout = p->Cout; a.Hi = p->Hi; a.Wi = p->Wi; a.Ho = p->Ho; a.Wo = p->Wo;
  a.mode = p->mode; a.max_words = p->max_words; a.per_sample = p->per_sample;
  a.zero_words = p->zero_words; a.n_zero = p->n_zero;
  a.sub = p->sub; a.mul = p->mul; a.add = p->add; a.div = p->div;
  a.normalize = p->normalize;
  for (int c = 0; c < 3; ++c) { a.mean[c] = p->mean[c]; a.std[c] = p->std[c]; }
  a.pred = p->pred; a.threshold = p->threshold; a.decision = p->decision; a.n_decision = p->n_decision;
  const long total = (long)p->B * p->Cout * p->Ho * ((p->Wo + 3) / 4);
  LD_REQUIRE((total + 255) / 256 < (1L << 31), "ld_clf_resize: %ld output groups", total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(clf_resize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
  LD_LAUNCH_CHECK("clf_resize");
  return LD_OK;
}

extern "C" int ld_clf_decide(const float* pred_score, float threshold, int32_t* decision, int n, void* stream) {
  LD_REQUIRE(pred_score && decision, "ld_clf_decide: null pointer");
  LD_REQUIRE(n >= 1, "ld_clf_decide: n %d", n);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(clf_decide_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, pred_score, threshold, decision, n);
  LD_LAUNCH_CHECK("clf_decide");
  return LD_OK;
}
