// The MNIST digit classifier (train_mnist_cls.py: SimpleCNN) and its training step, fp32, activations NHWC.
//
//   conv1 (1 -> 32, 3x3) + bias + ReLU + MaxPool2d(2)   mc_conv1_kernel, plain vector code (K = 9); the pooled map is
//                                                      written with a channel stride of 64 (the upper 32 stay zero) so
//                                                      that conv2 and its two gradients run through ld_pc_conv /
//                                                      ld_seg_wgrad (exact-f32 MFMA implicit GEMMs, 64-channel granule)
//   MaxPool2d(2) of conv2's output                      mc_pool_kernel
//   fc1 (3136 -> 128)                                   mc_gemm_kernel on v_mfma_f32_32x32x2_f32, K cut into slabs that
//                                                      mc_fc1_finish_kernel adds in order (+ bias, ReLU); the weight sits
//                                                      repacked to the NHWC feature order (y, x, c)
//   fc2 + softmax cross-entropy + its gradient          mc_head_kernel, one wave per sample: logits, lowest-index argmax,
//                                                      the sample's loss, d loss / d logits and the gradient of fc1's
//                                                      output behind its ReLU
//   fc2 / fc1-bias gradients and the mean loss          mc_small_grads_kernel (serial over the batch, in order)
//   fc1 weight / data gradient                          mc_gemm_kernel again (K = B and K = 128, no split)
//   pool backward                                       mc_pool_bwd_kernel: the 2-bit position stored by the forward pass
//                                                      (first maximum in row-major order, ATen's rule), ReLU'(0) = 0
//   conv1 weight / bias gradient                        mc_conv1_wgrad_kernel: the gradient is non-zero only at the pooled
//                                                      positions, so it is a gather over the pooled map; fixed slabs of
//                                                      pixels per workgroup, added in order by mc_conv1_wgrad_final_kernel
//   Adam                                                ld_seg_adam (segtrain.hip): all eight tensors in one launch,
//                                                      reading each gradient through its kernel layout's strides and
//                                                      writing the updated value into the kernel-layout copies as well
//
// No reduction uses floating-point atomics: two steps from the same state give the same bits.
#include "common.hip.h"

namespace {
typedef __attribute__((ext_vector_type(16))) float mc_f32x16;
constexpr int MC_T = 64;          // GEMM tile: 64 x 64 outputs per workgroup (four waves, one 32 x 32 block each)
constexpr int MC_KC = 32;         // K per chunk
constexpr int MC_HW = 28, MC_PW = 14, MC_C1 = 32, MC_CS = 64;   // image, pooled map, conv1 channels, their stride
constexpr int MC_HID = 128, MC_CLS = 10;
constexpr int MC_WG_PIX = 64;     // pooled pixels per workgroup of the conv1 weight gradient

inline unsigned mc_blocks(long n) { return (unsigned)((n + 255) / 256); }

// ------------------------------------------------------------------------------------------------ conv1 + ReLU + pool
// one thread per (pooled pixel, channel); the 32 channels of a pixel share the 4 x 4 input patch (broadcast loads)
__global__ __launch_bounds__(256) void mc_conv1_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* out, unsigned char* idx,
                                                       long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % MC_C1);
  const long p = i / MC_C1;                                   // (b * 14 + py) * 14 + px
  const int px = (int)(p % MC_PW), py = (int)((p / MC_PW) % MC_PW);
  const long b = p / (MC_PW * MC_PW);
  const float* img = x + b * (MC_HW * MC_HW);
  float patch[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int yy = 2 * py - 1 + r, xx = 2 * px - 1 + q;
      patch[r][q] = (yy >= 0 && yy < MC_HW && xx >= 0 && xx < MC_HW) ? img[yy * MC_HW + xx] : 0.0f;
    }
  float wk[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wk[t] = w[c * 9 + t];
  const float bc = bias[c];
  float best = 0.0f;
  int where = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {                               // window positions in row-major order
    const int dy = k >> 1, dx = k & 1;
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < 9; ++t) acc += patch[dy + t / 3][dx + t % 3] * wk[t];
    const float v = fmaxf(acc + bc, 0.0f);
    if (k == 0 || v > best) { best = v; where = k; }          // strict: the first maximum wins
  }
  out[p * MC_CS + c] = best;
  if (idx) idx[p * MC_C1 + c] = (unsigned char)where;
}

// MaxPool2d(2): x [B, 2H, 2W, C] -> out [B, H, W, C] and the window position of the first maximum
__global__ void mc_pool_kernel(const float* __restrict__ x, float* out, unsigned char* idx, long total, int H, int W, int C) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const long p = i / C;
  const int ox = (int)(p % W);
  const long r = p / W;                                       // b * H + oy
  const float* s = x + ((r * 2) * (2L * W) + 2 * ox) * C + c;
  const float v[4] = {s[0], s[C], s[2L * W * C], s[(2L * W + 1) * C]};
  float best = v[0];
  int where = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (v[k] > best) { best = v[k]; where = k; }
  out[i] = best;
  if (idx) idx[i] = (unsigned char)where;
}

// dx [B, 2H, 2W, C]: dpool at the stored position where the pooled activation (a ReLU output) is positive, else 0
__global__ void mc_pool_bwd_kernel(const float* __restrict__ dpool, const float* __restrict__ pooled,
                                   const unsigned char* __restrict__ idx, float* dx, long total, int H, int W, int C) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const long p = i / C;
  const int ox = (int)(p % W);
  const long r = p / W;
  float* d = dx + ((r * 2) * (2L * W) + 2 * ox) * C + c;
  const float g = pooled[i] > 0.0f ? dpool[i] : 0.0f;
  const int where = idx[i] & 3;
  d[0] = where == 0 ? g : 0.0f;
  d[C] = where == 1 ? g : 0.0f;
  d[2L * W * C] = where == 2 ? g : 0.0f;
  d[(2L * W + 1) * C] = where == 3 ? g : 0.0f;
}

// ------------------------------------------------------------------------------------------------ GEMM (fc1 and its gradients)
// out[z][m * cm + n] = sum over the K range of split z of A[m * am + k * ak] * Bm[n * bn + k * bk]
struct McGemmDev {
  const float* a; const float* b; float* out;
  long am, ak, bn, bk, cm, slab;
  int M, N, K, k_per_split;
};

__global__ __launch_bounds__(256) void mc_gemm_kernel(McGemmDev d) {
  __shared__ float sa[MC_KC][MC_T + 4];                       // [k][m]
  __shared__ float sb[MC_KC][MC_T + 4];                       // [k][n]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.y * MC_T, n0 = blockIdx.x * MC_T;
  const int k0 = blockIdx.z * d.k_per_split;
  const int k1 = k0 + d.k_per_split < d.K ? k0 + d.k_per_split : d.K;
  // loaders: along k where k is the contiguous axis of the operand, along the row otherwise (uniform per launch)
  const bool a_k = d.ak == 1, b_k = d.bk == 1;
  float ra[8], rb[8];
  auto fetch = [&](int kc) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int ka = a_k ? (tid & 31) : (tid >> 6) + 4 * u, ma = a_k ? (tid >> 5) + 8 * u : (tid & 63);
      const int kb = b_k ? (tid & 31) : (tid >> 6) + 4 * u, nb = b_k ? (tid >> 5) + 8 * u : (tid & 63);
      ra[u] = (kc + ka < k1 && m0 + ma < d.M) ? d.a[(long)(m0 + ma) * d.am + (long)(kc + ka) * d.ak] : 0.0f;
      rb[u] = (kc + kb < k1 && n0 + nb < d.N) ? d.b[(long)(n0 + nb) * d.bn + (long)(kc + kb) * d.bk] : 0.0f;
    }
  };
  mc_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  if (k0 < k1) fetch(k0);
  const int kh = lane >> 5, c = lane & 31;
  for (int kc = k0; kc < k1; kc += MC_KC) {
    __syncthreads();                                          // the previous chunk's reads of the tiles are done
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int ka = a_k ? (tid & 31) : (tid >> 6) + 4 * u, ma = a_k ? (tid >> 5) + 8 * u : (tid & 63);
      const int kb = b_k ? (tid & 31) : (tid >> 6) + 4 * u, nb = b_k ? (tid >> 5) + 8 * u : (tid & 63);
      sa[ka][ma] = ra[u];
      sb[kb][nb] = rb[u];
    }
    __syncthreads();
    if (kc + MC_KC < k1) fetch(kc + MC_KC);
#pragma unroll
    for (int kk = 0; kk < MC_KC; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[kk + kh][wm * 32 + c], sb[kk + kh][wn * 32 + c], acc, 0, 0, 0);
  }
  // C/D layout of 32x32x2f32: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* slab = d.out + (long)blockIdx.z * d.slab;
  const int n = n0 + wn * 32 + c;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
    if (m < d.M && n < d.N) slab[(long)m * d.cm + n] = acc[r];
  }
}

// h [B][N] = relu(sum over the slabs in order + bias)
__global__ void mc_fc1_finish_kernel(const float* __restrict__ work, const float* __restrict__ bias, float* h, long total, int N,
                                     int splits) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  float s = work[i];
  for (int k = 1; k < splits; ++k) s += work[(long)k * total + i];
  h[i] = fmaxf(s + bias[i % N], 0.0f);
}

// ------------------------------------------------------------------------------------------------ fc2 + loss
// one wave per sample.  label NULL: logits (and pred) only
__global__ __launch_bounds__(64) void mc_head_kernel(const float* __restrict__ h, const float* __restrict__ w2,
                                                     const float* __restrict__ b2, const long long* __restrict__ label,
                                                     float* logits, long long* pred, float* loss_b, float* dz, float* dh,
                                                     int* bad_label, int B) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float h0 = h[(long)b * MC_HID + lane], h1 = h[(long)b * MC_HID + 64 + lane];
  float z[MC_CLS];
#pragma unroll
  for (int j = 0; j < MC_CLS; ++j) {
    float s = h0 * w2[j * MC_HID + lane] + h1 * w2[j * MC_HID + 64 + lane];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);          // the same tree in every lane and every run
    z[j] = s + b2[j];
  }
  float zmax = z[0];
  int arg = 0;
#pragma unroll
  for (int j = 1; j < MC_CLS; ++j)
    if (z[j] > zmax) { zmax = z[j]; arg = j; }               // strict: the lowest index on equal logits (torch.max)
  if (lane < MC_CLS) {
    float mine = z[0];
#pragma unroll
    for (int j = 1; j < MC_CLS; ++j) mine = lane == j ? z[j] : mine;
    logits[(long)b * MC_CLS + lane] = mine;
  }
  if (pred && lane == 0) pred[b] = arg;
  if (!label) return;
  const long long lab = label[b];
  const bool ok = lab >= 0 && lab < MC_CLS;
  float e[MC_CLS], sum = 0.0f, zl = 0.0f;
#pragma unroll
  for (int j = 0; j < MC_CLS; ++j) {
    e[j] = expf(z[j] - zmax);
    sum += e[j];
    zl = (ok && lab == j) ? z[j] : zl;
  }
  const float inv_b = 1.0f / (float)B;
  float g[MC_CLS];
#pragma unroll
  for (int j = 0; j < MC_CLS; ++j) g[j] = ok ? (e[j] / sum - (lab == j ? 1.0f : 0.0f)) * inv_b : 0.0f;
  if (lane == 0) {
    // a label outside 0..9 indexes nothing: its sample gets a NaN loss, no gradient, and the sticky flag is raised
    loss_b[b] = ok ? (zmax - zl) + logf(sum) : __int_as_float(0x7fc00000);
    if (!ok) *bad_label = 1;
  }
  if (lane < MC_CLS) {
    float mine = g[0];
#pragma unroll
    for (int j = 1; j < MC_CLS; ++j) mine = lane == j ? g[j] : mine;
    dz[(long)b * MC_CLS + lane] = mine;
  }
  float d0 = 0.0f, d1 = 0.0f;
#pragma unroll
  for (int j = 0; j < MC_CLS; ++j) {
    d0 += g[j] * w2[j * MC_HID + lane];
    d1 += g[j] * w2[j * MC_HID + 64 + lane];
  }
  dh[(long)b * MC_HID + lane] = h0 > 0.0f ? d0 : 0.0f;       // ReLU'(0) = 0
  dh[(long)b * MC_HID + 64 + lane] = h1 > 0.0f ? d1 : 0.0f;
}

// gw2 [10][128], gb2 [10], gb1 [128] (fc1's bias) and the mean loss: each output adds over the batch in index order
__global__ void mc_small_grads_kernel(const float* __restrict__ dz, const float* __restrict__ h, const float* __restrict__ dh,
                                      const float* __restrict__ loss_b, float* gw2, float* gb2, float* gb1, float* loss, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int NW = MC_CLS * MC_HID;
  float s = 0.0f;
  if (i < NW) {
    const int j = i / MC_HID, k = i % MC_HID;
    for (int b = 0; b < B; ++b) s += dz[(long)b * MC_CLS + j] * h[(long)b * MC_HID + k];
    gw2[i] = s;
  } else if (i < NW + MC_CLS) {
    const int j = i - NW;
    for (int b = 0; b < B; ++b) s += dz[(long)b * MC_CLS + j];
    gb2[j] = s;
  } else if (i < NW + MC_CLS + MC_HID) {
    const int k = i - NW - MC_CLS;
    for (int b = 0; b < B; ++b) s += dh[(long)b * MC_HID + k];
    gb1[k] = s;
  } else if (i == NW + MC_CLS + MC_HID) {
    for (int b = 0; b < B; ++b) s += loss_b[b];
    loss[0] = s / (float)B;
  }
}

// ------------------------------------------------------------------------------------------------ conv1 weight gradient
// part [slab][32][10]: 9 taps + the bias, over MC_WG_PIX pooled pixels; thread = (channel, pixel lane of 8)
__global__ __launch_bounds__(256) void mc_conv1_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ p1,
                                                             const float* __restrict__ dp1, const unsigned char* __restrict__ idx,
                                                             float* part, long npix) {
  __shared__ float red[8][MC_C1 * 10];
  const int c = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const long q0 = (long)blockIdx.x * MC_WG_PIX;
  const long q1 = q0 + MC_WG_PIX < npix ? q0 + MC_WG_PIX : npix;
  float acc[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) acc[t] = 0.0f;
  for (long q = q0 + pl; q < q1; q += 8) {
    const float g = p1[q * MC_CS + c] > 0.0f ? dp1[q * MC_CS + c] : 0.0f;
    const int where = idx[q * MC_C1 + c] & 3;
    const int px = (int)(q % MC_PW), py = (int)((q / MC_PW) % MC_PW);
    const float* img = x + (q / (MC_PW * MC_PW)) * (MC_HW * MC_HW);
    const int y = 2 * py + (where >> 1), xx0 = 2 * px + (where & 1);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int yy = y + t / 3 - 1, xx = xx0 + t % 3 - 1;
      const float v = (yy >= 0 && yy < MC_HW && xx >= 0 && xx < MC_HW) ? img[yy * MC_HW + xx] : 0.0f;
      acc[t] += g * v;
    }
    acc[9] += g;
  }
#pragma unroll
  for (int t = 0; t < 10; ++t) red[pl][c * 10 + t] = acc[t];
  __syncthreads();
  for (int o = threadIdx.x; o < MC_C1 * 10; o += 256) {
    float s = red[0][o];
#pragma unroll
    for (int k = 1; k < 8; ++k) s += red[k][o];
    part[(long)blockIdx.x * (MC_C1 * 10) + o] = s;
  }
}

__global__ void mc_conv1_wgrad_final_kernel(const float* __restrict__ part, int slabs, float* gw, float* gb) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= MC_C1 * 10) return;
  float s = 0.0f;
  for (int k = 0; k < slabs; ++k) s += part[(long)k * (MC_C1 * 10) + o];
  const int c = o / 10, t = o % 10;
  if (t < 9) gw[c * 9 + t] = s;
  else gb[c] = s;
}
}  // namespace

extern "C" int ld_mc_conv1(const float* x, const float* w, const float* bias, float* out, unsigned char* idx, int B,
                           void* stream) {
  LD_REQUIRE(B > 0 && B <= (1 << 20), "ld_mc_conv1: batch %d", B);
  LD_REQUIRE(x && w && bias && out, "ld_mc_conv1: null pointer");
  const long total = (long)B * MC_PW * MC_PW * MC_C1;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(mc_conv1_kernel, dim3(mc_blocks(total)), dim3(256), 0, st, x, w, bias, out, idx, total);
  LD_LAUNCH_CHECK("mc_conv1");
  return LD_OK;
}

static int mc_pool_shape(const char* name, int B, int H, int W, int C, long* total) {
  LD_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "%s: shape B=%d H=%d W=%d C=%d", name, B, H, W, C);
  *total = (long)B * H * W * C;
  LD_REQUIRE((*total + 255) / 256 < (1L << 31), "%s: %ld elements", name, *total);
  return LD_OK;
}

extern "C" int ld_mc_pool(const float* x, float* out, unsigned char* idx, int B, int H, int W, int C, void* stream) {
  long total = 0;
  if (int rc = mc_pool_shape("ld_mc_pool", B, H, W, C, &total)) return rc;
  LD_REQUIRE(x && out, "ld_mc_pool: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(mc_pool_kernel, dim3(mc_blocks(total)), dim3(256), 0, st, x, out, idx, total, H, W, C);
  LD_LAUNCH_CHECK("mc_pool");
  return LD_OK;
}

extern "C" int ld_mc_pool_backward(const float* dpool, const float* pooled, const unsigned char* idx, float* dx, int B, int H,
                                   int W, int C, void* stream) {
  long total = 0;
  if (int rc = mc_pool_shape("ld_mc_pool_backward", B, H, W, C, &total)) return rc;
  LD_REQUIRE(dpool && pooled && idx && dx, "ld_mc_pool_backward: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(mc_pool_bwd_kernel, dim3(mc_blocks(total)), dim3(256), 0, st, dpool, pooled, idx, dx, total, H, W, C);
  LD_LAUNCH_CHECK("mc_pool_backward");
  return LD_OK;
}

extern "C" int ld_mc_gemm(const float* a, const float* b, float* out, int M, int N, int K, int64_t am, int64_t ak, int64_t bn,
                          int64_t bk, int64_t cm, int splits, void* stream) {
  LD_REQUIRE(M > 0 && N > 0 && K > 0, "ld_mc_gemm: shape M=%d N=%d K=%d", M, N, K);
  LD_REQUIRE(am > 0 && ak > 0 && bn > 0 && bk > 0 && cm >= N, "ld_mc_gemm: strides (positive, cm >= N)");
  LD_REQUIRE(splits >= 1 && splits <= (K + MC_KC - 1) / MC_KC && splits <= 65535, "ld_mc_gemm: splits %d (1..ceil(K / 32))", splits);
  LD_REQUIRE((M + MC_T - 1) / MC_T <= 65535, "ld_mc_gemm: M %d", M);
  LD_REQUIRE(a && b && out, "ld_mc_gemm: null pointer");
  int per = (K + splits - 1) / splits;
  per = (per + MC_KC - 1) / MC_KC * MC_KC;                    // whole chunks per split
  LD_REQUIRE((long)(splits - 1) * per < K, "ld_mc_gemm: splits %d leave an empty slab for K %d", splits, K);
  McGemmDev d{a, b, out, (long)am, (long)ak, (long)bn, (long)bk, (long)cm, (long)M * cm, M, N, K, per};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(mc_gemm_kernel, dim3((unsigned)((N + MC_T - 1) / MC_T), (unsigned)((M + MC_T - 1) / MC_T), (unsigned)splits),
            dim3(256), 0, st, d);
  LD_LAUNCH_CHECK("mc_gemm");
  return LD_OK;
}

extern "C" int ld_mc_fc1_finish(const float* work, const float* bias, float* h, int B, int N, int splits, void* stream) {
  LD_REQUIRE(B > 0 && N > 0 && splits >= 1, "ld_mc_fc1_finish: B=%d N=%d splits=%d", B, N, splits);
  LD_REQUIRE(work && bias && h, "ld_mc_fc1_finish: null pointer");
  const long total = (long)B * N;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(mc_fc1_finish_kernel, dim3(mc_blocks(total)), dim3(256), 0, st, work, bias, h, total, N, splits);
  LD_LAUNCH_CHECK("mc_fc1_finish");
  return LD_OK;
}

extern "C" int ld_mc_head(const float* h, const float* w2, const float* b2, const int64_t* label, float* logits, int64_t* pred,
                          float* loss_b, float* dz, float* dh, int32_t* bad_label, int B, void* stream) {
  LD_REQUIRE(B > 0 && B <= (1 << 20), "ld_mc_head: batch %d", B);
  LD_REQUIRE(h && w2 && b2 && logits, "ld_mc_head: null pointer");
  LD_REQUIRE(!label || (loss_b && dz && dh && bad_label), "ld_mc_head: labels without loss_b / dz / dh / bad_label");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(mc_head_kernel, dim3((unsigned)B), dim3(64), 0, st, h, w2, b2, (const long long*)label, logits, (long long*)pred,
            loss_b, dz, dh, (int*)bad_label, B);
  LD_LAUNCH_CHECK("mc_head");
  return LD_OK;
}

extern "C" int ld_mc_small_grads(const float* dz, const float* h, const float* dh, const float* loss_b, float* gw2, float* gb2,
                                 float* gb1, float* loss, int B, void* stream) {
  LD_REQUIRE(B > 0 && B <= (1 << 20), "ld_mc_small_grads: batch %d", B);
  LD_REQUIRE(dz && h && dh && loss_b && gw2 && gb2 && gb1 && loss, "ld_mc_small_grads: null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long n = MC_CLS * MC_HID + MC_CLS + MC_HID + 1;
  LD_LAUNCH(mc_small_grads_kernel, dim3(mc_blocks(n)), dim3(256), 0, st, dz, h, dh, loss_b, gw2, gb2, gb1, loss, B);
  LD_LAUNCH_CHECK("mc_small_grads");
  return LD_OK;
}

extern "C" int64_t ld_mc_conv1_wgrad_work_floats(int B) {
  if (B <= 0) return 0;
  const long npix = (long)B * MC_PW * MC_PW;
  return (npix + MC_WG_PIX - 1) / MC_WG_PIX * (MC_C1 * 10);
}

extern "C" int ld_mc_conv1_wgrad(const float* x, const float* p1, const float* dp1, const unsigned char* idx, float* work,
                                 float* gw, float* gb, int B, void* stream) {
  LD_REQUIRE(B > 0 && B <= (1 << 20), "ld_mc_conv1_wgrad: batch %d", B);
  LD_REQUIRE(x && p1 && dp1 && idx && work && gw && gb, "ld_mc_conv1_wgrad: null pointer");
  const long npix = (long)B * MC_PW * MC_PW;
  const int slabs = (int)((npix + MC_WG_PIX - 1) / MC_WG_PIX);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(mc_conv1_wgrad_kernel, dim3((unsigned)slabs), dim3(256), 0, st, x, p1, dp1, idx, work, npix);
  LD_LAUNCH(mc_conv1_wgrad_final_kernel, dim3(mc_blocks(MC_C1 * 10)), dim3(256), 0, st, (const float*)work, slabs, gw, gb);
  LD_LAUNCH_CHECK("mc_conv1_wgrad");
  return LD_OK;
}
