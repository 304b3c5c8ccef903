// PatchCore (models.py:42-254, eval mode): the default OOD anomaly-map producer that test.py:150-178, 240-247 runs on
// the conditioning image before sample(..., mask=...).  Everything here is fp32 in storage and arithmetic: the mask
// thresholds of test.py:251-375 are absolute distances.
//
//   * pc_conv_kernel: the wide_resnet50_2 trunk's 1x1 / 3x3 convolutions (stride 1 or 2) as an NHWC implicit GEMM,
//     M = output pixels, N = output channels, K = taps x input channels, with BatchNorm (eval) + optional residual +
//     optional ReLU as the epilogue;
//   * pc_knn_kernel: the nearest-neighbour search, a GEMM of query rows against the memory bank whose epilogue keeps a
//     running (d2, index) minimum per query instead of writing the N x M matrix; bank splits are merged with a 64-bit
//     atomicMin on (d2 bits << 32 | index), monotone for d2 >= 0 and lowest-index on ties as torch's min(1) is;
//   * the stem (7x7 s2 from the NCHW image), the max-pool, the embedding (pool / resample / concat / |x|^2), the image
//     score and the anomaly map (nearest upsample + separable Gaussian, reflect padding) as small direct kernels.
//
// Both GEMMs share pc_gemm: a workgroup of 4 waves owns a TM x 64 output tile (2 x 2 waves, each TM/2 x 32 as TM/64
// blocks of v_mfma_f32_32x32x2_f32, exact f32), K in chunks of 32 staged through LDS with the next chunk's global loads
// in registers while the current one is multiplied.  Both operands are K-contiguous rows (activations / query rows and
// OHWI weights / bank rows), so one loader shape serves both.
#include "common.hip.h"
#include "pc_knn.hip.h"

namespace {
constexpr int PC_TN = 64;   // output columns per workgroup (output channels / bank rows)
constexpr int PC_KC = 32;   // K per chunk
typedef __attribute__((ext_vector_type(16))) float pc_f32x16;

template <int TM>
struct PcSmem {
  float a[PC_KC][TM + 4];      // [k][row]
  float b[PC_KC][PC_TN + 4];   // [k][column]
};

// Main loop.  fa(q, u) / fb(q, u): the float4 that thread slot u loads for chunk q (row (tid >> 3) + 32 u, k offset
// (tid & 7) * 4 of the chunk); they return zeros where the operand is padding.
template <int TM, typename FA, typename FB>
__device__ __forceinline__ void pc_gemm(PcSmem<TM>& sm, int nq, FA fa, FB fb, pc_f32x16 (&acc)[TM / 64]) {
  constexpr int UA = TM / 32, UB = PC_TN / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int lr = tid >> 3, lk = (tid & 7) * 4;
#pragma unroll
  for (int m = 0; m < TM / 64; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.0f;
  float4 ra[UA], rb[UB];
#pragma unroll
  for (int u = 0; u < UA; ++u) ra[u] = fa(0, u);
#pragma unroll
  for (int u = 0; u < UB; ++u) rb[u] = fb(0, u);
  for (int q = 0; q < nq; ++q) {
    __syncthreads();                                  // the previous chunk's reads of the tile are done
#pragma unroll
    for (int u = 0; u < UA; ++u) {
      const int r = lr + 32 * u;
      sm.a[lk][r] = ra[u].x; sm.a[lk + 1][r] = ra[u].y; sm.a[lk + 2][r] = ra[u].z; sm.a[lk + 3][r] = ra[u].w;
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int r = lr + 32 * u;
      sm.b[lk][r] = rb[u].x; sm.b[lk + 1][r] = rb[u].y; sm.b[lk + 2][r] = rb[u].z; sm.b[lk + 3][r] = rb[u].w;
    }
    __syncthreads();
    if (q + 1 < nq) {
#pragma unroll
      for (int u = 0; u < UA; ++u) ra[u] = fa(q + 1, u);
#pragma unroll
      for (int u = 0; u < UB; ++u) rb[u] = fb(q + 1, u);
    }
    const int kh = lane >> 5, c = lane & 31;
#pragma unroll
    for (int kk = 0; kk < PC_KC; kk += 2) {
      const float bv = sm.b[kk + kh][wn * 32 + c];
#pragma unroll
      for (int m = 0; m < TM / 64; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(sm.a[kk + kh][wm * (TM / 2) + m * 32 + c], bv, acc[m], 0, 0, 0);
    }
  }
}

// Row of the output tile that accumulator register r of block m holds in this lane (C/D layout of 32x32x2f32: column
// lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5))
template <int TM>
__device__ __forceinline__ int pc_acc_row(int m, int r) {
  const int lane = threadIdx.x & 63, wm = (threadIdx.x >> 6) & 1;
  return wm * (TM / 2) + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}
__device__ __forceinline__ int pc_acc_col() { return ((threadIdx.x >> 6) >> 1) * 32 + (threadIdx.x & 31); }

// ------------------------------------------------------------------------------------------------ convolution
constexpr int PC_CONV_TM = 64;

__global__ __launch_bounds__(256) void pc_conv_kernel(ld_pc_conv_args a) {
  __shared__ __attribute__((aligned(16))) PcSmem<PC_CONV_TM> sm;
  constexpr int UA = PC_CONV_TM / 32;
  const int tid = threadIdx.x;
  const long M = (long)a.B * a.Ho * a.Wo;
  const long p0 = (long)blockIdx.x * PC_CONV_TM;
  const int n0 = blockIdx.y * PC_TN;
  const int ks = a.ksize, pad = ks == 3 ? 1 : 0, nch = a.Cin / PC_KC, K = ks * ks * a.Cin;
  const int lr = tid >> 3, lk = (tid & 7) * 4;
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
    const int tap = q / nch, c0 = (q - tap * nch) * PC_KC;
    const int iy = py[u] * a.stride - pad + tap / ks, ix = px[u] * a.stride - pad + tap % ks;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (pv[u] && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi)
      v = *reinterpret_cast<const float4*>(a.src + (((long)pb[u] * a.Hi + iy) * a.Wi + ix) * a.Cin + c0 + lk);
    return v;
  };
  auto fb = [&](int q, int u) {
    return *reinterpret_cast<const float4*>(a.weight + (long)(n0 + lr + 32 * u) * K + q * PC_KC + lk);
  };
  pc_f32x16 acc[PC_CONV_TM / 64];
  pc_gemm<PC_CONV_TM>(sm, ks * ks * nch, fa, fb, acc);
  const int co = n0 + pc_acc_col();
  const float s = a.scale[co], t = a.shift[co];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long p = p0 + pc_acc_row<PC_CONV_TM>(0, r);
    if (p >= M) continue;
    float v = acc[0][r] * s + t;
    if (a.residual) v += a.residual[p * a.Cout + co];
    if (a.relu) v = fmaxf(v, 0.0f);
    a.out[p * a.Cout + co] = v;
  }
}

// ------------------------------------------------------------------------------------------------ nearest neighbours
constexpr int PC_KNN_TM = 128;

struct PcKnnDev {
  const float* q; const float* qn; const float* bank; const float* bn;
  unsigned long long* keys;   // MODE 0: [N] running minimum
  float* d2;                  // MODE 1: [N, M] all distances
  long M; int N, D, tiles_per_split;
  const int32_t* list; const int32_t* count;   // MODE 2 only
};

// MODE 0: min / argmin per query over this workgroup's bank tiles, merged by atomicMin.  MODE 1: d2 matrix (top-k).
// MODE 2: MODE 0 for the *a.count queries whose row numbers are in a.list (the exact search of the queries that the
// fp16 screen of knn16.hip could not certify); the grid is sized for N, surplus workgroups leave on the count.
template <int MODE>
__global__ __launch_bounds__(256) void pc_knn_kernel(PcKnnDev a) {
  __shared__ __attribute__((aligned(16))) PcSmem<PC_KNN_TM> sm;
  constexpr int NB = PC_KNN_TM / 64;
  const int tid = threadIdx.x, lr = tid >> 3, lk = (tid & 7) * 4;
  const int row0 = blockIdx.x * PC_KNN_TM;
  int nrows = a.N;
  if constexpr (MODE == 2) {
    nrows = *a.count;
    if (row0 >= nrows) return;
  }
  auto src = [&](int i) { if constexpr (MODE == 2) return (int)a.list[i]; else return i; };   // row i of the tile space
  const long ntiles = (a.M + PC_TN - 1) / PC_TN;
  const long t0 = (long)blockIdx.y * a.tiles_per_split;
  const long t1 = t0 + a.tiles_per_split < ntiles ? t0 + a.tiles_per_split : ntiles;
  const float* qrow[PC_KNN_TM / 32];
#pragma unroll
  for (int u = 0; u < PC_KNN_TM / 32; ++u) {
    const int r = row0 + lr + 32 * u;
    qrow[u] = a.q + (long)src(r < nrows ? r : nrows - 1) * a.D + lk;   // padding rows read a real row, never stored
  }
  float qn[NB][16];
#pragma unroll
  for (int m = 0; m < NB; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = row0 + pc_acc_row<PC_KNN_TM>(m, r);
      qn[m][r] = a.qn[src(i < nrows ? i : nrows - 1)];
    }
  float best[NB][16];
  unsigned bidx[NB][16];
#pragma unroll
  for (int m = 0; m < NB; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) { best[m][r] = __builtin_inff(); bidx[m][r] = 0xffffffffu; }
  const int nq = a.D / PC_KC;
  for (long tile = t0; tile < t1; ++tile) {
    const long m0 = tile * PC_TN;
    const float* brow[PC_TN / 32];
#pragma unroll
    for (int u = 0; u < PC_TN / 32; ++u) {
      const long j = m0 + lr + 32 * u;
      brow[u] = a.bank + (j < a.M ? j : a.M - 1) * a.D + lk;
    }
    auto fa = [&](int q, int u) { return *reinterpret_cast<const float4*>(qrow[u] + q * PC_KC); };
    auto fb = [&](int q, int u) { return *reinterpret_cast<const float4*>(brow[u] + q * PC_KC); };
    pc_f32x16 acc[NB];
    pc_gemm<PC_KNN_TM>(sm, nq, fa, fb, acc);
    const long j = m0 + pc_acc_col();
    if (j >= a.M) continue;
    const float bnj = a.bn[j];
#pragma unroll
    for (int m = 0; m < NB; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float d2 = fmaxf((qn[m][r] - 2.0f * acc[m][r]) + bnj, 0.0f);     // euclidean_dist's order (models.py:194)
        if constexpr (MODE != 1) {
          if (d2 < best[m][r]) { best[m][r] = d2; bidx[m][r] = (unsigned)j; }   // columns rise: the first index stays
        } else {
          const int i = row0 + pc_acc_row<PC_KNN_TM>(m, r);
          if (i < a.N) a.d2[(long)i * a.M + j] = d2;
        }
      }
  }
  if constexpr (MODE != 1) {
#pragma unroll
    for (int m = 0; m < NB; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        unsigned long long k = bidx[m][r] == 0xffffffffu ? ~0ull : pc_key(best[m][r], bidx[m][r]);
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {                // the 32 lanes of a half-wave hold the same row
          const unsigned long long k2 = pc_shfl_xor64(k, o);
          k = k2 < k ? k2 : k;
        }
        const int i = row0 + pc_acc_row<PC_KNN_TM>(m, r);
        if ((threadIdx.x & 31) == 0 && i < nrows && k != ~0ull) atomicMin(a.keys + src(i), k);
      }
  }
}

__global__ void pc_knn_init_kernel(unsigned long long* keys, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) keys[i] = ~0ull;
}

__global__ void pc_knn_finish_kernel(const unsigned long long* keys, float* dist, int32_t* idx, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const unsigned long long k = keys[i];
  if (k == ~0ull) {                                   // no finite distance at all (NaN input): index 0, distance NaN
    dist[i] = __builtin_nanf("");
    idx[i] = 0;
    return;
  }
  dist[i] = sqrtf(__uint_as_float((unsigned)(k >> 32)));
  idx[i] = (int32_t)(unsigned)(k & 0xffffffffu);
}

// top-k of one row of d2 [N, M] per workgroup: each thread keeps a sorted list of its k best (d2, index) keys, then k
// rounds of a workgroup minimum over the list heads.  Keys are unique (the index is in them), so ties go to the lower
// index.
constexpr int PC_TOPK_MAX = 16;
__global__ __launch_bounds__(256) void pc_topk_kernel(const float* d2, long M, int k, float* dist, int32_t* idx) {
  __shared__ unsigned long long wmin[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  unsigned long long lst[PC_TOPK_MAX];
#pragma unroll
  for (int t = 0; t < PC_TOPK_MAX; ++t) lst[t] = ~0ull;
  const float* p = d2 + (long)row * M;
  for (long j = tid; j < M; j += 256) {
    unsigned long long key = pc_key(p[j], (unsigned)j);
#pragma unroll
    for (int t = 0; t < PC_TOPK_MAX; ++t) {
      const unsigned long long lo = key < lst[t] ? key : lst[t], hi = key < lst[t] ? lst[t] : key;
      lst[t] = lo;
      key = hi;
    }
  }
  for (int r = 0; r < k; ++r) {
    unsigned long long m = lst[0];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long m2 = pc_shfl_xor64(m, o);
      m = m2 < m ? m2 : m;
    }
    if ((tid & 63) == 0) wmin[tid >> 6] = m;
    __syncthreads();
    unsigned long long g = wmin[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) g = wmin[w] < g ? wmin[w] : g;
    __syncthreads();
    if (lst[0] == g) {                                    // the one thread whose head won pops it
#pragma unroll
      for (int t = 0; t < PC_TOPK_MAX - 1; ++t) lst[t] = lst[t + 1];
      lst[PC_TOPK_MAX - 1] = ~0ull;
    }
    if (tid == 0) {
      dist[(long)row * k + r] = sqrtf(__uint_as_float((unsigned)(g >> 32)));
      idx[(long)row * k + r] = (int32_t)(unsigned)(g & 0xffffffffu);
    }
  }
}

// ------------------------------------------------------------------------------------------------ small kernels
// conv1 7x7 s2 p3 (3 -> 64) + bn1 + ReLU, one thread per output pixel, the weights in LDS as [ci*49 + tap][64]
__global__ __launch_bounds__(256) void pc_stem_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      float* out, int B, int H, int W, int Ho, int Wo) {
  __shared__ __attribute__((aligned(16))) float ws[3 * 49][64];
  for (int i = threadIdx.x; i < 64 * 3 * 49; i += blockDim.x) {
    const int co = i / (3 * 49), k = i - co * 3 * 49;     // OIHW: [co][ci][ky][kx] = [co][k]
    ws[k][co] = w[i];
  }
  __syncthreads();
  const long M = (long)B * Ho * Wo;
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= M) return;
  const int ox = (int)(p % Wo);
  const long r = p / Wo;
  const int oy = (int)(r % Ho), b = (int)(r / Ho);
  float acc[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) acc[c] = 0.0f;
  for (int ci = 0; ci < 3; ++ci) {
    const float* xp = x + ((long)b * 3 + ci) * H * W;
    for (int ky = 0; ky < 7; ++ky) {
      const int sy = oy * 2 - 3 + ky;
      if (sy < 0 || sy >= H) continue;
      for (int kx = 0; kx < 7; ++kx) {
        const int sx = ox * 2 - 3 + kx;
        if (sx < 0 || sx >= W) continue;
        const float v = xp[(long)sy * W + sx];
        const float* wr = ws[ci * 49 + ky * 7 + kx];
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
  }
  float* op = out + p * 64;
#pragma unroll
  for (int c = 0; c < 64; c += 4) {
    float4 v;
    v.x = fmaxf(acc[c] * scale[c] + shift[c], 0.0f);
    v.y = fmaxf(acc[c + 1] * scale[c + 1] + shift[c + 1], 0.0f);
    v.z = fmaxf(acc[c + 2] * scale[c + 2] + shift[c + 2], 0.0f);
    v.w = fmaxf(acc[c + 3] * scale[c + 3] + shift[c + 3], 0.0f);
    *reinterpret_cast<float4*>(op + c) = v;
  }
}

// MaxPool2d(3, 2, 1), one thread per (output pixel, 4 channels); padding never wins (it is -inf in torch)
__global__ void pc_maxpool_kernel(const float* __restrict__ x, float* out, int B, int H, int W, int C, int Ho, int Wo) {
  const int C4 = C / 4;
  const long total = (long)B * Ho * Wo * C4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4) * 4;
  const long p = i / C4;
  const int ox = (int)(p % Wo);
  const long r = p / Wo;
  const int oy = (int)(r % Ho), b = (int)(r / Ho);
  float4 m = make_float4(-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff());
  for (int dy = 0; dy < 3; ++dy) {
    const int sy = oy * 2 - 1 + dy;
    if (sy < 0 || sy >= H) continue;
    for (int dx = 0; dx < 3; ++dx) {
      const int sx = ox * 2 - 1 + dx;
      if (sx < 0 || sx >= W) continue;
      const float4 v = *reinterpret_cast<const float4*>(x + (((long)b * H + sy) * W + sx) * C + c);
      m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
  }
  *reinterpret_cast<float4*>(out + p * C + c) = m;
}

// AvgPool2d(3, 1, 1) at (y, x) of channel c of an NHWC map: the in-range taps summed in (dy, dx) order, / 9
__device__ __forceinline__ float pc_avg3(const float* m, int H, int W, int C, int b, int y, int x, int c) {
  float s = 0.0f;
  for (int dy = -1; dy <= 1; ++dy) {
    const int sy = y + dy;
    if (sy < 0 || sy >= H) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int sx = x + dx;
      if (sx < 0 || sx >= W) continue;
      s += m[(((long)b * H + sy) * W + sx) * C + c];
    }
  }
  return s / 9.0f;
}

// torch's bilinear source index (align_corners=False): i0, i1 and the weights l0, l1 of output index o
__device__ __forceinline__ void pc_lin(int o, int in, int out, int& i0, int& i1, float& l0, float& l1) {
  const float scale = (float)in / (float)out;
  float real = scale * ((float)o + 0.5f) - 0.5f;
  if (real < 0.0f) real = 0.0f;
  i0 = (int)real;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(real - (float)i0, 0.0f), 1.0f);
  l0 = 1.0f - l1;
}

// one workgroup per embedding row (b, y, x) of the layer2 grid
__global__ __launch_bounds__(256) void pc_embed_kernel(const float* __restrict__ l2, const float* __restrict__ l3,
                                                       float* rows, float* norms, int h2, int w2, int C2, int h3, int w3,
                                                       int C3) {
  __shared__ float part[4];
  const long n = blockIdx.x;
  const int x = (int)(n % w2);
  const int y = (int)((n / w2) % h2), b = (int)(n / ((long)w2 * h2));
  int y0, y1, x0, x1;
  float hy0, hy1, wx0, wx1;
  pc_lin(y, h3, h2, y0, y1, hy0, hy1);
  pc_lin(x, w3, w2, x0, x1, wx0, wx1);
  const int D = C2 + C3;
  float* out = rows + n * D;
  float ss = 0.0f;
  for (int c = threadIdx.x; c < D; c += blockDim.x) {
    float v;
    if (c < C2) {
      v = pc_avg3(l2, h2, w2, C2, b, y, x, c);
    } else {
      const int cc = c - C2;
      const float v00 = pc_avg3(l3, h3, w3, C3, b, y0, x0, cc), v01 = pc_avg3(l3, h3, w3, C3, b, y0, x1, cc);
      const float v10 = pc_avg3(l3, h3, w3, C3, b, y1, x0, cc), v11 = pc_avg3(l3, h3, w3, C3, b, y1, x1, cc);
      v = hy0 * (wx0 * v00 + wx1 * v01) + hy1 * (wx0 * v10 + wx1 * v11);
    }
    out[c] = v;
    ss = fmaf(v, v, ss);
  }
  for (int o = 1; o < 64; o <<= 1) ss += __shfl_xor(ss, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0) norms[n] = (part[0] + part[1]) + (part[2] + part[3]);
}

// |x|^2 per row, one wave per row
__global__ __launch_bounds__(256) void pc_row_norms_kernel(const float* __restrict__ x, float* norms, long n, int d) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* p = x + row * d;
  float s = 0.0f;
  for (int c = threadIdx.x & 63; c < d; c += 64) s = fmaf(p[c], p[c], s);
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) norms[row] = s;
}

// image score, part 1: one workgroup per image
__global__ __launch_bounds__(256) void pc_score_prepare_kernel(const float* __restrict__ ps, const int32_t* __restrict__ loc,
                                                               const float* __restrict__ bank, const float* __restrict__ bn,
                                                               int P, int D, float* q, float* qn, int32_t* amax) {
  __shared__ float wv[4];
  __shared__ int wi[4];
  __shared__ int best;
  const int b = blockIdx.x, tid = threadIdx.x;
  float v = -__builtin_inff();
  int vi = 0x7fffffff;
  for (int p = tid; p < P; p += 256) {
    const float s = ps[(long)b * P + p];
    if (s > v) { v = s; vi = p; }                       // p rises: the first maximum stays
  }
  for (int o = 1; o < 64; o <<= 1) {
    const float v2 = __shfl_xor(v, o);
    const int i2 = __shfl_xor(vi, o);
    if (v2 > v || (v2 == v && i2 < vi)) { v = v2; vi = i2; }
  }
  if ((tid & 63) == 0) { wv[tid >> 6] = v; wi[tid >> 6] = vi; }
  __syncthreads();
  if (tid == 0) {
    float bv = wv[0];
    int bi = wi[0];
    for (int w = 1; w < 4; ++w)
      if (wv[w] > bv || (wv[w] == bv && wi[w] < bi)) { bv = wv[w]; bi = wi[w]; }
    if (bi >= P) bi = 0;                                // all NaN: patch 0, as an index that is in range
    best = bi;
    amax[b] = bi;
    qn[b] = bn[loc[(long)b * P + bi]];
  }
  __syncthreads();
  const float* src = bank + (long)loc[(long)b * P + best] * D;
  for (int c = tid; c < D; c += 256) q[(long)b * D + c] = src[c];
}

// image score, part 2: one workgroup per image
__global__ __launch_bounds__(256) void pc_score_kernel(const float* __restrict__ rows, const float* __restrict__ rn,
                                                       const float* __restrict__ ps, const int32_t* __restrict__ amax,
                                                       const float* __restrict__ bank, const float* __restrict__ bn,
                                                       const int32_t* __restrict__ sup, int P, int D, int k, float* score) {
  __shared__ float part[4];
  __shared__ float dist[PC_TOPK_MAX];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long pr = (long)b * P + amax[b];
  const float s_star = ps[pr];
  if (k == 0) {
    if (tid == 0) score[b] = s_star;
    return;
  }
  const float* x = rows + pr * D;
  for (int t = 0; t < k; ++t) {
    const int j = sup[(long)b * k + t];
    const float* y = bank + (long)j * D;
    float s = 0.0f;
    for (int c = tid; c < D; c += 256) s = fmaf(x[c], y[c], s);
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
      const float dot = (part[0] + part[1]) + (part[2] + part[3]);
      dist[t] = sqrtf(fmaxf((rn[pr] - 2.0f * dot) + bn[j], 0.0f));
    }
    __syncthreads();
  }
  if (tid == 0) {
    float m = dist[0];
    for (int t = 1; t < k; ++t) m = fmaxf(m, dist[t]);
    float z = 0.0f;
    for (int t = 0; t < k; ++t) z += expf(dist[t] - m);
    score[b] = (1.0f - expf(dist[0] - m) / z) * s_star;
  }
}

__device__ __forceinline__ int pc_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
// torch's nearest source index: min(floor(o * (float)in / out), in - 1)
__device__ __forceinline__ int pc_nearest(int o, int in, int out) {
  const int i = (int)floorf((float)o * ((float)in / (float)out));
  return i < in - 1 ? i : in - 1;
}

// nearest upsample fused into the horizontal pass: tmp[b][y][x] = sum_t g[t] up[b][y][reflect(x + t - R)]
__global__ void pc_blur_x_kernel(const float* __restrict__ s, const float* __restrict__ g, int ks, float* tmp, int B, int h,
                                 int w, int H, int W) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * H * W) return;
  const int x = (int)(i % W), y = (int)((i / W) % H), b = (int)(i / ((long)W * H));
  const float* row = s + ((long)b * h + pc_nearest(y, h, H)) * w;
  const int R = ks / 2;
  float acc = 0.0f;
  for (int t = 0; t < ks; ++t) acc = fmaf(g[t], row[pc_nearest(pc_reflect(x + t - R, W), w, W)], acc);
  tmp[i] = acc;
}

__global__ void pc_blur_y_kernel(const float* __restrict__ tmp, const float* __restrict__ g, int ks, float* out, int B,
                                 int H, int W) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * H * W) return;
  const int x = (int)(i % W), y = (int)((i / W) % H), b = (int)(i / ((long)W * H));
  const float* col = tmp + (long)b * H * W + x;
  const int R = ks / 2;
  float acc = 0.0f;
  for (int t = 0; t < ks; ++t) acc = fmaf(g[t], col[(long)pc_reflect(y + t - R, H) * W], acc);
  out[i] = acc;
}

int pc_knn_launch(int mode, const float* q, const float* qn, int N, const float* bank, const float* bn, long M, int D,
                  unsigned long long* keys, float* d2, hipStream_t st, const int32_t* list = nullptr,
                  const int32_t* count = nullptr) {
  const long ntiles = (M + PC_TN - 1) / PC_TN;
  const int rtiles = (N + PC_KNN_TM - 1) / PC_KNN_TM;
  long splits = 1024 / rtiles;                          // about four workgroups per CU in all
  if (splits < 1) splits = 1;
  if (splits > ntiles) splits = ntiles;
  const long per = (ntiles + splits - 1) / splits;
  splits = (ntiles + per - 1) / per;
  PcKnnDev d{q, qn, bank, bn, keys, d2, M, N, D, (int)per, list, count};
  const dim3 grid((unsigned)rtiles, (unsigned)splits);
  if (mode == 0)
    LD_LAUNCH(pc_knn_kernel<0>, grid, dim3(256), 0, st, d);
  else if (mode == 1)
    LD_LAUNCH(pc_knn_kernel<1>, grid, dim3(256), 0, st, d);
  else
    LD_LAUNCH(pc_knn_kernel<2>, grid, dim3(256), 0, st, d);
  return 0;
}
}  // namespace

void pc_knn_exact_listed(const float* q, const float* qn, int N, const float* bank, const float* bn, long M, int D,
                         unsigned long long* keys, const int32_t* list, const int32_t* count, hipStream_t st) {
  pc_knn_launch(2, q, qn, N, bank, bn, M, D, keys, nullptr, st, list, count);
}

extern "C" int ld_pc_conv(const ld_pc_conv_args* a, void* stream) {
  LD_REQUIRE(a, "ld_pc_conv: null args");
  LD_REQUIRE(a->ksize == 1 || a->ksize == 3, "ld_pc_conv: ksize %d (1 or 3)", a->ksize);
  LD_REQUIRE(a->stride == 1 || a->stride == 2, "ld_pc_conv: stride %d (1 or 2)", a->stride);
  LD_REQUIRE(a->B > 0 && a->Hi > 0 && a->Wi > 0, "ld_pc_conv: empty input B=%d H=%d W=%d", a->B, a->Hi, a->Wi);
  const int pad = a->ksize == 3 ? 1 : 0;
  LD_REQUIRE(a->Ho == (a->Hi + 2 * pad - a->ksize) / a->stride + 1 && a->Wo == (a->Wi + 2 * pad - a->ksize) / a->stride + 1,
             "ld_pc_conv: output %dx%d does not match input %dx%d, k %d, s %d", a->Ho, a->Wo, a->Hi, a->Wi, a->ksize,
             a->stride);
  LD_REQUIRE(a->Cin > 0 && a->Cin % PC_KC == 0, "ld_pc_conv: Cin %d (a multiple of 32)", a->Cin);
  LD_REQUIRE(a->Cout > 0 && a->Cout % PC_TN == 0, "ld_pc_conv: Cout %d (a multiple of 64)", a->Cout);
  LD_REQUIRE(a->src && a->weight && a->scale && a->shift && a->out, "ld_pc_conv: null pointer");
  const long M = (long)a->B * a->Ho * a->Wo;
  LD_REQUIRE((M + PC_CONV_TM - 1) / PC_CONV_TM < (1L << 31), "ld_pc_conv: %ld pixels", M);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((M + PC_CONV_TM - 1) / PC_CONV_TM), (unsigned)(a->Cout / PC_TN));
  LD_LAUNCH(pc_conv_kernel, grid, dim3(256), 0, st, *a);
  LD_LAUNCH_CHECK("pc_conv");
  return LD_OK;
}

extern "C" int ld_pc_stem(const float* x_nchw, const float* w_oihw, const float* scale, const float* shift, float* out,
                          int B, int H, int W, void* stream) {
  LD_REQUIRE(x_nchw && w_oihw && scale && shift && out, "ld_pc_stem: null pointer");
  LD_REQUIRE(B > 0 && H > 0 && W > 0, "ld_pc_stem: empty shape B=%d H=%d W=%d", B, H, W);
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long M = (long)B * Ho * Wo;
  LD_REQUIRE((M + 255) / 256 < (1L << 31), "ld_pc_stem: %ld pixels", M);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(pc_stem_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, x_nchw, w_oihw, scale, shift, out, B, H,
            W, Ho, Wo);
  LD_LAUNCH_CHECK("pc_stem");
  return LD_OK;
}

extern "C" int ld_pc_maxpool(const float* x, float* out, int B, int H, int W, int C, void* stream) {
  LD_REQUIRE(x && out, "ld_pc_maxpool: null pointer");
  LD_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "ld_pc_maxpool: shape B=%d H=%d W=%d C=%d", B, H, W, C);
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long total = (long)B * Ho * Wo * (C / 4);
  LD_REQUIRE((total + 255) / 256 < (1L << 31), "ld_pc_maxpool: %ld elements", total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(pc_maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, out, B, H, W, C, Ho, Wo);
  LD_LAUNCH_CHECK("pc_maxpool");
  return LD_OK;
}

extern "C" int ld_pc_embed(const float* l2, const float* l3, float* rows, float* norms, int B, int h2, int w2, int C2,
                           int h3, int w3, int C3, void* stream) {
  LD_REQUIRE(l2 && l3 && rows && norms, "ld_pc_embed: null pointer");
  LD_REQUIRE(B > 0 && h2 > 0 && w2 > 0 && h3 > 0 && w3 > 0 && C2 > 0 && C3 > 0, "ld_pc_embed: empty shape");
  const long N = (long)B * h2 * w2;
  LD_REQUIRE(N < (1L << 31), "ld_pc_embed: %ld rows", N);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(pc_embed_kernel, dim3((unsigned)N), dim3(256), 0, st, l2, l3, rows, norms, h2, w2, C2, h3, w3, C3);
  LD_LAUNCH_CHECK("pc_embed");
  return LD_OK;
}

extern "C" int ld_pc_row_norms(const float* x, float* norms, int64_t n, int d, void* stream) {
  LD_REQUIRE(x && norms, "ld_pc_row_norms: null pointer");
  LD_REQUIRE(n > 0 && d > 0 && (n + 3) / 4 < (1L << 31), "ld_pc_row_norms: n %ld d %d", (long)n, d);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(pc_row_norms_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, x, norms, (long)n, d);
  LD_LAUNCH_CHECK("pc_row_norms");
  return LD_OK;
}

extern "C" int ld_pc_knn(const float* q, const float* qn, int N, const float* bank, const float* bn, int64_t M, int D,
                         unsigned long long* work, float* dist, int32_t* idx, void* stream) {
  LD_REQUIRE(q && qn && bank && bn && work && dist && idx, "ld_pc_knn: null pointer");
  LD_REQUIRE(N > 0 && M > 0 && M < (1L << 31), "ld_pc_knn: N %d M %ld", N, (long)M);
  LD_REQUIRE(D > 0 && D % PC_KC == 0, "ld_pc_knn: D %d (a multiple of 32)", D);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(pc_knn_init_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, work, N);
  pc_knn_launch(0, q, qn, N, bank, bn, (long)M, D, work, nullptr, st);
  LD_LAUNCH(pc_knn_finish_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, work, dist, idx, N);
  LD_LAUNCH_CHECK("pc_knn");
  return LD_OK;
}

extern "C" int ld_pc_knn_topk(const float* q, const float* qn, int N, const float* bank, const float* bn, int64_t M, int D,
                              int k, float* d2, float* dist, int32_t* idx, void* stream) {
  LD_REQUIRE(q && qn && bank && bn && d2 && dist && idx, "ld_pc_knn_topk: null pointer");
  LD_REQUIRE(N > 0 && M > 0 && M < (1L << 31), "ld_pc_knn_topk: N %d M %ld", N, (long)M);
  LD_REQUIRE(D > 0 && D % PC_KC == 0, "ld_pc_knn_topk: D %d (a multiple of 32)", D);
  LD_REQUIRE(k >= 1 && k <= PC_TOPK_MAX && k <= M, "ld_pc_knn_topk: k %d (1..16, at most M = %ld)", k, (long)M);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  pc_knn_launch(1, q, qn, N, bank, bn, (long)M, D, nullptr, d2, st);
  LD_LAUNCH(pc_topk_kernel, dim3((unsigned)N), dim3(256), 0, st, d2, (long)M, k, dist, idx);
  LD_LAUNCH_CHECK("pc_knn_topk");
  return LD_OK;
}

extern "C" int ld_pc_score_prepare(const float* patch_scores, const int32_t* loc, const float* bank, const float* bn, int B,
                                   int P, int D, float* q, float* qn, int32_t* argmax, void* stream) {
  LD_REQUIRE(patch_scores && loc && bank && bn && q && qn && argmax, "ld_pc_score_prepare: null pointer");
  LD_REQUIRE(B > 0 && P > 0 && D > 0, "ld_pc_score_prepare: B %d P %d D %d", B, P, D);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(pc_score_prepare_kernel, dim3((unsigned)B), dim3(256), 0, st, patch_scores, loc, bank, bn, P, D, q, qn, argmax);
  LD_LAUNCH_CHECK("pc_score_prepare");
  return LD_OK;
}

extern "C" int ld_pc_score(const float* rows, const float* row_norms, const float* patch_scores, const int32_t* argmax,
                           const float* bank, const float* bn, const int32_t* support, int B, int P, int D, int k,
                           float* pred_score, void* stream) {
  LD_REQUIRE(rows && row_norms && patch_scores && argmax && bank && bn && pred_score && (k == 0 || support),
             "ld_pc_score: null pointer");
  LD_REQUIRE(B > 0 && P > 0 && D > 0 && k >= 0 && k <= PC_TOPK_MAX, "ld_pc_score: B %d P %d D %d k %d", B, P, D, k);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(pc_score_kernel, dim3((unsigned)B), dim3(256), 0, st, rows, row_norms, patch_scores, argmax, bank, bn, support,
            P, D, k, pred_score);
  LD_LAUNCH_CHECK("pc_score");
  return LD_OK;
}

extern "C" int ld_pc_anomaly_map(const float* scores, const float* g, int ks, float* tmp, float* out, int B, int h, int w,
                                 int H, int W, void* stream) {
  LD_REQUIRE(scores && g && tmp && out, "ld_pc_anomaly_map: null pointer");
  LD_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "ld_pc_anomaly_map: empty shape");
  LD_REQUIRE(ks > 0 && ks % 2 == 1 && ks / 2 < H && ks / 2 < W,
             "ld_pc_anomaly_map: kernel size %d (odd, reflect padding %d below the map size %dx%d)", ks, ks / 2, H, W);
  const long total = (long)B * H * W;
  LD_REQUIRE((total + 255) / 256 < (1L << 31), "ld_pc_anomaly_map: %ld pixels", total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((total + 255) / 256));
  LD_LAUNCH(pc_blur_x_kernel, grid, dim3(256), 0, st, scores, g, ks, tmp, B, h, w, H, W);
  LD_LAUNCH(pc_blur_y_kernel, grid, dim3(256), 0, st, tmp, g, ks, out, B, H, W);
  LD_LAUNCH_CHECK("pc_anomaly_map");
  return LD_OK;
}
