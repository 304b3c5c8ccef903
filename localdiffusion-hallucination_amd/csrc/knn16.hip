// PatchCore's nearest-neighbour search with the fp16 matrix cores as a SCREEN and an exact fp32 re-rank
// (PatchCore.knn_precision = "fp16").  The answer is the one an fp32 search gives: for every query the argmin, lowest
// index on ties, of the re-rank distance r over ALL bank rows, or, for a query that could not be certified, exactly
// what ld_pc_knn returns.  The re-rank sums in pc_knn_kernel's own order (v_mfma_f32_32x32x2_f32 is a k-ordered fmaf
// chain), so r is ld_pc_knn's d2 and the two statements are one: the result is ld_pc_knn's.  tests/knn16_ref.py is the
// same arithmetic in torch; docs/findings.md 138 has the numbers.
//
//   1. split     x_hi = fp16_rne(x), x_lo = fp16_rne(x - float(x_hi)) (the subtraction is exact in fp32), so
//                |x - x_hi - x_lo| <= 2^-22 |x| + 2^-25 (the second term: a lo in fp16's subnormal range, |x| < 2^-3).
//                The bank once per bank (ld_pc_pack_bank16), the queries per call (k16_pack_q_kernel).
//   2. screen    s = max((qn - 2 dot16) + bn, 0), qn / bn the caller's fp32 |.|^2 of the unrounded rows,
//                dot16 = q_hi.m_hi + (q_hi.m_lo + q_lo.m_hi) on v_mfma_f32_32x32x16_f16: hi.hi in P = 4 accumulators
//                (K-step mod 4), the two lo terms in one.  dot16 = ((hh0 + hh1) + (hh2 + hh3)) + lo.
//   3. collect   pass A: min of s per query (64-bit atomicMin of (s, row) keys);  window: thr = s_min + W;
//                pass B: every (query, row) with s <= thr goes into the query's segment of LD_PC_KNN16_CAND entries
//                (an integer atomic counter per query; the order in a segment does not matter).
//   4. re-rank   one wave per candidate: r = max((qn - 2 dot32) + bn, 0) from the fp32 rows, dot32 = ONE fmaf chain
//                over k = 0, 1, ... D - 1 from 0.0f (what pc_knn_kernel's accumulator holds); atomicMin of (r, row) keys.
//   5. fallback  a query whose segment overflowed, whose s_min / W / norm is not finite or that holds |x| > 65504 is
//                uncertified: such queries are listed on the device and searched by pc_knn_kernel<2> (exact f32).
//
// The bound.  With t = max((qn - 2 q.m) + bn, 0) in exact arithmetic on the same fp32 qn, bn (they enter s, r and t
// alike, so their own rounding cancels), a = |q|, b = |m| <= b_max:
//   * dropped and rounded operand parts: q.m - dot16(exact sums) = q_lo.m_lo + dq.m + (q_hi + q_lo).dm with |q_lo| <=
//     2^-11 |q|, |dq| <= 2^-22 |q| + 2^-25 elementwise: at most 3 * 2^-22 a b + 2^-25 sqrt(D) (a + b); 2^-20 a b covers
//     the first term and every second-order product (|q_hi| <= (1 + 2^-11) |q|, (1 + u)^L - 1 <= L u (1 + 2^-11) ...).
//   * fp16 x fp16 products are exact in fp32.  Each of the L = D / P + P additions that an hi.hi accumulator element
//     sees (D / P products, then the merges and the + lo) errs by at most 2^-23 of the partial sum ("no worse than
//     truncation": the hardware check is the screen test), the partial sums are at most sum |q_k m_k| <= a b.  The
//     lo chain has 2 D + 2 additions on terms 2^-10 as large.
//     gamma = 2^-20 + L 2^-23 + (2 D + 2) 2^-33,   |dot16 - q.m| <= gamma a b + 2^-25 sqrt(D) (a + b)
//   * the two roundings of (qn - 2 dot) + bn: 2^-24 (2 qn + bn) + 2^-24 (2 qn + 2 bn) <= 2^-22 (qn + bn); max(., 0) is
//     1-Lipschitz.
//     eps_s(q) = 2 gamma a b_max + 2^-22 (qn + bn_max) + 2^-24 sqrt(D) (a + b_max)
//     eps_r(q) = 2 D 2^-24 a b_max + 2^-22 (qn + bn_max)                         (an fmaf chain of D roundings)
//     W(q)     = 2 (eps_s + eps_r) (1 + 2^-10)          (the factor: a = sqrt(qn) is itself rounded, in double here)
//   For a row outside the window r(m) >= s(m) - eps_s - eps_r > s_min + W - eps_s - eps_r >= r(argmin s): it cannot
//   hold the smallest r, ties included.
//
// The screen kernel: 4 waves own a 128 (queries) x 64 (bank rows) tile, 2 x 2 waves of 64 x 32, K in chunks of 64 halves
// staged through LDS as row-major [row][64] images of hi and lo with a 144-byte pitch (a ds_read_b128 of rows r, k
// fixed, touches 16-byte slot (9 r + c) mod 16: conflict-free over the 16 rows of a lane group), the next chunk's global
// loads in registers over the current chunk's 24 MFMAs per wave.  A lane's fragment is eight consecutive halves of one
// row for both operands (both are K-contiguous rows), so the k order inside the MFMA is the same on both sides.
#include "common.hip.h"
#include "pc_knn.hip.h"

namespace {
constexpr int K16_TM = 128;      // query rows per workgroup
constexpr int K16_TN = 64;       // bank rows per tile
constexpr int K16_KC = 64;       // halves of K per chunk
constexpr int K16_P = 4;         // partial hi.hi accumulators
constexpr int K16_PITCH = 144;   // bytes per LDS row: 128 + 16
constexpr float K16_F16_MAX = 65504.0f;
typedef __attribute__((ext_vector_type(16))) float k16_f32x16;

struct K16Smem {
  unsigned char qh[K16_TM * K16_PITCH], ql[K16_TM * K16_PITCH];
  unsigned char bh[K16_TN * K16_PITCH], bl[K16_TN * K16_PITCH];
  float qn[K16_TM], thr[K16_TM];
};

struct K16Dev {
  const f16* qh; const f16* ql; const float* qn;
  const f16* bh; const f16* bl; const float* bn;
  unsigned long long* keys;   // MODE 0: [N] running minimum of (s, row)
  const float* thr;           // MODE 1: [N] s_min + W (-inf: collect nothing)
  int32_t* cnt;               // MODE 1: [N] rows inside the window
  int32_t* cand;              // MODE 1: [N, LD_PC_KNN16_CAND]
  float* s_out;               // MODE 2: [N, M]
  long M; int N, D, tiles_per_split;
};

__device__ __forceinline__ void k16_split(float x, f16& hi, f16& lo) {
  hi = (f16)x;                        // v_cvt_f16_f32, round-to-nearest-even, subnormals kept
  lo = (f16)(x - (float)hi);          // exact subtraction; inf - inf = NaN for |x| > 65504 (refused / uncertified)
}

// MODE 0: pass A.  MODE 1: pass B.  MODE 2: the screened distances themselves (test instrument).
template <int MODE>
__global__ __launch_bounds__(256) void k16_screen_kernel(K16Dev a) {
  __shared__ __attribute__((aligned(16))) K16Smem sm;
  constexpr int NB = K16_TM / 64, UQ = K16_TM / 32, UB = K16_TN / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int lr = tid >> 3, ls = tid & 7;               // loader: row lr + 32 u, 16-byte segment ls of the chunk
  const int row0 = blockIdx.x * K16_TM;
  const long ntiles = (a.M + K16_TN - 1) / K16_TN;
  const long t0 = (long)blockIdx.y * a.tiles_per_split;
  const long t1 = t0 + a.tiles_per_split < ntiles ? t0 + a.tiles_per_split : ntiles;
  const int nq = (a.D + K16_KC - 1) / K16_KC;          // D is a multiple of 32: the last chunk may be half zeros
  long qoff[UQ];
#pragma unroll
  for (int u = 0; u < UQ; ++u) {
    const int r = row0 + lr + 32 * u;
    qoff[u] = (long)(r < a.N ? r : a.N - 1) * a.D;              // padding rows read a real row, never stored
  }
  auto arow = [&](int m, int r) { return wm * (K16_TM / 2) + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); };
  if (tid < K16_TM) {                                  // (the first barrier of the chunk loop orders these writes)
    const int i = row0 + tid;
    sm.qn[tid] = a.qn[i < a.N ? i : a.N - 1];
    if constexpr (MODE == 1) sm.thr[tid] = i < a.N ? a.thr[i] : -__builtin_inff();   // padding rows collect nothing
  }
  float best[MODE == 0 ? NB : 1][16];                  // MODE 0: the running minimum and its row
  unsigned bidx[MODE == 0 ? NB : 1][16];
  if constexpr (MODE == 0) {
#pragma unroll
    for (int m = 0; m < NB; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) { best[m][r] = __builtin_inff(); bidx[m][r] = 0xffffffffu; }
  }
  const int fr = lane & 31, fh = lane >> 5;             // fragment: row fr of the wave's block, halves 8 fh .. 8 fh + 7
  for (long tile = t0; tile < t1; ++tile) {
    const long m0 = tile * K16_TN;
    long boff[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const long j = m0 + lr + 32 * u;
      boff[u] = (j < a.M ? j : a.M - 1) * a.D;
    }
    uint4 rqh[UQ], rql[UQ], rbh[UB], rbl[UB];
    auto load = [&](int q) {                            // beyond D (the last chunk's second half): zeros
      const bool in = q * K16_KC + ls * 8 < a.D;
      const int k = in ? q * K16_KC + ls * 8 : 0;        // (out of the row: its first 16 bytes, masked to zero)
      const unsigned keep = in ? ~0u : 0u;
      auto ld = [&](const f16* p) {
        uint4 v = *reinterpret_cast<const uint4*>(p + k);
        v.x &= keep; v.y &= keep; v.z &= keep; v.w &= keep;
        return v;
      };
#pragma unroll
      for (int u = 0; u < UQ; ++u) { rqh[u] = ld(a.qh + qoff[u]); rql[u] = ld(a.ql + qoff[u]); }
#pragma unroll
      for (int u = 0; u < UB; ++u) { rbh[u] = ld(a.bh + boff[u]); rbl[u] = ld(a.bl + boff[u]); }
    };
    k16_f32x16 hh[NB][K16_P], lo[NB];
#pragma unroll
    for (int m = 0; m < NB; ++m) {
#pragma unroll
      for (int r = 0; r < 16; ++r) lo[m][r] = 0.0f;
#pragma unroll
      for (int p = 0; p < K16_P; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) hh[m][p][r] = 0.0f;
    }
    load(0);
    for (int q = 0; q < nq; ++q) {
      __syncthreads();                                  // the previous chunk's reads of the images are done
#pragma unroll
      for (int u = 0; u < UQ; ++u) {
        const int o = (lr + 32 * u) * K16_PITCH + ls * 16;
        *reinterpret_cast<uint4*>(sm.qh + o) = rqh[u];
        *reinterpret_cast<uint4*>(sm.ql + o) = rql[u];
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int o = (lr + 32 * u) * K16_PITCH + ls * 16;
        *reinterpret_cast<uint4*>(sm.bh + o) = rbh[u];
        *reinterpret_cast<uint4*>(sm.bl + o) = rbl[u];
      }
      __syncthreads();
      if (q + 1 < nq) load(q + 1);
#pragma unroll
      for (int ks = 0; ks < K16_KC / 16; ++ks) {        // K-step ks of the chunk feeds hi.hi accumulator ks
        const int ob = (wn * 32 + fr) * K16_PITCH + ks * 32 + fh * 16;
        const f16x8 bh = *reinterpret_cast<const f16x8*>(sm.bh + ob);
        const f16x8 bl = *reinterpret_cast<const f16x8*>(sm.bl + ob);
#pragma unroll
        for (int m = 0; m < NB; ++m) {
          const int oa = (wm * (K16_TM / 2) + m * 32 + fr) * K16_PITCH + ks * 32 + fh * 16;
          const f16x8 ah = *reinterpret_cast<const f16x8*>(sm.qh + oa);
          const f16x8 al = *reinterpret_cast<const f16x8*>(sm.ql + oa);
          hh[m][ks] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, hh[m][ks], 0, 0, 0);
          lo[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, lo[m], 0, 0, 0);
          lo[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, lo[m], 0, 0, 0);
        }
      }
    }
    const long j = m0 + wn * 32 + (lane & 31);
    if (j >= a.M) continue;
    const float bnj = a.bn[j];
#pragma unroll
    for (int m = 0; m < NB; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ar = arow(m, r);
        const float dot = ((hh[m][0][r] + hh[m][1][r]) + (hh[m][2][r] + hh[m][3][r])) + lo[m][r];
        const float s = fmaxf((sm.qn[ar] - 2.0f * dot) + bnj, 0.0f);
        if constexpr (MODE == 0) {
          if (s < best[m][r]) { best[m][r] = s; bidx[m][r] = (unsigned)j; }    // columns rise: the first index stays
        } else if constexpr (MODE == 1) {
          if (s <= sm.thr[ar]) {
            const int i = row0 + ar;
            const int slot = atomicAdd(a.cnt + i, 1);
            if (slot < LD_PC_KNN16_CAND) a.cand[(long)i * LD_PC_KNN16_CAND + slot] = (int32_t)j;
          }
        } else {
          const int i = row0 + ar;
          if (i < a.N) a.s_out[(long)i * a.M + j] = s;
        }
      }
  }
  if constexpr (MODE == 0) {
#pragma unroll
    for (int m = 0; m < NB; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        unsigned long long k = bidx[m][r] == 0xffffffffu ? ~0ull : pc_key(best[m][r], bidx[m][r]);
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {                // the 32 lanes of a half-wave hold the same query
          const unsigned long long k2 = pc_shfl_xor64(k, o);
          k = k2 < k ? k2 : k;
        }
        const int i = row0 + arow(m, r);
        if ((lane & 31) == 0 && i < a.N && k != ~0ull) atomicMin(a.keys + i, k);
      }
  }
}

// hi / lo of 8 consecutive elements per thread; clears info[1] when one is not finite in fp16 (flag may be null)
__global__ __launch_bounds__(256) void k16_pack_kernel(const float* __restrict__ x, f16* hi, f16* lo, long n8,
                                                       uint32_t* flag) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const float4 v0 = *reinterpret_cast<const float4*>(x + i * 8), v1 = *reinterpret_cast<const float4*>(x + i * 8 + 4);
  const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
  f16x8 h, l;
  bool ok = true;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f16 a, b;
    k16_split(v[e], a, b);
    h[e] = a; l[e] = b;
    ok = ok && fabsf(v[e]) <= K16_F16_MAX;               // false for NaN
  }
  *reinterpret_cast<f16x8*>(hi + i * 8) = h;
  *reinterpret_cast<f16x8*>(lo + i * 8) = l;
  if (flag && !ok) atomicMin(flag, 0u);                   // the bits of 1.0f -> 0.0f
}

__global__ void k16_info_init_kernel(uint32_t* info) {
  info[0] = 0u;                                           // 0.0f: the identity of the maximum of |m|^2 >= 0
  info[1] = __float_as_uint(1.0f);
}
// the largest of norms [n] (>= 0, so the bit patterns order as the values; a NaN's bits are above every number's)
__global__ __launch_bounds__(256) void k16_norm_max_kernel(const float* __restrict__ norms, long n, uint32_t* info) {
  unsigned m = 0u;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const unsigned b = __float_as_uint(norms[i]) & 0x7fffffffu;
    m = b > m ? b : m;
  }
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned m2 = __shfl_xor(m, o);
    m = m2 > m ? m2 : m;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(info, m);
}

// Per-query state of one ld_pc_knn16 call, carved out of the caller's work buffer
struct K16Work {
  f16* qh; f16* ql;
  unsigned long long* keys_a; unsigned long long* keys_r; unsigned long long* keys_x;   // screen, re-rank, exact
  float* thr; int32_t* cnt; int32_t* qbad; int32_t* unc; int32_t* list; int32_t* cand; int32_t* fbcount;
};
__host__ size_t k16_work_bytes(long N, int D, K16Work* w, unsigned char* base) {
  size_t o = 0;
  auto take = [&](size_t bytes) { unsigned char* p = base + o; o += (bytes + 15) & ~(size_t)15; return p; };
  unsigned char* p;
  p = take((size_t)N * D * 2); if (w) w->qh = reinterpret_cast<f16*>(p);
  p = take((size_t)N * D * 2); if (w) w->ql = reinterpret_cast<f16*>(p);
  p = take((size_t)N * 8); if (w) w->keys_a = reinterpret_cast<unsigned long long*>(p);
  p = take((size_t)N * 8); if (w) w->keys_r = reinterpret_cast<unsigned long long*>(p);
  p = take((size_t)N * 8); if (w) w->keys_x = reinterpret_cast<unsigned long long*>(p);
  p = take((size_t)N * 4); if (w) w->thr = reinterpret_cast<float*>(p);
  p = take((size_t)N * 4); if (w) w->cnt = reinterpret_cast<int32_t*>(p);
  p = take((size_t)N * 4); if (w) w->qbad = reinterpret_cast<int32_t*>(p);
  p = take((size_t)N * 4); if (w) w->unc = reinterpret_cast<int32_t*>(p);
  p = take((size_t)N * 4); if (w) w->list = reinterpret_cast<int32_t*>(p);
  p = take((size_t)N * LD_PC_KNN16_CAND * 4); if (w) w->cand = reinterpret_cast<int32_t*>(p);
  p = take(16); if (w) w->fbcount = reinterpret_cast<int32_t*>(p);
  return o;
}

__global__ void k16_init_kernel(K16Work w, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4) w.fbcount[i] = 0;                         // [0] uncertified queries, [1] rows inside all windows, [2] the most
  if (i >= N) return;
  w.keys_a[i] = ~0ull; w.keys_r[i] = ~0ull; w.keys_x[i] = ~0ull;
  w.cnt[i] = 0; w.qbad[i] = 0;
}

// the queries' split, one wave per row; qbad[row] = 1 when an element is not finite in fp16 (qbad may be null)
__global__ __launch_bounds__(256) void k16_pack_q_kernel(const float* __restrict__ q, f16* qh, f16* ql, int N, int D,
                                                         int32_t* qbad) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const long base = (long)row * D;
  bool ok = true;
  for (int c = (threadIdx.x & 63) * 4; c < D; c += 256) {
    const float4 v4 = *reinterpret_cast<const float4*>(q + base + c);
    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
    f16 h[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      k16_split(v[e], h[e], l[e]);
      ok = ok && fabsf(v[e]) <= K16_F16_MAX;
    }
    typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
    const f16x4 hv = {h[0], h[1], h[2], h[3]}, lv = {l[0], l[1], l[2], l[3]};
    *reinterpret_cast<f16x4*>(qh + base + c) = hv;
    *reinterpret_cast<f16x4*>(ql + base + c) = lv;
  }
  if (qbad && __any(!ok) && (threadIdx.x & 63) == 0) qbad[row] = 1;
}

// thr = s_min + W(q), rounded up; -inf (collect nothing, fall back) when the query cannot be certified at this point
__global__ void k16_window_kernel(K16Work w, const float* __restrict__ qn, const float* __restrict__ info, int N, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const unsigned long long key = w.keys_a[i];
  const double smin = (double)__uint_as_float((unsigned)(key >> 32));
  const double q2 = (double)qn[i], b2 = (double)info[0];
  const double a = sqrt(q2), b = sqrt(b2), rtD = sqrt((double)D);
  const double L = (double)(D / K16_P + K16_P), Llo = 2.0 * D + 2.0, Lr = (double)D;
  const double gamma = 0x1p-20 + L * 0x1p-23 + Llo * 0x1p-33;
  const double eps_s = 2.0 * gamma * a * b + 0x1p-22 * (q2 + b2) + 0x1p-24 * rtD * (a + b);
  const double eps_r = 2.0 * Lr * 0x1p-24 * a * b + 0x1p-22 * (q2 + b2);
  const double W = 2.0 * (eps_s + eps_r) * (1.0 + 0x1p-10);
  const double t = smin + W;
  float thr = (float)t;
  if ((double)thr < t) thr = __uint_as_float(__float_as_uint(thr) + 1u);      // t >= 0: the next float up
  const bool ok = key != ~0ull && w.qbad[i] == 0 && q2 >= 0.0 && t < 3.0e38;   // false for a NaN in smin, W or qn
  w.thr[i] = ok ? thr : -__builtin_inff();
  w.qbad[i] = ok ? 0 : 1;
}

// one wave per (query, slot): r from the fp32 rows, atomicMin of (r, row) into the query's re-rank key
__global__ __launch_bounds__(256) void k16_rerank_kernel(K16Work w, const float* __restrict__ q, const float* __restrict__ qn,
                                                         const float* __restrict__ bank, const float* __restrict__ bn,
                                                         int N, int D) {
  const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int i = (int)(wid / LD_PC_KNN16_CAND), slot = (int)(wid % LD_PC_KNN16_CAND);
  if (i >= N) return;
  const int n = w.cnt[i];
  if (n > LD_PC_KNN16_CAND || slot >= n) return;        // an overflowed segment is searched exactly instead
  const int j = w.cand[(long)i * LD_PC_KNN16_CAND + slot];
  const float* x = q + (long)i * D;
  const float* y = bank + (long)j * D;
  // pc_knn_kernel's accumulator: fma(x_k, y_k, acc) for k = 0, 1, ... in turn.  The wave loads 64 elements of both rows
  // at once and every lane runs the same chain on them, lane k's pair broadcast by v_readlane.
  const int lane = threadIdx.x & 63;
  auto bc = [](float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); };
  float s = 0.0f;
  for (int k0 = 0; k0 < D; k0 += 64) {
    const int c = k0 + lane;
    const float xv = c < D ? x[c] : 0.0f, yv = c < D ? y[c] : 0.0f;
#pragma unroll
    for (int k = 0; k < 32; ++k) s = fmaf(bc(xv, k), bc(yv, k), s);
    if (k0 + 32 < D) {                                  // D is a multiple of 32: the last load may be half a wave
#pragma unroll
      for (int k = 32; k < 64; ++k) s = fmaf(bc(xv, k), bc(yv, k), s);
    }
  }
  const float r = fmaxf((qn[i] - 2.0f * s) + bn[j], 0.0f);
  if ((threadIdx.x & 63) == 0 && r == r) atomicMin(w.keys_r + i, pc_key(r, (unsigned)j));
}

// uncertified queries -> list (an integer atomic counter; their results do not depend on the order in the list)
__global__ void k16_compact_kernel(K16Work w, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int n = w.cnt[i];
  const bool unc = w.qbad[i] != 0 || n < 1 || n > LD_PC_KNN16_CAND || w.keys_r[i] == ~0ull;
  w.unc[i] = unc ? 1 : 0;
  if (unc) w.list[atomicAdd(w.fbcount, 1)] = i;
  atomicAdd(w.fbcount + 1, n);                          // (integer sums: any order gives the same)
  atomicMax(w.fbcount + 2, n);
}

__global__ void k16_finish_kernel(K16Work w, float* dist, int32_t* idx, int32_t* stats, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && stats) { stats[0] = N - w.fbcount[0]; stats[1] = w.fbcount[0]; stats[2] = w.fbcount[1]; stats[3] = w.fbcount[2]; }
  if (i >= N) return;
  const unsigned long long k = w.unc[i] ? w.keys_x[i] : w.keys_r[i];
  if (k == ~0ull) {                                     // no finite distance at all (NaN input): as ld_pc_knn
    dist[i] = __builtin_nanf("");
    idx[i] = 0;
    return;
  }
  dist[i] = sqrtf(__uint_as_float((unsigned)(k >> 32)));
  idx[i] = (int32_t)(unsigned)(k & 0xffffffffu);
}

void k16_screen_launch(int mode, K16Dev d, hipStream_t st) {
  const long ntiles = (d.M + K16_TN - 1) / K16_TN;
  const int rtiles = (d.N + K16_TM - 1) / K16_TM;
  long splits = 1024 / rtiles;                          // about four workgroups per CU in all
  if (splits < 1) splits = 1;
  if (splits > ntiles) splits = ntiles;
  const long per = (ntiles + splits - 1) / splits;
  splits = (ntiles + per - 1) / per;
  d.tiles_per_split = (int)per;
  const dim3 grid((unsigned)rtiles, (unsigned)splits);
  if (mode == 0)
    LD_LAUNCH(k16_screen_kernel<0>, grid, dim3(256), 0, st, d);
  else if (mode == 1)
    LD_LAUNCH(k16_screen_kernel<1>, grid, dim3(256), 0, st, d);
  else
    LD_LAUNCH(k16_screen_kernel<2>, grid, dim3(256), 0, st, d);
}
bool k16_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

extern "C" int ld_pc_pack_bank16(const float* bank, const float* bn, int64_t M, int D, void* bank_hi, void* bank_lo,
                                 float* info, void* stream) {
  LD_REQUIRE(bank && bn && bank_hi && bank_lo && info, "ld_pc_pack_bank16: null pointer");
  LD_REQUIRE(M > 0 && M < (1L << 31), "ld_pc_pack_bank16: M %ld", (long)M);
  LD_REQUIRE(D > 0 && D % 32 == 0, "ld_pc_pack_bank16: D %d (a multiple of 32)", D);
  LD_REQUIRE(k16_aligned(bank) && k16_aligned(bank_hi) && k16_aligned(bank_lo), "ld_pc_pack_bank16: 16-byte alignment");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  uint32_t* iw = reinterpret_cast<uint32_t*>(info);
  const long n8 = (long)M * D / 8;
  LD_LAUNCH(k16_info_init_kernel, dim3(1), dim3(1), 0, st, iw);
  LD_LAUNCH(k16_pack_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, bank, reinterpret_cast<f16*>(bank_hi),
            reinterpret_cast<f16*>(bank_lo), n8, iw + 1);
  const long nb = (M + 255) / 256;
  LD_LAUNCH(k16_norm_max_kernel, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, st, bn, (long)M, iw);
  LD_LAUNCH_CHECK("pc_pack_bank16");
  return LD_OK;
}

extern "C" int64_t ld_pc_knn16_work_bytes(int N, int D) {
  if (N <= 0 || D <= 0) return 0;
  return (int64_t)k16_work_bytes(N, D, nullptr, nullptr);
}

extern "C" int ld_pc_knn16(const float* q, const float* qn, int N, const float* bank, const void* bank_hi,
                           const void* bank_lo, const float* bn, const float* info, int64_t M, int D, void* work,
                           float* dist, int32_t* idx, int32_t* stats, void* stream) {
  LD_REQUIRE(q && qn && bank && bank_hi && bank_lo && bn && info && work && dist && idx, "ld_pc_knn16: null pointer");
  LD_REQUIRE(N > 0 && M > 0 && M < (1L << 31), "ld_pc_knn16: N %d M %ld", N, (long)M);
  LD_REQUIRE(D > 0 && D % 32 == 0, "ld_pc_knn16: D %d (a multiple of 32)", D);
  LD_REQUIRE((long)N * LD_PC_KNN16_CAND / 4 + 1 < (1L << 31), "ld_pc_knn16: N %d", N);
  LD_REQUIRE(k16_aligned(q) && k16_aligned(bank_hi) && k16_aligned(bank_lo) && k16_aligned(work),
             "ld_pc_knn16: 16-byte alignment");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  K16Work w;
  k16_work_bytes(N, D, &w, reinterpret_cast<unsigned char*>(work));
  const dim3 pq((unsigned)((N + 255) / 256));
  LD_LAUNCH(k16_init_kernel, pq, dim3(256), 0, st, w, N);
  LD_LAUNCH(k16_pack_q_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, q, w.qh, w.ql, N, D, w.qbad);
  K16Dev d{w.qh, w.ql, qn, reinterpret_cast<const f16*>(bank_hi), reinterpret_cast<const f16*>(bank_lo), bn,
           w.keys_a, w.thr, w.cnt, w.cand, nullptr, (long)M, N, D, 0};
  k16_screen_launch(0, d, st);
  LD_LAUNCH(k16_window_kernel, pq, dim3(256), 0, st, w, qn, info, N, D);
  k16_screen_launch(1, d, st);
  const long waves = (long)N * LD_PC_KNN16_CAND;
  LD_LAUNCH(k16_rerank_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, w, q, qn, bank, bn, N, D);
  LD_LAUNCH(k16_compact_kernel, pq, dim3(256), 0, st, w, N);
  pc_knn_exact_listed(q, qn, N, bank, bn, (long)M, D, w.keys_x, w.list, w.fbcount, st);
  LD_LAUNCH(k16_finish_kernel, pq, dim3(256), 0, st, w, dist, idx, stats, N);
  LD_LAUNCH_CHECK("pc_knn16");
  return LD_OK;
}

extern "C" int ld_pc_knn16_screen(const float* q, const float* qn, int N, const void* bank_hi, const void* bank_lo,
                                  const float* bn, int64_t M, int D, void* work, float* s_out, void* stream) {
  LD_REQUIRE(q && qn && bank_hi && bank_lo && bn && work && s_out, "ld_pc_knn16_screen: null pointer");
  LD_REQUIRE(N > 0 && M > 0 && M < (1L << 31), "ld_pc_knn16_screen: N %d M %ld", N, (long)M);
  LD_REQUIRE(D > 0 && D % 32 == 0, "ld_pc_knn16_screen: D %d (a multiple of 32)", D);
  LD_REQUIRE(k16_aligned(q) && k16_aligned(bank_hi) && k16_aligned(bank_lo) && k16_aligned(work),
             "ld_pc_knn16_screen: 16-byte alignment");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  K16Work w;
  k16_work_bytes(N, D, &w, reinterpret_cast<unsigned char*>(work));
  LD_LAUNCH(k16_pack_q_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, q, w.qh, w.ql, N, D,
            static_cast<int32_t*>(nullptr));
  K16Dev d{w.qh, w.ql, qn, reinterpret_cast<const f16*>(bank_hi), reinterpret_cast<const f16*>(bank_lo), bn,
           nullptr, nullptr, nullptr, nullptr, s_out, (long)M, N, D, 0};
  k16_screen_launch(2, d, st);
  LD_LAUNCH_CHECK("pc_knn16_screen");
  return LD_OK;
}
