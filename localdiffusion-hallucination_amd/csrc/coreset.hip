// PatchCore memory-bank construction (anomaly_model_train.py:339-385, models.py:165-172): anomalib's KCenterGreedy
// coreset over the embedding rows E [N, D].  fp32 throughout.
//
//   * pc_project_kernel: F = E @ R^T with the sparse random projection R [k, D] in CSR form.  F is written
//     feature-major, Ft [k, ld] (ld >= N, a multiple of 4): the greedy loop then streams it with one lane per row
//     group, coalesced, with no cross-lane reduction.  A workgroup stages 8 rows of E in LDS as [column][row] (one
//     coalesced read of E, from HBM once), and each thread computes the 8 rows of one output feature j from R's row j;
//   * pc_coreset_step_kernel: one greedy step.  The previous step's winner is decoded from a 64-bit key in device
//     memory (float bits of min_d << 32 | 0xFFFFFFFF - row: monotone for min_d >= 0, the lowest row on ties, as
//     torch.argmax), its k features are gathered into LDS, every row's min_d is updated with
//     |x - c + 1e-6|_2 (F.pairwise_distance), the winner's own entry forced to 0, and each workgroup's maximum key goes
//     to keys[step] by one atomicMax.  One launch per step: the kernel boundary is the only dependency, no host sync;
//   * pc_coreset_finish_kernel: keys -> int64 row indices.
//
// Each row's distance is summed in feature order by one thread, so the picks are the same from run to run.
#include "common.hip.h"

namespace {
constexpr int PJ_ROWS = 8;         // rows of E per projection workgroup
constexpr int PJ_THREADS = 256;
constexpr int PJ_MAX_D = 2048;     // PJ_ROWS x D floats of LDS (64 KiB at most)
constexpr int CS_THREADS = 128;    // greedy step: 2 waves, 4 rows per lane (one float4 of each feature row of Ft)
constexpr int CS_ROWS = CS_THREADS * 4;
constexpr int CS_MAX_K = 8192;     // the centre's features in LDS (32 KiB at most)

__global__ __launch_bounds__(PJ_THREADS) void pc_project_kernel(const float* __restrict__ e, long N, int D,
                                                                const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ cols,
                                                                const float* __restrict__ vals, int k, float* out,
                                                                long ld) {
  extern __shared__ __attribute__((aligned(16))) float et[];     // [D][PJ_ROWS]
  const long row0 = (long)blockIdx.x * PJ_ROWS;
  const int tid = threadIdx.x, nq = D / 4;
  // thread -> (row tid % 8, float4 column tid / 8 + 32 u): 8 lanes read one column's float4 of the 8 rows, 32 lanes per
  // row read 512 contiguous bytes of it
  for (int f = tid; f < nq * PJ_ROWS; f += PJ_THREADS) {
    const int r = f & (PJ_ROWS - 1), q = f >> 3;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row0 + r < N) v = *reinterpret_cast<const f32x4*>(e + (row0 + r) * D + 4 * q);
    et[(4 * q + 0) * PJ_ROWS + r] = v.x;
    et[(4 * q + 1) * PJ_ROWS + r] = v.y;
    et[(4 * q + 2) * PJ_ROWS + r] = v.z;
    et[(4 * q + 3) * PJ_ROWS + r] = v.w;
  }
  __syncthreads();
  const f32x4* et4 = reinterpret_cast<const f32x4*>(et);
  for (int j = tid; j < k; j += PJ_THREADS) {
    f32x4 a = {0.0f, 0.0f, 0.0f, 0.0f}, b = {0.0f, 0.0f, 0.0f, 0.0f};
    const int p1 = rowptr[j + 1];
#pragma unroll 4
    for (int p = rowptr[j]; p < p1; ++p) {
      const int c = cols[p];
      if ((unsigned)c >= (unsigned)D) continue;                    // a bad column index reads nothing
      const float v = vals[p];
      a += v * et4[2 * c];
      b += v * et4[2 * c + 1];
    }
    float* o = out + (long)j * ld + row0;
    if (row0 + PJ_ROWS <= N) {
      reinterpret_cast<f32x4*>(o)[0] = a;
      reinterpret_cast<f32x4*>(o)[1] = b;
    } else {
      const float t[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      for (int r = 0; r < PJ_ROWS && row0 + r < N; ++r) o[r] = t[r];
    }
  }
}

__device__ __forceinline__ unsigned long long cs_shfl_xor64(unsigned long long v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
  return ((unsigned long long)hi << 32) | lo;
}

// The row a key names (keys hold 0xFFFFFFFF - row so that atomicMax prefers the lower row on equal distances).
__device__ __forceinline__ long cs_key_row(unsigned long long key) { return (long)(0xffffffffu - (unsigned)key); }

__global__ __launch_bounds__(CS_THREADS) void pc_coreset_step_kernel(const float* __restrict__ ft, long ld, long N, int k,
                                                                     float* min_d, unsigned long long* keys, long step,
                                                                     long start) {
  extern __shared__ float cen[];                                   // [k]: the centre's features
  __shared__ unsigned long long wmax[CS_THREADS / 64];
  const int tid = threadIdx.x;
  const long w = step == 0 ? start : cs_key_row(keys[step - 1]);
  for (int j = tid; j < k; j += CS_THREADS) cen[j] = ft[(long)j * ld + w];
  __syncthreads();
  const long r0 = ((long)blockIdx.x * CS_THREADS + tid) * 4;
  unsigned long long best = 0;                                     // below every real key (row 0xFFFFFFFF cannot exist)
  if (r0 < N) {
    const float* p = ft + r0;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 8
    for (int j = 0; j < k; ++j) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(p + (long)j * ld);
      f32x4 d = x - cen[j];
      d += 1e-6f;
      acc += d * d;
    }
    f32x4 m = {sqrtf(acc.x), sqrtf(acc.y), sqrtf(acc.z), sqrtf(acc.w)};
    if (step > 0) {
      const f32x4 old = *reinterpret_cast<const f32x4*>(min_d + r0);
#pragma unroll
      for (int q = 0; q < 4; ++q) m[q] = old[q] < m[q] ? old[q] : m[q];
      if (w >= r0 && w < r0 + 4) m[w - r0] = 0.0f;                // the previous pick leaves the candidates
    }
    *reinterpret_cast<f32x4*>(min_d + r0) = m;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (r0 + q < N) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(m[q]) << 32) | (0xffffffffu - (unsigned)(r0 + q));
        best = key > best ? key : best;
      }
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long b2 = cs_shfl_xor64(best, o);
    best = b2 > best ? b2 : best;
  }
  if ((tid & 63) == 0) wmax[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < CS_THREADS / 64; ++i) best = wmax[i] > best ? wmax[i] : best;
    atomicMax(keys + step, best);
  }
}

__global__ void pc_coreset_finish_kernel(const unsigned long long* keys, int64_t* idx, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) idx[i] = cs_key_row(keys[i]);
}
}  // namespace

extern "C" int ld_pc_project(const float* e, int64_t N, int D, const int32_t* rowptr, const int32_t* cols,
                             const float* vals, int k, float* out, int64_t ld, void* stream) {
  LD_REQUIRE(e && rowptr && cols && vals && out, "ld_pc_project: null pointer");
  LD_REQUIRE(N > 0 && (N + PJ_ROWS - 1) / PJ_ROWS < (1L << 31), "ld_pc_project: N %ld", (long)N);
  LD_REQUIRE(D >= 4 && D <= PJ_MAX_D && D % 4 == 0, "ld_pc_project: D %d (a multiple of 4, at most %d)", D, PJ_MAX_D);
  LD_REQUIRE(k > 0, "ld_pc_project: k %d", k);
  LD_REQUIRE(ld >= N && ld % 4 == 0, "ld_pc_project: ld %ld (at least N = %ld, a multiple of 4)", (long)ld, (long)N);
  LD_REQUIRE(((uintptr_t)e & 15) == 0 && ((uintptr_t)out & 15) == 0, "ld_pc_project: E and out must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(pc_project_kernel, dim3((unsigned)((N + PJ_ROWS - 1) / PJ_ROWS)), dim3(PJ_THREADS),
            (size_t)D * PJ_ROWS * sizeof(float), st, e, (long)N, D, rowptr, cols, vals, k, out, (long)ld);
  LD_LAUNCH_CHECK("pc_project");
  return LD_OK;
}

extern "C" int ld_pc_coreset(const float* ft, int64_t ld, int64_t N, int k, int64_t n, int64_t start, float* min_d,
                             unsigned long long* keys, int64_t* idx, void* stream) {
  LD_REQUIRE(ft && min_d && keys && idx, "ld_pc_coreset: null pointer");
  LD_REQUIRE(N > 0 && N < (1L << 31), "ld_pc_coreset: N %ld", (long)N);
  LD_REQUIRE(k > 0 && k <= CS_MAX_K, "ld_pc_coreset: k %d (1..%d)", k, CS_MAX_K);
  LD_REQUIRE(ld >= N && ld % 4 == 0, "ld_pc_coreset: ld %ld (at least N = %ld, a multiple of 4)", (long)ld, (long)N);
  LD_REQUIRE(n > 0 && n <= N, "ld_pc_coreset: n %ld (1..N = %ld)", (long)n, (long)N);
  LD_REQUIRE(start >= 0 && start < N, "ld_pc_coreset: start %ld (0..N-1)", (long)start);
  LD_REQUIRE(((uintptr_t)ft & 15) == 0 && ((uintptr_t)min_d & 15) == 0,
             "ld_pc_coreset: features and min_d must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_HIP(hipMemsetAsync(keys, 0, (size_t)n * sizeof(unsigned long long), st));
  const dim3 grid((unsigned)((N + CS_ROWS - 1) / CS_ROWS));
  const size_t lds = (size_t)k * sizeof(float);
  for (long i = 0; i < n; ++i) {
    LD_LAUNCH(pc_coreset_step_kernel, grid, dim3(CS_THREADS), lds, st, ft, (long)ld, (long)N, k, min_d, keys, i,
              (long)start);
    LD_LAUNCH_CHECK("pc_coreset_step");
  }
  LD_LAUNCH(pc_coreset_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, idx, (long)n);
  LD_LAUNCH_CHECK("pc_coreset_finish");
  return LD_OK;
}
