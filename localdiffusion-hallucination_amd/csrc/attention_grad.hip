// Training the denoiser, third slice: the core of a trainable full Attention (ddpm.py:253-282 + the non-flash path of
// attend.py) -- softmax(q k^T / sqrt(32)) v per (sample, head) -- forward with the row statistics kept, and its backward.
// The two 1x1 convolutions, the RMSNorm in front and their gradients are the launches linattn_grad.py already makes.
//
// fp32 storage, exact fp32 products (fmaf chains on the VALU), the layout of linattn_grad.hip: qkv [B, H, W, ld3] with q at
// channel 0, k at `hidden`, v at 2 * hidden, a head's 32 channels contiguous at head * 32 inside each; the attention output
// and its gradient are [B, H, W, ldo].  q is NOT pre-scaled: the kernels apply 32^-0.5 to the logits.  Nothing of size
// n x n is written to memory in either direction: the forward is an online softmax over tiles of 64 keys that keeps one
// number per row, lse = max + log(normaliser); the backward recomputes p = exp(s - lse) from qkv.
//
// Who owns what (the shape of attention_kernel<float> in attention.hip, three times):
//   * forward, one workgroup per 64 queries of a (sample, head): lane = query (its q row and its 32 outputs in
//     registers), wave w = keys 16 w .. 16 w + 15 of every 64-key tile that goes through LDS (a key's row is a broadcast
//     read).  Every wave keeps its own (m, l, o); the four meet at the end, rescaled to the common maximum, in wave order.
//   * backward, row pass, the same grid: delta = rowsum(dO o) of the lane's query (kept in `work` for the column pass),
//     then per key ds = p (dO . v - delta) and dq += ds k; the four waves' dq meet in wave order; dq carries the 32^-0.5.
//   * backward, column pass, one workgroup per 64 KEYS: lane = key (k, v, dk, dv in registers), wave w = queries
//     16 w .. 16 w + 15 of every 64-query tile of q, dO, lse and delta in LDS; dv += p dO, dk += ds q.
// Two passes cost seven tile products instead of five and buy a fixed order of every sum without a per-tile dq workspace:
// every result is reproducible bit for bit, and there are no atomics.
//
// Masking: rows past n in a tile are staged as zeros and their p is SELECTED to 0 (not exp of a masking constant: see
// ld_attention on what exp(rounding error of a huge negative) x 0 gave).  A wave that never saw a valid key ends with
// m = -1e30 (finite), l = 0, o = 0, and its weight in the merge is exp2(-huge) = 0: it contributes exactly nothing.
// Lanes whose query / key is past n work on row n - 1 and store nothing.  Padded channels of qkv, out and dout are never
// read; those of out and dqkv are written as zeros by extra workgroup columns (blockIdx.y >= heads).
// exp is v_exp_f32 on a * log2(e), the arguments are <= 0 up to rounding (linattn_grad.hip on its error).
#include "common.hip.h"
#include "dn_common.hip.h"
#include "fa_common.hip.h"

namespace {

constexpr int FA_W = 16;              // rows of a tile per wave (lane = row: four waves share a tile of FA_T)

// rows [r0, r0 + 64) of a [n][ld] matrix, 32 channels each, into LDS; zeros past n
__device__ __forceinline__ void fa_stage(float (*dst)[FA_D], const float* __restrict__ src, long r0, long n, int ld, int tid) {
#pragma unroll
  for (int i = tid; i < FA_T * FA_D / 4; i += FA_BS) {
    const int row = i >> 3, c = (i & 7) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + row < n) v = ld4(src + (size_t)(r0 + row) * ld + c);
    *reinterpret_cast<float4*>(&dst[row][c]) = v;
  }
}
// a . LDS row
__device__ __forceinline__ float fa_dot(const float (&a)[FA_D], const float* row) {
  float acc = 0.f;
#pragma unroll
  for (int d = 0; d < FA_D; d += 4) {
    const float4 r = *reinterpret_cast<const float4*>(row + d);          // (broadcast read)
    acc = fmaf(a[d], r.x, acc); acc = fmaf(a[d + 1], r.y, acc); acc = fmaf(a[d + 2], r.z, acc); acc = fmaf(a[d + 3], r.w, acc);
  }
  return acc;
}
// a += w x LDS row
__device__ __forceinline__ void fa_axpy(float (&a)[FA_D], float w, const float* row) {
#pragma unroll
  for (int d = 0; d < FA_D; d += 4) {
    const float4 r = *reinterpret_cast<const float4*>(row + d);
    a[d] = fmaf(w, r.x, a[d]); a[d + 1] = fmaf(w, r.y, a[d + 1]); a[d + 2] = fmaf(w, r.z, a[d + 2]); a[d + 3] = fmaf(w, r.w, a[d + 3]);
  }
}
__device__ __forceinline__ void fa_load_row(float (&a)[FA_D], const float* __restrict__ src) {
#pragma unroll
  for (int d = 0; d < FA_D; d += 4) {
    const float4 r = ld4(src + d);
    a[d] = r.x; a[d + 1] = r.y; a[d + 2] = r.z; a[d + 3] = r.w;
  }
}
// The four waves' 32 sums per lane meet in wave order: s_o [wave][d][lane]; this thread gets channels 8 wv .. 8 wv + 7 of
// its lane's row, times `scale`.
__device__ __forceinline__ void fa_meet(float (*s_o)[FA_D][FA_T], const float (&a)[FA_D], int wv, int lane, float scale,
                                        float (&r)[8]) {
#pragma unroll
  for (int d = 0; d < FA_D; ++d) s_o[wv][d][lane] = a[d];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int d = 8 * wv + i;
    r[i] = (((s_o[0][d][lane] + s_o[1][d][lane]) + s_o[2][d][lane]) + s_o[3][d][lane]) * scale;
  }
}

// ================================================================================================ forward
__global__ __launch_bounds__(FA_BS) void fa_forward_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                           float* __restrict__ lse, long n, int heads, int ld3, int ldo) {
  __shared__ __attribute__((aligned(16))) float s_k[FA_T][FA_D];
  __shared__ __attribute__((aligned(16))) float s_v[FA_T][FA_D];
  __shared__ float s_m[4][FA_T], s_l[4][FA_T];
  __shared__ float s_o[4][FA_D][FA_T];                    // [wave][d][query]: conflict-free
  const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, hidden = heads * FA_D;
  const long q0 = (long)blockIdx.x * FA_T;
  float* orow = out + (size_t)b * n * ldo;
  if (h >= heads) {
    fa_zero_cols(orow, q0, n, ldo, h * FA_D, tid);
    return;
  }
  const float* base = qkv + (size_t)b * n * ld3 + h * FA_D;
  const long qi = q0 + lane < n ? q0 + lane : n - 1;
  float q[FA_D], o[FA_D];
  fa_load_row(q, base + (size_t)qi * ld3);
#pragma unroll
  for (int d = 0; d < FA_D; ++d) o[d] = 0.f;
  float m = FA_NEG, l = 0.f;
  for (long j0 = 0; j0 < n; j0 += FA_T) {
    __syncthreads();
    fa_stage(s_k, base + hidden, j0, n, ld3, tid);
    fa_stage(s_v, base + 2 * hidden, j0, n, ld3, tid);
    __syncthreads();
    float s[FA_W];
    float tmax = FA_NEG;
#pragma unroll
    for (int kk = 0; kk < FA_W; ++kk) {
      const int key = wv * FA_W + kk;
      const float a = fa_dot(q, s_k[key]) * FA_SCALE;
      s[kk] = j0 + key < n ? a : FA_NEG;
      tmax = fmaxf(tmax, s[kk]);
    }
    const float mn = fmaxf(m, tmax);
    const float alpha = fa_exp(m - mn);                  // (both -1e30 while the wave has seen no valid key: 1, on l = o = 0)
    l *= alpha;
#pragma unroll
    for (int d = 0; d < FA_D; ++d) o[d] *= alpha;
    m = mn;
#pragma unroll
    for (int kk = 0; kk < FA_W; ++kk) {
      const int key = wv * FA_W + kk;
      const float p = j0 + key < n ? fa_exp(s[kk] - m) : 0.f;
      l += p;
      fa_axpy(o, p, s_v[key]);
    }
  }
  s_m[wv][lane] = m;
  s_l[wv][lane] = l;
#pragma unroll
  for (int d = 0; d < FA_D; ++d) s_o[wv][d][lane] = o[d];
  __syncthreads();
  const float M = fmaxf(fmaxf(s_m[0][lane], s_m[1][lane]), fmaxf(s_m[2][lane], s_m[3][lane]));
  float f[4], L = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    f[w] = fa_exp(s_m[w][lane] - M);                     // (a wave without a valid key: exp2(-huge) = 0, on l = o = 0)
    L += s_l[w][lane] * f[w];
  }
  if (q0 + lane >= n) return;
  const float inv = 1.0f / L;                            // (L >= 1: the wave that holds the maximum has f = 1 and l >= 1)
  float r[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int d = 8 * wv + i;
    r[i] = (((s_o[0][d][lane] * f[0] + s_o[1][d][lane] * f[1]) + s_o[2][d][lane] * f[2]) + s_o[3][d][lane] * f[3]) * inv;
  }
  float* dst = orow + (size_t)(q0 + lane) * ldo + h * FA_D + 8 * wv;
  st4(dst, r[0], r[1], r[2], r[3]);
  st4(dst + 4, r[4], r[5], r[6], r[7]);
  if (lse && wv == 0) lse[((size_t)b * heads + h) * n + q0 + lane] = M + logf(L);
}

// ================================================================================================ backward: rows (dq)
__global__ __launch_bounds__(FA_BS) void fa_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                      const float* __restrict__ dout, const float* __restrict__ lse,
                                                      float* __restrict__ delta, float* __restrict__ dqkv, long n, int heads,
                                                      int ld3, int ldo) {
  __shared__ __attribute__((aligned(16))) float s_k[FA_T][FA_D];
  __shared__ __attribute__((aligned(16))) float s_v[FA_T][FA_D];
  __shared__ float s_o[4][FA_D][FA_T];
  const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, hidden = heads * FA_D;
  const long q0 = (long)blockIdx.x * FA_T;
  float* drow = dqkv + (size_t)b * n * ld3;
  if (h >= heads) {
    fa_zero_cols(drow, q0, n, ld3, 3 * hidden + (h - heads) * FA_D, tid);
    return;
  }
  const float* base = qkv + (size_t)b * n * ld3 + h * FA_D;
  const long qi = q0 + lane < n ? q0 + lane : n - 1;
  const size_t stat = ((size_t)b * heads + h) * n + qi;
  float q[FA_D], g[FA_D], dq[FA_D];
  fa_load_row(q, base + (size_t)qi * ld3);
  fa_load_row(g, dout + ((size_t)b * n + qi) * ldo + h * FA_D);
  float dl = 0.f;
  {
    const float* op = out + ((size_t)b * n + qi) * ldo + h * FA_D;
#pragma unroll
    for (int d = 0; d < FA_D; d += 4) {
      const float4 r = ld4(op + d);
      dl = fmaf(g[d], r.x, dl); dl = fmaf(g[d + 1], r.y, dl); dl = fmaf(g[d + 2], r.z, dl); dl = fmaf(g[d + 3], r.w, dl);
    }
  }
  if (wv == 0 && q0 + lane < n) delta[stat] = dl;        // (every wave holds the same bits)
  const float ls = lse[stat];
#pragma unroll
  for (int d = 0; d < FA_D; ++d) dq[d] = 0.f;
  for (long j0 = 0; j0 < n; j0 += FA_T) {
    __syncthreads();
    fa_stage(s_k, base + hidden, j0, n, ld3, tid);
    fa_stage(s_v, base + 2 * hidden, j0, n, ld3, tid);
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < FA_W; ++kk) {
      const int key = wv * FA_W + kk;
      const float a = fa_dot(q, s_k[key]) * FA_SCALE, dp = fa_dot(g, s_v[key]);
      const float p = j0 + key < n ? fa_exp(a - ls) : 0.f;
      fa_axpy(dq, p * (dp - dl), s_k[key]);
    }
  }
  float r[8];
  fa_meet(s_o, dq, wv, lane, FA_SCALE, r);
  if (q0 + lane >= n) return;
  float* dst = drow + (size_t)(q0 + lane) * ld3 + h * FA_D + 8 * wv;
  st4(dst, r[0], r[1], r[2], r[3]);
  st4(dst + 4, r[4], r[5], r[6], r[7]);
}

// ================================================================================================ backward: columns (dk, dv)
__global__ __launch_bounds__(FA_BS) void fa_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                       const float* __restrict__ lse, const float* __restrict__ delta,
                                                       float* __restrict__ dqkv, long n, int heads, int ld3, int ldo) {
  __shared__ __attribute__((aligned(16))) float s_q[FA_T][FA_D];
  __shared__ __attribute__((aligned(16))) float s_g[FA_T][FA_D];
  __shared__ float s_ls[FA_T], s_dl[FA_T];
  __shared__ float s_o[4][FA_D][FA_T];
  const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, hidden = heads * FA_D;
  const long k0 = (long)blockIdx.x * FA_T;
  const float* base = qkv + (size_t)b * n * ld3 + h * FA_D;
  const float* gbase = dout + (size_t)b * n * ldo + h * FA_D;
  const size_t stat = ((size_t)b * heads + h) * n;
  const long ki = k0 + lane < n ? k0 + lane : n - 1;
  float k[FA_D], v[FA_D], dk[FA_D], dv[FA_D];
  fa_load_row(k, base + hidden + (size_t)ki * ld3);
  fa_load_row(v, base + 2 * hidden + (size_t)ki * ld3);
#pragma unroll
  for (int d = 0; d < FA_D; ++d) dk[d] = dv[d] = 0.f;
  for (long i0 = 0; i0 < n; i0 += FA_T) {
    __syncthreads();
    fa_stage(s_q, base, i0, n, ld3, tid);
    fa_stage(s_g, gbase, i0, n, ldo, tid);
    if (tid < FA_T) {
      const bool ok = i0 + tid < n;
      s_ls[tid] = ok ? lse[stat + i0 + tid] : 0.f;
      s_dl[tid] = ok ? delta[stat + i0 + tid] : 0.f;
    }
    __syncthreads();
#pragma unroll 1                                            // (222 registers, two waves per SIMD; unrolled by 2 or 4: 256 and one)
    for (int qq = 0; qq < FA_W; ++qq) {
      const int i = wv * FA_W + qq;
      const float a = fa_dot(k, s_q[i]) * FA_SCALE, dp = fa_dot(v, s_g[i]);   // (k . q in the forward's order: the same bits)
      const float p = i0 + i < n ? fa_exp(a - s_ls[i]) : 0.f;
      fa_axpy(dv, p, s_g[i]);
      fa_axpy(dk, p * (dp - s_dl[i]), s_q[i]);
    }
  }
  const bool live = k0 + lane < n;
  float* dst = dqkv + ((size_t)b * n + (live ? k0 + lane : 0)) * ld3 + h * FA_D + 8 * wv;
  float r[8];
  fa_meet(s_o, dk, wv, lane, FA_SCALE, r);
  if (live) {
    st4(dst + hidden, r[0], r[1], r[2], r[3]);
    st4(dst + hidden + 4, r[4], r[5], r[6], r[7]);
  }
  __syncthreads();
  fa_meet(s_o, dv, wv, lane, 1.0f, r);
  if (live) {
    st4(dst + 2 * hidden, r[0], r[1], r[2], r[3]);
    st4(dst + 2 * hidden + 4, r[4], r[5], r[6], r[7]);
  }
}

// ================================================================================================ host side
}  // namespace

extern "C" int64_t ld_dn_fa_work_bytes(int B, int heads, int H, int W) {
  if (!fa_shape_ok(B, H, W, heads)) return 0;
  return ((int64_t)B * heads * H * W * (int64_t)sizeof(float) + 7) / 8 * 8;          // delta [B, heads, n]
}

extern "C" int ld_dn_fa_forward(const float* qkv, float* out, float* lse, int B, int H, int W, int heads, int ld3, int ldo,
                                void* stream) {
  LD_REQUIRE(fa_shape_ok(B, H, W, heads) && fa_strides_ok(heads, ld3, ldo),
             "ld_dn_fa_forward: B=%d H=%d W=%d heads=%d ld3=%d ldo=%d (heads >= 1, ld3 >= 96 heads, ldo >= 32 heads, multiples of 4)",
             B, H, W, heads, ld3, ldo);
  LD_REQUIRE(qkv && out, "ld_dn_fa_forward: null pointer");
  LD_REQUIRE(dn_aligned16(qkv) && dn_aligned16(out) && (reinterpret_cast<uintptr_t>(lse) & 3) == 0,
             "ld_dn_fa_forward: a pointer is not aligned (qkv, out: 16 bytes)");
  const int slots = fa_slots(heads, ldo, heads * FA_D);
  LD_REQUIRE(slots <= 65535, "ld_dn_fa_forward: ldo %d", ldo);
  const long n = (long)H * W;
  LD_LAUNCH(fa_forward_kernel, dim3((unsigned)((n + FA_T - 1) / FA_T), (unsigned)slots, (unsigned)B), dim3(FA_BS), 0,
            dn_st(stream), qkv, out, lse, n, heads, ld3, ldo);
  LD_LAUNCH_CHECK("dn_fa_forward");
  return LD_OK;
}

extern "C" int ld_dn_fa_backward(const float* qkv, const float* out, const float* dout, const float* lse, void* work, float* dqkv,
                                 int B, int H, int W, int heads, int ld3, int ldo, void* stream) {
  LD_REQUIRE(fa_shape_ok(B, H, W, heads) && fa_strides_ok(heads, ld3, ldo),
             "ld_dn_fa_backward: B=%d H=%d W=%d heads=%d ld3=%d ldo=%d (heads >= 1, ld3 >= 96 heads, ldo >= 32 heads, multiples of "
             "4)", B, H, W, heads, ld3, ldo);
  LD_REQUIRE(qkv && out && dout && lse && work && dqkv, "ld_dn_fa_backward: null pointer");
  LD_REQUIRE(dn_aligned16(qkv) && dn_aligned16(out) && dn_aligned16(dout) && dn_aligned16(dqkv) &&
                 (reinterpret_cast<uintptr_t>(lse) & 3) == 0 && (reinterpret_cast<uintptr_t>(work) & 3) == 0,
             "ld_dn_fa_backward: a pointer is not aligned (qkv, out, dout, dqkv: 16 bytes)");
  const int slots = fa_slots(heads, ld3, 3 * heads * FA_D);
  LD_REQUIRE(slots <= 65535, "ld_dn_fa_backward: ld3 %d", ld3);
  const long n = (long)H * W;
  const unsigned tiles = (unsigned)((n + FA_T - 1) / FA_T);
  hipStream_t st = dn_st(stream);
  float* delta = static_cast<float*>(work);
  LD_LAUNCH(fa_dq_kernel, dim3(tiles, (unsigned)slots, (unsigned)B), dim3(FA_BS), 0, st, qkv, out, dout, lse, delta, dqkv, n, heads,
            ld3, ldo);
  LD_LAUNCH(fa_dkv_kernel, dim3(tiles, (unsigned)heads, (unsigned)B), dim3(FA_BS), 0, st, qkv, dout, lse, (const float*)delta, dqkv,
            n, heads, ld3, ldo);
  LD_LAUNCH_CHECK("dn_fa_backward");
  return LD_OK;
}
