// Training the denoiser, sixth slice: what a trainable Unet (ddpm.py:286-451) needs besides its blocks -- the time MLP in
// training form (sinusoidal embedding -> Linear -> GELU -> Linear, ddpm.py:136-149 and :339-344, keeping the embedding and the
// pre-GELU value for its backward), that backward, and the glue of Unet.forward in the padded NHWC layout: torch.cat of two
// activations and attn(x) + x, as one copy kernel.
//
// fp32 data.  The time MLP's sums are fp64 and run in a fixed order: over the input features, a lane's features in index
// order and then the 64 lanes of a wave by the shuffle tree; over the batch in index order, one thread per output element.
// No atomics, nothing allocates, every entry point checks its arguments before it launches.
#include "common.hip.h"
#include "dn_common.hip.h"

namespace {

constexpr int TM_BS = 256;

__device__ __forceinline__ double tm_wave_sum(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// nn.GELU() (approximate='none'): x Phi(x), and its derivative Phi(x) + x phi(x)
__device__ __forceinline__ float tm_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float tm_gelu_grad(float x) {
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
  return cdf + x * pdf;
}

// ---------------------------------------------------------------- the time MLP, forward: one workgroup per sample
// A wave owns output features wave, wave + 4, ..: its lanes stride over the input features (coalesced rows of the weight).
__global__ __launch_bounds__(TM_BS) void tm_forward_kernel(const float* __restrict__ times, const float* __restrict__ freqs,
                                                           const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ w3, const float* __restrict__ b3,
                                                           float* __restrict__ emb, float* __restrict__ h1,
                                                           float* __restrict__ temb, int dim, int T) {
  extern __shared__ float tm_sh[];                   // e [dim] | act [T]
  float* e = tm_sh;
  float* act = tm_sh + dim;
  const int b = blockIdx.x, tid = threadIdx.x, half = dim / 2;
  const int wave = tid >> 6, lane = tid & 63;
  const float t = times[b];
  for (int k = tid; k < half; k += TM_BS) {
    const float ang = t * freqs[k];
    const float s = sinf(ang), c = cosf(ang);
    e[k] = s;
    e[half + k] = c;
    emb[(size_t)b * dim + k] = s;
    emb[(size_t)b * dim + half + k] = c;
  }
  __syncthreads();
  for (int o = wave; o < T; o += TM_BS / 64) {
    double acc = 0.0;
    for (int k = lane; k < dim; k += 64) acc = fma((double)w1[(size_t)o * dim + k], (double)e[k], acc);
    acc = tm_wave_sum(acc);
    const float h = (float)(acc + (double)b1[o]);
    if (lane == 0) {
      h1[(size_t)b * T + o] = h;
      act[o] = tm_gelu(h);
    }
  }
  __syncthreads();
  for (int o = wave; o < T; o += TM_BS / 64) {
    double acc = 0.0;
    for (int k = lane; k < T; k += 64) acc = fma((double)w3[(size_t)o * T + k], (double)act[k], acc);
    acc = tm_wave_sum(acc);
    if (lane == 0) temb[(size_t)b * T + o] = (float)(acc + (double)b3[o]);
  }
}

// ---------------------------------------------------------------- the time MLP, backward
// pass 1, an element (b, k) per thread: act [B][T] = gelu(h1) and dh1 [B][T] = (sum_j dtemb[b][j] w3[j][k]) gelu'(h1[b][k])
__global__ __launch_bounds__(TM_BS) void tm_bwd_hidden_kernel(const float* __restrict__ dtemb, const float* __restrict__ h1,
                                                              const float* __restrict__ w3, float* __restrict__ act,
                                                              float* __restrict__ dh1, long n, int T) {
  const long i = (long)blockIdx.x * TM_BS + threadIdx.x;
  if (i >= n) return;
  const long b = i / T;
  const int k = (int)(i - b * T);
  double acc = 0.0;
#pragma unroll 8                                    // (eight independent loads in flight; the additions keep their order)
  for (int j = 0; j < T; ++j) acc = fma((double)dtemb[(size_t)b * T + j], (double)w3[(size_t)j * T + k], acc);
  const float h = h1[i];
  act[i] = tm_gelu(h);
  dh1[i] = (float)acc * tm_gelu_grad(h);
}
// pass 2, an output element per thread, the batch added in index order: four kinds of workgroups -- dw3 [T][T] = dtemb^T
// act, dw1 [T][dim] = dh1^T emb, db3 [T] = sum_b dtemb, db1 [T] = sum_b dh1
__global__ __launch_bounds__(TM_BS) void tm_bwd_params_kernel(const float* __restrict__ dtemb, const float* __restrict__ emb,
                                                              const float* __restrict__ act, const float* __restrict__ dh1,
                                                              float* __restrict__ dw1, float* __restrict__ db1,
                                                              float* __restrict__ dw3, float* __restrict__ db3, int B, int dim,
                                                              int T, int wg_w3, int wg_w1, int wg_b) {
  int wg = blockIdx.x;
  const float *rows, *cols;                          // out[j][k] = sum_b rows[b][j] cols[b][k], cols nc wide
  float* out;
  int nc;
  long n;
  if (wg < wg_w3) {
    rows = dtemb; cols = act; out = dw3; nc = T; n = (long)T * T;
  } else if ((wg -= wg_w3) < wg_w1) {
    rows = dh1; cols = emb; out = dw1; nc = dim; n = (long)T * dim;
  } else {
    wg -= wg_w1;
    const float* src = wg < wg_b ? dtemb : dh1;
    float* dst = wg < wg_b ? db3 : db1;
    if (wg >= wg_b) wg -= wg_b;
    const int j = wg * TM_BS + (int)threadIdx.x;
    if (j >= T) return;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) acc += (double)src[(size_t)b * T + j];
    dst[j] = (float)acc;
    return;
  }
  const long i = (long)wg * TM_BS + threadIdx.x;
  if (i >= n) return;
  const int j = (int)(i / nc), k = (int)(i - (long)j * nc);
  double acc = 0.0;
  for (int b = 0; b < B; ++b) acc = fma((double)rows[(size_t)b * T + j], (double)cols[(size_t)b * nc + k], acc);
  out[i] = (float)acc;
}

// ---------------------------------------------------------------- the glue: out[..., :ca] = a (+ a2), out[..., ca:ca+cb] = b
// A 16-byte lane of the output per thread; ca and cb are multiples of 4, so a lane lies in one of the three parts.
__global__ __launch_bounds__(256) void dn_join_kernel(const float* __restrict__ a, const float* __restrict__ a2,
                                                      const float* __restrict__ b, float* __restrict__ out, long n, int ca,
                                                      int lda, int cb, int ldb, int ldo) {
  const int Q = ldo / 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long p = i / Q;
    const int c0 = 4 * (int)(i - p * Q);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 < ca) {
      v = ld4(a + (size_t)p * lda + c0);
      if (a2) {
        const float4 w = ld4(a2 + (size_t)p * lda + c0);
        v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
      }
    } else if (c0 < ca + cb) {
      v = ld4(b + (size_t)p * ldb + (c0 - ca));
    }
    st4(out + (size_t)p * ldo + c0, v.x, v.y, v.z, v.w);
  }
}

inline bool tm_shape_ok(int B, int dim, int T) {
  return B > 0 && dim >= 4 && dim % 2 == 0 && T > 0 && T % 4 == 0 && (long)dim + T <= 12288 &&     // (48 KB of LDS)
         (long)T * T < (1L << 31) && (long)T * dim < (1L << 31) && (long)B * (T > dim ? T : dim) < (1L << 40);
}
}  // namespace

extern "C" int ld_dn_time_mlp_forward(const float* times, const float* freqs, const float* w1, const float* b1, const float* w3,
                                      const float* b3, float* emb, float* h1, float* temb, int B, int dim, int T, void* stream) {
  LD_REQUIRE(tm_shape_ok(B, dim, T), "ld_dn_time_mlp_forward: B=%d dim=%d T=%d (dim even and >= 4, T a multiple of 4, dim + T <= "
             "12288)", B, dim, T);
  LD_REQUIRE(times && freqs && w1 && b1 && w3 && b3 && emb && h1 && temb, "ld_dn_time_mlp_forward: null pointer");
  LD_REQUIRE(((uintptr_t)times | (uintptr_t)freqs | (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w3 | (uintptr_t)b3 |
              (uintptr_t)emb | (uintptr_t)h1 | (uintptr_t)temb) % 4 == 0, "ld_dn_time_mlp_forward: a pointer is not 4-byte aligned");
  LD_LAUNCH(tm_forward_kernel, dim3((unsigned)B), dim3(TM_BS), ((size_t)dim + T) * sizeof(float), dn_st(stream), times, freqs, w1,
            b1, w3, b3, emb, h1, temb, dim, T);
  LD_LAUNCH_CHECK("dn_time_mlp_forward");
  return LD_OK;
}

extern "C" int64_t ld_dn_time_mlp_work_bytes(int B, int dim, int T) {
  if (!tm_shape_ok(B, dim, T)) return 0;
  return 2 * (int64_t)B * T * (int64_t)sizeof(float);
}

extern "C" int ld_dn_time_mlp_backward(const float* dtemb, const float* emb, const float* h1, const float* w3, float* work,
                                       float* dw1, float* db1, float* dw3, float* db3, int B, int dim, int T, void* stream) {
  LD_REQUIRE(tm_shape_ok(B, dim, T), "ld_dn_time_mlp_backward: B=%d dim=%d T=%d (dim even and >= 4, T a multiple of 4, dim + T <= "
             "12288)", B, dim, T);
  LD_REQUIRE(dtemb && emb && h1 && w3 && work && dw1 && db1 && dw3 && db3, "ld_dn_time_mlp_backward: null pointer");
  LD_REQUIRE(((uintptr_t)dtemb | (uintptr_t)emb | (uintptr_t)h1 | (uintptr_t)w3 | (uintptr_t)work | (uintptr_t)dw1 |
              (uintptr_t)db1 | (uintptr_t)dw3 | (uintptr_t)db3) % 4 == 0, "ld_dn_time_mlp_backward: a pointer is not 4-byte aligned");
  const long n = (long)B * T;
  float* act = work;
  float* dh1 = work + n;
  hipStream_t st = dn_st(stream);
  LD_LAUNCH(tm_bwd_hidden_kernel, dim3((unsigned)((n + TM_BS - 1) / TM_BS)), dim3(TM_BS), 0, st, dtemb, h1, w3, act, dh1, n, T);
  const long wg_w3 = ((long)T * T + TM_BS - 1) / TM_BS, wg_w1 = ((long)T * dim + TM_BS - 1) / TM_BS, wg_b = (T + TM_BS - 1) / TM_BS;
  LD_REQUIRE(wg_w3 + wg_w1 + 2 * wg_b < (1L << 31), "ld_dn_time_mlp_backward: %d x %d weights", T, T);
  LD_LAUNCH(tm_bwd_params_kernel, dim3((unsigned)(wg_w3 + wg_w1 + 2 * wg_b)), dim3(TM_BS), 0, st, dtemb, emb, (const float*)act,
            (const float*)dh1, dw1, db1, dw3, db3, B, dim, T, (int)wg_w3, (int)wg_w1, (int)wg_b);
  LD_LAUNCH_CHECK("dn_time_mlp_backward");
  return LD_OK;
}

extern "C" int ld_dn_join(const float* a, const float* a2, const float* b, float* out, int B, int H, int W, int ca, int lda,
                          int cb, int ldb, int ldo, void* stream) {
  LD_REQUIRE(B > 0 && H > 0 && W > 0, "ld_dn_join: shape B=%d H=%d W=%d", B, H, W);
  LD_REQUIRE(ca > 0 && ca % 32 == 0 && cb >= 0 && cb % 32 == 0 && lda >= ca && lda % 4 == 0 && ldo % 4 == 0 &&
                 (long)ca + cb <= ldo && ldo <= (1 << 20) && lda <= (1 << 20),
             "ld_dn_join: ca=%d lda=%d cb=%d ldo=%d (ca, cb multiples of 32, strides multiples of 4, lda >= ca, ldo >= ca + cb)", ca,
             lda, cb, ldo);
  LD_REQUIRE((b != nullptr) == (cb > 0), "ld_dn_join: b and cb go together");
  LD_REQUIRE(!b || (ldb >= cb && ldb % 4 == 0 && ldb <= (1 << 20)), "ld_dn_join: cb=%d ldb=%d (ldb >= cb a multiple of 4)", cb, ldb);
  LD_REQUIRE(a && out, "ld_dn_join: null pointer");
  LD_REQUIRE(a2 || b, "ld_dn_join: neither a2 nor b: nothing to join");
  LD_REQUIRE(dn_aligned16(a) && dn_aligned16(a2) && dn_aligned16(b) && dn_aligned16(out), "ld_dn_join: a pointer is not 16-byte aligned");
  LD_REQUIRE(out != a && out != a2 && out != b, "ld_dn_join: out is one of the inputs");
  const long px = (long)B * H * W;
  LD_REQUIRE(px <= (1L << 40) / ldo && px <= (1L << 40) / lda && (!b || px <= (1L << 40) / ldb), "ld_dn_join: %ld pixels of %d floats",
             px, ldo);
  const long n = px * (ldo / 4);
  long wgs = (n + 255) / 256;
  if (wgs > 8192) wgs = 8192;
  LD_LAUNCH(dn_join_kernel, dim3((unsigned)wgs), dim3(256), 0, dn_st(stream), a, a2, b, out, n, ca, lda, cb, ldb, ldo);
  LD_LAUNCH_CHECK("dn_join");
  return LD_OK;
}
