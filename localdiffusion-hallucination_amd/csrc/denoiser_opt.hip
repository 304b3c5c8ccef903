// Training the denoiser, seventh slice: the optimiser step of the reference's Trainer.train (ddpm.py:1558-1571) over every
// parameter tensor of the Unet in two launches -- clip_grad_norm_'s total norm, then the clipped Adam update, the zeroing of
// the gradients and the EMA update in one pass.
//
// The tensors are described by a table in device memory (ld_dn_opt_tensor: 264 or 334 entries do not fit in kernel
// arguments) that ld_dn_opt_layout fills on the host: every tensor owns a 16-byte aligned segment of the flat grad / exp_avg /
// exp_avg_sq / ema buffers and a run of workgroups of LD_DN_OPT_CHUNK elements each, so no workgroup straddles two tensors;
// a workgroup finds its tensor by bisection of the first_wg column.  A thread owns up to four 16-byte lanes of its chunk;
// the last lanes of a tensor whose count is no multiple of 4 are walked element by element.
//
// fp32 storage.  The sum of squares is fp64: a thread adds its elements in index order, a wave by the shuffle tree, the four
// waves in order, one partial per workgroup, and a second launch of one workgroup adds the partials the same way (thread t
// takes partials t, t + 256, .. in index order, then the tree and the waves): an order that depends on the sizes alone.  No
// atomics, nothing allocates, the norm never leaves the device: the step reads it from memory.  Adam's arithmetic is
// ld_adam_update (adam.hip.h, shared with ld_seg_adam), applied to g * coef.
//
// Data-parallel training puts ld_dn_opt_reduce in the place of ld_dn_opt_sqnorm: the ranks all-gather their flat gradients,
// and one launch adds the copies in rank order (plain fp32, left to right) while it gathers the norm's partials, so every
// rank steps on the same bits and a W-rank step equals a one-rank step that accumulated the W shards in order.
//
// Loss scaling (amp = "fp16"): the gradients arrive multiplied by a scale that lives in device memory (ld_dn_scaler_state).
// Between the norm and the step a one-thread kernel, ld_dn_opt_scaler_update, takes torch.amp.GradScaler's decisions from
// the squared norm alone -- a non-finite norm skips the step and backs the scale off, growth_interval finite ones in a row
// grow it -- and leaves what the step needs (found_inf, 1 / scale, Adam's two bias corrections for its OWN step count,
// which does not advance on a skip) in the state; ld_dn_opt_step_scaled is the step above reading them there.  The host
// never sees any of it, so a step still does not wait for the GPU.
#include "common.hip.h"
#include "adam.hip.h"
#include "dn_common.hip.h"

namespace {

constexpr int OPT_BS = 256;
constexpr int OPT_LANES = LD_DN_OPT_CHUNK / (4 * OPT_BS);          // 16-byte lanes per thread
static_assert(LD_DN_OPT_CHUNK % (4 * OPT_BS) == 0, "a chunk is whole 16-byte lanes for every thread");

// The chunk [lo, hi) of tensor e that workgroup wg owns; false when the table does not give it one inside the flat buffers.
struct OptChunk {
  ld_dn_opt_tensor e;
  long lo, hi;
};
__device__ __forceinline__ bool opt_chunk(const ld_dn_opt_tensor* __restrict__ tab, int n, long flat, OptChunk& c) {
  const int wg = (int)blockIdx.x;
  int a = 0, b = n;                                   // the last entry whose first_wg <= wg
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if (tab[mid].first_wg <= wg) a = mid; else b = mid;
  }
  c.e = tab[a];
  const long k = (long)wg - c.e.first_wg;
  if (k < 0 || c.e.count <= 0 || c.e.offset < 0 || (c.e.offset & 3) || c.e.offset > flat || c.e.count > flat - c.e.offset)
    return false;
  c.lo = k * LD_DN_OPT_CHUNK;
  c.hi = c.lo + LD_DN_OPT_CHUNK < c.e.count ? c.lo + LD_DN_OPT_CHUNK : c.e.count;
  return c.lo < c.hi;
}

// the workgroup's sum in a fixed order: the shuffle tree of each wave, then the waves in index order; thread 0 has it
__device__ __forceinline__ double opt_block_sum(double v, double* red) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < OPT_BS / 64; ++w) s += red[w];
  return s;
}

// ---------------------------------------------------------------- the squared norm: one fp64 partial per workgroup
__global__ __launch_bounds__(OPT_BS) void opt_sqnorm_kernel(const ld_dn_opt_tensor* __restrict__ tab, int n,
                                                            const float* __restrict__ grad, long flat,
                                                            double* __restrict__ partial) {
  __shared__ double red[OPT_BS / 64];
  OptChunk c;
  double acc = 0.0;
  if (opt_chunk(tab, n, flat, c) && (c.e.flags & LD_DN_OPT_ADAM)) {
    const float* g = grad + c.e.offset;
#pragma unroll
    for (int k = 0; k < OPT_LANES; ++k) {
      const long i = c.lo + 4L * (k * OPT_BS + (int)threadIdx.x);
      if (i + 4 <= c.hi) {
        const float4 q = ld4(g + i);
        acc += (double)q.x * (double)q.x;
        acc += (double)q.y * (double)q.y;
        acc += (double)q.z * (double)q.z;
        acc += (double)q.w * (double)q.w;
      } else {
        for (long j = i; j < c.hi; ++j) acc += (double)g[j] * (double)g[j];
      }
    }
  }
  const double s = opt_block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(OPT_BS) void opt_sqnorm_final_kernel(const double* __restrict__ partial, int n_wg,
                                                                  double* __restrict__ sumsq) {
  __shared__ double red[OPT_BS / 64];
  double acc = 0.0;
  for (int i = (int)threadIdx.x; i < n_wg; i += OPT_BS) acc += partial[i];
  const double s = opt_block_sum(acc, red);
  if (threadIdx.x == 0) *sumsq = s;
}

// ---------------------------------------------------------------- the step
struct OptScalars {
  float omb1, beta2, omb2, eps, step_size, bc2_sqrt, ema_w;
  int ema_mode;
};

// torch.optim.Adam on g * coef (ld_seg_adam's arithmetic): p, m, v are updated in place
__device__ __forceinline__ void opt_adam(float& p, float g, float& m, float& v, float coef, const OptScalars& s) {
  g = g * coef;                                                   // clip_grad_norm_: g.mul_(clip_coef_clamped)
  ld_adam_update(p, g, m, v, s.omb1, s.beta2, s.omb2, s.eps, s.step_size, s.bc2_sqrt);
}
// ema.lerp_(p, w) as ATen evaluates it: e + w (p - e) below w = 0.5, p - (p - e)(1 - w) from there on (w = 1 gives p)
__device__ __forceinline__ float opt_lerp(float e, float p, float w) {
  const float d = p - e;
  return w < 0.5f ? e + w * d : p - d * (1.0f - w);
}

__device__ __forceinline__ void opt_store4(float* p, const float4& q) { *reinterpret_cast<float4*>(p) = q; }

// The step of one workgroup.  SCALED (ld_dn_opt_step_scaled): the gradients carry the loss scale -- the norm and every
// gradient are multiplied by inv_scale first (torch unscales in place, then clips: (g * inv_scale) * coef, two multiplies in
// this order; with a power-of-two scale both are exact and the order could not matter) -- and on `skip` (the scaler found a
// non-finite gradient) parameters and moments keep their bits while the gradient is still zeroed and the EMA still acts.
// One body, two kernels: opt_step_kernel<> is the fp32 step with the argument list it always had; opt_step_kernel<const
// ld_dn_scaler_state*> takes the state behind it and reads found_inf, inv_scale and Adam's two bias corrections there.
template <typename... State>
__global__ __launch_bounds__(OPT_BS) void opt_step_kernel(const ld_dn_opt_tensor* __restrict__ tab, int n, float* grad, float* m,
                                                          float* v, float* ema, long flat, const double* __restrict__ sumsq,
                                                          double max_norm, OptScalars s, State... state) {
  constexpr bool SCALED = sizeof...(State) != 0;
  float inv_scale = 1.0f;
  bool skip = false;
  if constexpr (SCALED) {
    const ld_dn_scaler_state* st = (state, ...);
    s.step_size = st->step_size;
    s.bc2_sqrt = st->bc2_sqrt;
    inv_scale = st->inv_scale;
    skip = st->found_inf != 0;
  }
  OptChunk c;
  if (!opt_chunk(tab, n, flat, c)) return;
  const bool adam = (c.e.flags & LD_DN_OPT_ADAM) != 0;
  if (!adam && s.ema_mode == 0) return;
  // clip_grad_norm_'s coefficient; a NaN norm stays NaN (c > 1 is false for it), an infinite one gives 0
  double norm = sqrt(*sumsq);
  if constexpr (SCALED) norm *= (double)inv_scale;
  const double cd = max_norm / (norm + 1e-6);
  const float coef = (float)(cd > 1.0 ? 1.0 : cd);
  auto unscaled = [&](float g) {                                    // grad.mul_(inv_scale): GradScaler.unscale_
    if constexpr (SCALED) return g * inv_scale;
    else return g;
  };
  float* P = c.e.param;
  float* G = grad + c.e.offset;
  float* M = m + c.e.offset;
  float* V = v + c.e.offset;
  float* E = ema + c.e.offset;
  const bool vec = (reinterpret_cast<uintptr_t>(P) & 15) == 0;     // (the flat segments are 16-byte aligned by construction)
#pragma unroll
  for (int k = 0; k < OPT_LANES; ++k) {
    const long i = c.lo + 4L * (k * OPT_BS + (int)threadIdx.x);
    if (i >= c.hi) continue;
    if (vec && i + 4 <= c.hi) {
      float4 p = ld4(P + i);
      if (adam) {
        if (!SCALED || !skip) {
          const float4 g = ld4(G + i);
          float4 mm = ld4(M + i), vv = ld4(V + i);
          opt_adam(p.x, unscaled(g.x), mm.x, vv.x, coef, s);
          opt_adam(p.y, unscaled(g.y), mm.y, vv.y, coef, s);
          opt_adam(p.z, unscaled(g.z), mm.z, vv.z, coef, s);
          opt_adam(p.w, unscaled(g.w), mm.w, vv.w, coef, s);
          opt_store4(P + i, p);
          opt_store4(M + i, mm);
          opt_store4(V + i, vv);
        }
        opt_store4(G + i, make_float4(0.f, 0.f, 0.f, 0.f));
      }
      if (s.ema_mode == 1) {
        opt_store4(E + i, p);
      } else if (s.ema_mode == 2) {
        const float4 e = ld4(E + i);
        opt_store4(E + i, make_float4(opt_lerp(e.x, p.x, s.ema_w), opt_lerp(e.y, p.y, s.ema_w), opt_lerp(e.z, p.z, s.ema_w),
                                      opt_lerp(e.w, p.w, s.ema_w)));
      }
    } else {
      const long end = i + 4 < c.hi ? i + 4 : c.hi;
      for (long q = i; q < end; ++q) {
        float p = P[q];
        if (adam) {
          if (!SCALED || !skip) {
            float mm = M[q], vv = V[q];
            opt_adam(p, unscaled(G[q]), mm, vv, coef, s);
            P[q] = p;
            M[q] = mm;
            V[q] = vv;
          }
          G[q] = 0.f;
        }
        if (s.ema_mode == 1) E[q] = p;
        else if (s.ema_mode == 2) E[q] = opt_lerp(E[q], p, s.ema_w);
      }
    }
  }
}

// ---------------------------------------------------------------- the loss scaler: one thread
__global__ void opt_scaler_init_kernel(ld_dn_scaler_state* st, float scale, int adam_steps, int growth_tracker) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  st->scale = scale;
  st->growth_tracker = growth_tracker;
  st->adam_steps = adam_steps;
  st->skipped_steps = 0;
  st->found_inf = 0;
  st->inv_scale = (float)(1.0 / (double)scale);
  st->step_size = 0.0f;
  st->bc2_sqrt = 1.0f;
}

// GradScaler.step's decision and GradScaler.update (_amp_update_scale_) from the squared norm of the SCALED gradients: it is
// non-finite exactly when a gradient element is (fp64 does not overflow on squares of finite fp32 values)
__global__ void opt_scaler_update_kernel(ld_dn_scaler_state* st, const double* __restrict__ sumsq, double lr, double beta1,
                                         double beta2, double growth, double backoff, int growth_interval) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  ld_dn_scaler_state s = *st;
  const bool found_inf = !isfinite(*sumsq);
  s.found_inf = found_inf ? 1 : 0;
  s.inv_scale = (float)(1.0 / (double)s.scale);                     // of the scale these gradients were produced with
  if (!found_inf) {
    s.adam_steps += 1;
    const double t = (double)s.adam_steps;
    s.step_size = (float)(lr / (1.0 - pow(beta1, t)));              // what ld_dn_opt_step is handed in double and rounds
    s.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, t));
    s.growth_tracker += 1;
    if (s.growth_tracker == growth_interval) {
      const float grown = (float)((double)s.scale * growth);
      if (isfinite(grown)) s.scale = grown;
      s.growth_tracker = 0;
    }
  } else {
    s.skipped_steps += 1;
    s.scale = (float)((double)s.scale * backoff);
    s.growth_tracker = 0;
  }
  *st = s;
}

// ---------------------------------------------------------------- data-parallel: the rank-ordered sum of the gathered gradients
// gathered holds `world` copies of the flat gradient, rank r's at r * stride.  Per element g = copy 0, then += copy 1, 2, ..
// in plain fp32; grad = g, and the workgroup's fp64 partial of g * g is gathered exactly as opt_sqnorm_kernel gathers it (the
// same chunk, the same per-thread order, the same block sum), so the second launch gives the bits ld_dn_opt_sqnorm gives on
// the reduced buffer.  W > 0: world is W, every copy's 16-byte load is issued before the first add; W == 0: any world, the
// copies in batches of RB loads.  grad may be a rank's own slice of gathered: a thread stores only the elements it has
// loaded from every copy, so neither pointer is __restrict__.
constexpr int OPT_RB = 8;

template <int W>
__device__ __forceinline__ float4 opt_sum4(const float* src, int world, long stride) {
  if constexpr (W > 0) {
    float4 q[W];
#pragma unroll
    for (int r = 0; r < W; ++r) q[r] = ld4(src + (long)r * stride);
    float4 g = q[0];
#pragma unroll
    for (int r = 1; r < W; ++r) {
      g.x += q[r].x;
      g.y += q[r].y;
      g.z += q[r].z;
      g.w += q[r].w;
    }
    return g;
  } else {
    float4 g = ld4(src);
    for (int r0 = 1; r0 < world; r0 += OPT_RB) {
      float4 q[OPT_RB];
#pragma unroll
      for (int j = 0; j < OPT_RB; ++j) {
        const int r = r0 + j < world ? r0 + j : world - 1;           // (a repeated load of the last copy, not added)
        q[j] = ld4(src + (long)r * stride);
      }
#pragma unroll
      for (int j = 0; j < OPT_RB; ++j) {
        if (r0 + j < world) {
          g.x += q[j].x;
          g.y += q[j].y;
          g.z += q[j].z;
          g.w += q[j].w;
        }
      }
    }
    return g;
  }
}

template <int W>
__global__ __launch_bounds__(OPT_BS) void opt_reduce_kernel(const ld_dn_opt_tensor* __restrict__ tab, int n, const float* gathered,
                                                            int world_rt, long stride, float* grad, long flat,
                                                            double* __restrict__ partial) {
  __shared__ double red[OPT_BS / 64];
  const int world = W > 0 ? W : world_rt;
  OptChunk c;
  double acc = 0.0;
  if (opt_chunk(tab, n, flat, c) && (c.e.flags & LD_DN_OPT_ADAM)) {
    const float* src = gathered + c.e.offset;
    float* g = grad + c.e.offset;
#pragma unroll
    for (int k = 0; k < OPT_LANES; ++k) {
      const long i = c.lo + 4L * (k * OPT_BS + (int)threadIdx.x);
      if (i >= c.hi) continue;
      if (i + 4 <= c.hi) {
        const float4 q = opt_sum4<W>(src + i, world, stride);
        opt_store4(g + i, q);
        acc += (double)q.x * (double)q.x;
        acc += (double)q.y * (double)q.y;
        acc += (double)q.z * (double)q.z;
        acc += (double)q.w * (double)q.w;
      } else {
        for (long j = i; j < c.hi; ++j) {
          float v = src[j];
          for (int r = 1; r < world; ++r) v += src[(long)r * stride + j];
          g[j] = v;
          acc += (double)v * (double)v;
        }
      }
    }
  }
  const double s = opt_block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// the loss tail: *out = slot `at` of copy 0, then += copy 1, 2, .. (one thread)
__global__ void opt_reduce_tail_kernel(const float* __restrict__ gathered, int world, long stride, long at, float* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float v = gathered[at];
  for (int r = 1; r < world; ++r) v += gathered[(long)r * stride + at];
  *out = v;
}

inline bool opt_sizes_ok(int n_tensors, int n_wg, int64_t flat) {
  return n_tensors > 0 && n_tensors <= LD_DN_OPT_MAX_TENSORS && n_wg >= n_tensors && flat >= 4 && flat % 4 == 0 &&
         flat < (1LL << 40);
}
}  // namespace

extern "C" int ld_dn_opt_layout(ld_dn_opt_tensor* tensors, int n_tensors, int64_t* flat_floats, int64_t* workgroups) {
  LD_REQUIRE(tensors && flat_floats && workgroups, "ld_dn_opt_layout: null pointer");
  LD_REQUIRE(n_tensors > 0 && n_tensors <= LD_DN_OPT_MAX_TENSORS, "ld_dn_opt_layout: %d tensors (1..%d)", n_tensors,
             LD_DN_OPT_MAX_TENSORS);
  int64_t off = 0, wg = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const ld_dn_opt_tensor& t = tensors[i];
    LD_REQUIRE(t.param && reinterpret_cast<uintptr_t>(t.param) % 4 == 0, "ld_dn_opt_layout: tensor %d: null or misaligned parameter", i);
    LD_REQUIRE(t.count > 0 && t.count < (1LL << 40), "ld_dn_opt_layout: tensor %d: %lld elements", i, (long long)t.count);
    LD_REQUIRE((t.flags & ~LD_DN_OPT_ADAM) == 0, "ld_dn_opt_layout: tensor %d: flags %d", i, t.flags);
    off += (t.count + 3) / 4 * 4;
    wg += (t.count + LD_DN_OPT_CHUNK - 1) / LD_DN_OPT_CHUNK;
    LD_REQUIRE(wg < (1LL << 31) && off < (1LL << 40), "ld_dn_opt_layout: too many elements");
  }
  off = wg = 0;
  for (int i = 0; i < n_tensors; ++i) {                 // (nothing is written unless every entry is good)
    tensors[i].offset = off;
    tensors[i].first_wg = (int32_t)wg;
    off += (tensors[i].count + 3) / 4 * 4;
    wg += (tensors[i].count + LD_DN_OPT_CHUNK - 1) / LD_DN_OPT_CHUNK;
  }
  *flat_floats = off;
  *workgroups = wg;
  return LD_OK;
}

extern "C" int64_t ld_dn_opt_sqnorm_work_bytes(int n_wg) {
  return n_wg > 0 ? (int64_t)n_wg * (int64_t)sizeof(double) : 0;
}

extern "C" int ld_dn_opt_sqnorm(const ld_dn_opt_tensor* table, int n_tensors, int n_wg, const float* grad, int64_t flat_floats,
                                double* work, double* sumsq, void* stream) {
  LD_REQUIRE(opt_sizes_ok(n_tensors, n_wg, flat_floats), "ld_dn_opt_sqnorm: %d tensors, %d workgroups, %lld floats (at least one "
             "tensor, a workgroup per tensor, a multiple of 4 floats)", n_tensors, n_wg, (long long)flat_floats);
  LD_REQUIRE(table && grad && work && sumsq, "ld_dn_opt_sqnorm: null pointer");
  LD_REQUIRE(dn_aligned16(grad) && ((uintptr_t)table | (uintptr_t)work | (uintptr_t)sumsq) % 8 == 0,
             "ld_dn_opt_sqnorm: a pointer is not aligned (grad 16 bytes; the table, work and sumsq 8)");
  hipStream_t st = dn_st(stream);
  LD_LAUNCH(opt_sqnorm_kernel, dim3((unsigned)n_wg), dim3(OPT_BS), 0, st, table, n_tensors, grad, (long)flat_floats, work);
  LD_LAUNCH(opt_sqnorm_final_kernel, dim3(1), dim3(OPT_BS), 0, st, (const double*)work, n_wg, sumsq);
  LD_LAUNCH_CHECK("dn_opt_sqnorm");
  return LD_OK;
}

extern "C" int ld_dn_opt_reduce(const ld_dn_opt_tensor* table, int n_tensors, int n_wg, const float* gathered, int world,
                                int64_t rank_stride, float* grad, int64_t flat_floats, double* work, double* sumsq, void* stream) {
  LD_REQUIRE(opt_sizes_ok(n_tensors, n_wg, flat_floats), "ld_dn_opt_reduce: %d tensors, %d workgroups, %lld floats (at least one "
             "tensor, a workgroup per tensor, a multiple of 4 floats)", n_tensors, n_wg, (long long)flat_floats);
  LD_REQUIRE(world >= 1 && world <= LD_DN_OPT_MAX_WORLD, "ld_dn_opt_reduce: world %d (1..%d)", world, LD_DN_OPT_MAX_WORLD);
  LD_REQUIRE(rank_stride >= flat_floats && rank_stride % 4 == 0 && rank_stride < (1LL << 40),
             "ld_dn_opt_reduce: rank_stride %lld (a multiple of 4 floats, at least flat_floats = %lld)", (long long)rank_stride,
             (long long)flat_floats);
  LD_REQUIRE(table && gathered && grad && work && sumsq, "ld_dn_opt_reduce: null pointer");
  LD_REQUIRE(dn_aligned16(gathered) && dn_aligned16(grad) && ((uintptr_t)table | (uintptr_t)work | (uintptr_t)sumsq) % 8 == 0,
             "ld_dn_opt_reduce: a pointer is not aligned (gathered and grad 16 bytes; the table, work and sumsq 8)");
  const uintptr_t g0 = (uintptr_t)gathered, g1 = g0 + (uintptr_t)world * (uintptr_t)rank_stride * 4, d0 = (uintptr_t)grad;
  const bool apart = d0 + (uintptr_t)flat_floats * 4 <= g0 || d0 >= g1;
  LD_REQUIRE(apart || (d0 >= g0 && (d0 - g0) % ((uintptr_t)rank_stride * 4) == 0),
             "ld_dn_opt_reduce: grad overlaps gathered without being one rank's copy");
  hipStream_t st = dn_st(stream);
  const dim3 grid((unsigned)n_wg), block(OPT_BS);
  const long stride = (long)rank_stride, flat = (long)flat_floats;
  switch (world) {
    case 1: LD_LAUNCH(opt_reduce_kernel<1>, grid, block, 0, st, table, n_tensors, gathered, world, stride, grad, flat, work); break;
    case 2: LD_LAUNCH(opt_reduce_kernel<2>, grid, block, 0, st, table, n_tensors, gathered, world, stride, grad, flat, work); break;
    case 4: LD_LAUNCH(opt_reduce_kernel<4>, grid, block, 0, st, table, n_tensors, gathered, world, stride, grad, flat, work); break;
    case 8: LD_LAUNCH(opt_reduce_kernel<8>, grid, block, 0, st, table, n_tensors, gathered, world, stride, grad, flat, work); break;
    default: LD_LAUNCH(opt_reduce_kernel<0>, grid, block, 0, st, table, n_tensors, gathered, world, stride, grad, flat, work); break;
  }
  LD_LAUNCH(opt_sqnorm_final_kernel, dim3(1), dim3(OPT_BS), 0, st, (const double*)work, n_wg, sumsq);
  LD_LAUNCH_CHECK("dn_opt_reduce");
  return LD_OK;
}

extern "C" int ld_dn_opt_reduce_tail(const float* gathered, int world, int64_t rank_stride, int64_t at, float* out, void* stream) {
  LD_REQUIRE(world >= 1 && world <= LD_DN_OPT_MAX_WORLD, "ld_dn_opt_reduce_tail: world %d (1..%d)", world, LD_DN_OPT_MAX_WORLD);
  LD_REQUIRE(rank_stride > 0 && rank_stride < (1LL << 40) && at >= 0 && at < rank_stride,
             "ld_dn_opt_reduce_tail: slot %lld of a rank_stride of %lld floats", (long long)at, (long long)rank_stride);
  LD_REQUIRE(gathered && out, "ld_dn_opt_reduce_tail: null pointer");
  LD_REQUIRE(((uintptr_t)gathered | (uintptr_t)out) % 4 == 0, "ld_dn_opt_reduce_tail: a pointer is not aligned (4 bytes)");
  LD_LAUNCH(opt_reduce_tail_kernel, dim3(1), dim3(64), 0, dn_st(stream), gathered, world, (long)rank_stride, (long)at, out);
  LD_LAUNCH_CHECK("dn_opt_reduce_tail");
  return LD_OK;
}

extern "C" int ld_dn_opt_step(const ld_dn_opt_tensor* table, int n_tensors, int n_wg, float* grad, float* exp_avg,
                              float* exp_avg_sq, float* ema, int64_t flat_floats, const double* sumsq, double max_norm,
                              double beta1, double beta2, double eps, double step_size, double bc2_sqrt, int ema_mode, float ema_w,
                              void* stream) {
  LD_REQUIRE(opt_sizes_ok(n_tensors, n_wg, flat_floats), "ld_dn_opt_step: %d tensors, %d workgroups, %lld floats (at least one "
             "tensor, a workgroup per tensor, a multiple of 4 floats)", n_tensors, n_wg, (long long)flat_floats);
  LD_REQUIRE(max_norm >= 0.0, "ld_dn_opt_step: max_norm %g is negative or NaN", max_norm);
  LD_REQUIRE(bc2_sqrt > 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
             "ld_dn_opt_step: beta1 %g beta2 %g eps %g sqrt(1 - beta2^t) %g", beta1, beta2, eps, bc2_sqrt);
  LD_REQUIRE(ema_mode >= 0 && ema_mode <= 2 && ema_w >= 0.f && ema_w <= 1.f, "ld_dn_opt_step: ema_mode %d (0 keep, 1 copy, 2 lerp) "
             "weight %g (0..1)", ema_mode, (double)ema_w);
  LD_REQUIRE(table && grad && exp_avg && exp_avg_sq && ema && sumsq, "ld_dn_opt_step: null pointer");
  LD_REQUIRE(dn_aligned16(grad) && dn_aligned16(exp_avg) && dn_aligned16(exp_avg_sq) && dn_aligned16(ema) &&
                 ((uintptr_t)table | (uintptr_t)sumsq) % 8 == 0,
             "ld_dn_opt_step: a pointer is not aligned (the flat buffers 16 bytes; the table and sumsq 8)");
  OptScalars s;
  s.omb1 = (float)(1.0 - beta1);
  s.beta2 = (float)beta2;
  s.omb2 = (float)(1.0 - beta2);
  s.eps = (float)eps;
  s.step_size = (float)step_size;
  s.bc2_sqrt = (float)bc2_sqrt;
  s.ema_w = ema_w;
  s.ema_mode = ema_mode;
  LD_LAUNCH(opt_step_kernel<>, dim3((unsigned)n_wg), dim3(OPT_BS), 0, dn_st(stream), table, n_tensors, grad, exp_avg, exp_avg_sq, ema,
            (long)flat_floats, sumsq, max_norm, s);
  LD_LAUNCH_CHECK("dn_opt_step");
  return LD_OK;
}

extern "C" int ld_dn_scaler_init(ld_dn_scaler_state* state, float init_scale, int adam_steps, int growth_tracker, void* stream) {
  LD_REQUIRE(state && (uintptr_t)state % 4 == 0, "ld_dn_scaler_init: null or misaligned state");
  LD_REQUIRE(init_scale > 0.0f && init_scale <= 3.4028234663852886e38f, "ld_dn_scaler_init: init_scale %g (positive and finite)",
             (double)init_scale);
  LD_REQUIRE(adam_steps >= 0 && growth_tracker >= 0, "ld_dn_scaler_init: adam_steps %d, growth_tracker %d (non-negative)",
             adam_steps, growth_tracker);
  LD_LAUNCH(opt_scaler_init_kernel, dim3(1), dim3(64), 0, dn_st(stream), state, init_scale, adam_steps, growth_tracker);
  LD_LAUNCH_CHECK("dn_scaler_init");
  return LD_OK;
}

extern "C" int ld_dn_opt_scaler_update(ld_dn_scaler_state* state, const double* sumsq, double lr, double beta1, double beta2,
                                       double growth_factor, double backoff_factor, int growth_interval, void* stream) {
  LD_REQUIRE(state && sumsq, "ld_dn_opt_scaler_update: null pointer");
  LD_REQUIRE((uintptr_t)state % 4 == 0 && (uintptr_t)sumsq % 8 == 0,
             "ld_dn_opt_scaler_update: a pointer is not aligned (the state 4 bytes, sumsq 8)");
  LD_REQUIRE(lr > 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "ld_dn_opt_scaler_update: lr %g beta1 %g beta2 %g",
             lr, beta1, beta2);
  LD_REQUIRE(growth_factor > 1.0 && backoff_factor > 0.0 && backoff_factor < 1.0 && growth_interval >= 1,
             "ld_dn_opt_scaler_update: growth %g (> 1) backoff %g (0..1) growth_interval %d (>= 1)", growth_factor, backoff_factor,
             growth_interval);
  LD_LAUNCH(opt_scaler_update_kernel, dim3(1), dim3(64), 0, dn_st(stream), state, sumsq, lr, beta1, beta2, growth_factor,
            backoff_factor, growth_interval);
  LD_LAUNCH_CHECK("dn_opt_scaler_update");
  return LD_OK;
}

extern "C" int ld_dn_opt_step_scaled(const ld_dn_opt_tensor* table, int n_tensors, int n_wg, float* grad, float* exp_avg,
                                     float* exp_avg_sq, float* ema, int64_t flat_floats, const double* sumsq,
                                     const ld_dn_scaler_state* state, double max_norm, double beta1, double beta2, double eps,
                                     int ema_mode, float ema_w, void* stream) {
  LD_REQUIRE(opt_sizes_ok(n_tensors, n_wg, flat_floats), "ld_dn_opt_step_scaled: %d tensors, %d workgroups, %lld floats (at least "
             "one tensor, a workgroup per tensor, a multiple of 4 floats)", n_tensors, n_wg, (long long)flat_floats);
  LD_REQUIRE(max_norm >= 0.0, "ld_dn_opt_step_scaled: max_norm %g is negative or NaN", max_norm);
  LD_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0,
             "ld_dn_opt_step_scaled: beta1 %g beta2 %g eps %g", beta1, beta2, eps);
  LD_REQUIRE(ema_mode >= 0 && ema_mode <= 2 && ema_w >= 0.f && ema_w <= 1.f, "ld_dn_opt_step_scaled: ema_mode %d (0 keep, 1 copy, "
             "2 lerp) weight %g (0..1)", ema_mode, (double)ema_w);
  LD_REQUIRE(table && grad && exp_avg && exp_avg_sq && ema && sumsq && state, "ld_dn_opt_step_scaled: null pointer");
  LD_REQUIRE(dn_aligned16(grad) && dn_aligned16(exp_avg) && dn_aligned16(exp_avg_sq) && dn_aligned16(ema) &&
                 ((uintptr_t)table | (uintptr_t)sumsq) % 8 == 0 && (uintptr_t)state % 4 == 0,
             "ld_dn_opt_step_scaled: a pointer is not aligned (the flat buffers 16 bytes; the table and sumsq 8; the state 4)");
  OptScalars s;
  s.omb1 = (float)(1.0 - beta1);
  s.beta2 = (float)beta2;
  s.omb2 = (float)(1.0 - beta2);
  s.eps = (float)eps;
  s.step_size = 0.0f;                                               // (both from the state, on the device)
  s.bc2_sqrt = 1.0f;
  s.ema_w = ema_w;
  s.ema_mode = ema_mode;
  LD_LAUNCH(opt_step_kernel<const ld_dn_scaler_state*>, dim3((unsigned)n_wg), dim3(OPT_BS), 0, dn_st(stream), table, n_tensors,
            grad, exp_avg, exp_avg_sq, ema, (long)flat_floats, sumsq, max_norm, s, state);
  LD_LAUNCH_CHECK("dn_opt_step_scaled");
  return LD_OK;
}
