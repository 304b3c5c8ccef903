// Image-quality sums on the device (include/localdiff_hip.h, "quality metrics"): per sample and per region (whole image, OOD =
// mask >= 1 as ld_recompose reads a mask, IND = the rest) the element count, the squared error in fp64, the number of SSIM
// windows and the sum of their SSIM values.  MSE, PSNR and the mean SSIM are quotients of these on the host (metrics.py).
//
// SSIM is Wang et al.'s with the 11-tap Gaussian window (sigma 1.5), biased moments, K1 = 0.01, K2 = 0.03 and no padding: only
// windows that lie inside the image count, and a window belongs to the region of its centre pixel.  Everything per window is
// fp32 in ONE order -- the horizontal pass, then the vertical one, the taps added in index order, no fused multiply-add
// (-ffp-contract=off) -- which tests/metrics_ref.py restates in torch; the sums over windows and elements are fp64 in a fixed
// order as well (no floating-point atomics), and a sample's partial sums live in its own slice of `work`: its result depends
// neither on the batch size nor on its neighbours, which is what a sharded evaluation rests on.
//
// One workgroup per (sample, channel, tile of 32 x 32 window centres).  LDS:
//   s_img [2][42][44] fp32   the 42 x 42 halo of both images; rows padded to 44 floats so that every row starts on the 16-byte
//                            grid of the staging stores                                                            14,784 B
//   s_h   [5][42][32] fp32   the horizontal pass of the five moments (x, y, xx, yy, xy)                            26,880 B
// In both passes a lane owns a COLUMN (lane & 31) and a 32-lane half owns a row: the 32 lanes of a half -- the group that a
// 4-byte LDS access is banked in, bank = dword address mod 32 -- always touch 32 consecutive dwords, so neither pass has a
// bank conflict whatever the row stride is; the padding serves the alignment only.
#include "common.hip.h"

#include <math.h>

namespace {

constexpr int MT_TILE = 32;              // window centres per tile side
constexpr int MT_WIN = 11;               // taps
constexpr int MT_HALO = MT_TILE + MT_WIN - 1;
constexpr int MT_SP = 44;                // floats per staged row
constexpr int MT_BS = 256;
constexpr int MT_NV = 12;                // 3 regions x (n_elem, sse, n_win, ssim_sum)
constexpr int MT_UNITS = 11;             // staging units per row: ten of 4 floats and one of 2

struct MtTaps { float w[MT_WIN]; };

// The window: exp(-(j - 5)^2 / (2 sigma^2)) / sum in double, rounded to fp32 once.
void mt_taps(float* w) {
  double g[MT_WIN], s = 0.0;
  for (int j = 0; j < MT_WIN; ++j) {
    const double d = (double)(j - MT_WIN / 2);
    g[j] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    s += g[j];
  }
  for (int j = 0; j < MT_WIN; ++j) w[j] = (float)(g[j] / s);
}

// tile counts; false for a shape the launches do not take
bool mt_shape(int B, int C, int H, int W, int& nty, int& ntx, long long& wgs) {
  if (B < 1 || C < 1 || H < MT_WIN || W < MT_WIN) return false;
  nty = (H - MT_WIN + 1 + MT_TILE - 1) / MT_TILE;
  ntx = (W - MT_WIN + 1 + MT_TILE - 1) / MT_TILE;
  wgs = (long long)B * C * nty * ntx;
  return wgs <= 0x7fffffffLL && (long long)C * nty * ntx <= 0x7fffffffLL;
}

__global__ __launch_bounds__(MT_BS) void metric_tile_kernel(const float* __restrict__ pred, const float* __restrict__ ref,
                                                            const float* __restrict__ mask, double* __restrict__ work, int C,
                                                            int H, int W, int nty, int ntx, float c1, float c2, MtTaps taps) {
  __shared__ __attribute__((aligned(16))) float s_img[2][MT_HALO * MT_SP];
  __shared__ float s_h[5][MT_HALO * MT_TILE];
  __shared__ double s_red[MT_BS / 64][MT_NV];
  const int tid = (int)threadIdx.x;
  int id = (int)blockIdx.x;
  const int tx = id % ntx;
  id /= ntx;
  const int ty = id % nty;
  id /= nty;                                            // b * C + c
  const int b = id / C;
  const size_t plane = (size_t)id * H * W;
  const float* mplane = mask ? mask + (size_t)b * H * W : nullptr;
  const int y0 = ty * MT_TILE, x0 = tx * MT_TILE;

  // ---- stage the halo of both images: 16-byte loads where the row's address allows, element loads with bounds elsewhere
  //      (a row on another alignment, the ragged edge of the image); what lies outside the image is zero and feeds no
  //      counted window
  for (int i = tid; i < 2 * MT_HALO * MT_UNITS; i += MT_BS) {
    const int img = i / (MT_HALO * MT_UNITS);
    const int rem = i - img * (MT_HALO * MT_UNITS);
    const int r = rem / MT_UNITS, u = rem - r * MT_UNITS;
    const int y = y0 + r, x = x0 + 4 * u;
    float* dst = &s_img[img][r * MT_SP + 4 * u];
    const bool row_in = y < H;
    const float* src = (img ? ref : pred) + plane + (row_in ? (size_t)y * W : 0) + x;     // (dereferenced inside the image only)
    if (u < MT_UNITS - 1 && row_in && x + 3 < W && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
    } else {
      const int n = u < MT_UNITS - 1 ? 4 : 2;
      for (int e = 0; e < n; ++e) dst[e] = (row_in && x + e < W) ? src[e] : 0.0f;
    }
  }
  __syncthreads();

  double v[MT_NV];
#pragma unroll
  for (int i = 0; i < MT_NV; ++i) v[i] = 0.0;
  const int lc = tid & 31, lr = tid >> 5;

  // ---- squared error: a tile owns the 32 x 32 pixels at its origin, and the last tile of a row / column the rest of its halo
  //      (H <= 32 (nty - 1) + 42), so every pixel of the image has one owner
  const int rlim = ty == nty - 1 ? MT_HALO : MT_TILE, clim = tx == ntx - 1 ? MT_HALO : MT_TILE;
  for (int cb = 0; cb < MT_HALO; cb += 32) {
    const int c = cb + lc;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int r = lr + 8 * k;
      const int y = y0 + r, x = x0 + c;
      if (c < clim && r < rlim && y < H && x < W) {
        const float d = s_img[0][r * MT_SP + c] - s_img[1][r * MT_SP + c];
        const double dd = (double)d;
        const double sq = dd * dd;
        v[0] += 1.0;
        v[1] += sq;
        if (mplane) {
          const bool ood = mplane[(size_t)y * W + x] >= 1.0f;
          v[4] += ood ? 1.0 : 0.0;
          v[5] += ood ? sq : 0.0;
          v[8] += ood ? 0.0 : 1.0;
          v[9] += ood ? 0.0 : sq;
        }
      }
    }
  }

  // ---- horizontal pass: row r of the halo, window columns 0..31
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int r = lr + 8 * k;
    if (r < MT_HALO) {
      const float* px = &s_img[0][r * MT_SP + lc];
      const float* py = &s_img[1][r * MT_SP + lc];
      float ax = 0.f, ay = 0.f, axx = 0.f, ayy = 0.f, axy = 0.f;
#pragma unroll
      for (int j = 0; j < MT_WIN; ++j) {
        const float w = taps.w[j], x = px[j], y = py[j];
        const float tx_ = w * x, ty_ = w * y, txx = w * (x * x), tyy = w * (y * y), txy = w * (x * y);
        if (j == 0) { ax = tx_; ay = ty_; axx = txx; ayy = tyy; axy = txy; }
        else { ax = ax + tx_; ay = ay + ty_; axx = axx + txx; ayy = ayy + tyy; axy = axy + txy; }
      }
      const int o = r * MT_TILE + lc;
      s_h[0][o] = ax; s_h[1][o] = ay; s_h[2][o] = axx; s_h[3][o] = ayy; s_h[4][o] = axy;
    }
  }
  __syncthreads();

  // ---- vertical pass and the SSIM of window (y0 + r, x0 + lc), whose centre pixel is 5 down and 5 right of that
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = lr + 8 * k;
    float m[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const float* ph = &s_h[q][r * MT_TILE + lc];
      float a = taps.w[0] * ph[0];
#pragma unroll
      for (int j = 1; j < MT_WIN; ++j) a = a + taps.w[j] * ph[j * MT_TILE];
      m[q] = a;
    }
    const int oy = y0 + r, ox = x0 + lc;
    if (oy < H - (MT_WIN - 1) && ox < W - (MT_WIN - 1)) {
      const float mx = m[0], my = m[1];
      const float mxx = mx * mx, myy = my * my, mxy = mx * my;
      const float sx = m[2] - mxx, sy = m[3] - myy, sxy = m[4] - mxy;
      const float num = (2.0f * mxy + c1) * (2.0f * sxy + c2);
      const float den = (mxx + myy + c1) * (sx + sy + c2);
      const double s = (double)(num / den);
      v[2] += 1.0;
      v[3] += s;
      if (mplane) {
        const bool ood = mplane[(size_t)(oy + MT_WIN / 2) * W + ox + MT_WIN / 2] >= 1.0f;
        v[6] += ood ? 1.0 : 0.0;
        v[7] += ood ? s : 0.0;
        v[10] += ood ? 0.0 : 1.0;
        v[11] += ood ? 0.0 : s;
      }
    }
  }

  // ---- the workgroup's twelve sums in a fixed order: a xor tree inside each wave, then the four waves in index order
#pragma unroll
  for (int i = 0; i < MT_NV; ++i) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[i] += __shfl_xor(v[i], off);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < MT_NV; ++i) s_red[tid >> 6][i] = v[i];
  }
  __syncthreads();
  if (tid < MT_NV) {
    double s = s_red[0][tid];
    for (int wv = 1; wv < MT_BS / 64; ++wv) s += s_red[wv][tid];
    work[(size_t)blockIdx.x * MT_NV + tid] = s;
  }
}

// out[b][.] = the sample's partial sums added in (channel, tile row, tile column) order, which is their order in `work`
__global__ __launch_bounds__(64) void metric_finish_kernel(const double* __restrict__ work, double* __restrict__ out, int nparts) {
  const int f = (int)threadIdx.x;
  if (f >= MT_NV) return;
  const double* p = work + (size_t)blockIdx.x * nparts * MT_NV + f;
  double s = 0.0;
#pragma unroll 8
  for (int i = 0; i < nparts; ++i) s += p[(size_t)i * MT_NV];
  out[(size_t)blockIdx.x * MT_NV + f] = s;
}

}  // namespace

extern "C" int ld_metric_taps(float* taps /* host, 11 */) {
  LD_REQUIRE(taps, "ld_metric_taps: null pointer");
  mt_taps(taps);
  return LD_OK;
}

extern "C" int64_t ld_metric_work_doubles(int B, int C, int H, int W) {
  int nty, ntx;
  long long wgs;
  return mt_shape(B, C, H, W, nty, ntx, wgs) ? (int64_t)wgs * MT_NV : 0;
}

extern "C" int ld_metric_sums(const float* pred, const float* ref, const float* mask, double* work, double* out, int B, int C,
                              int H, int W, float data_range, void* stream) {
  LD_REQUIRE(pred && ref && work && out, "ld_metric_sums: null pointer (pred, ref, work and out are required)");
  LD_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "ld_metric_sums: B %d, C %d, H %d, W %d must be at least 1", B, C, H, W);
  LD_REQUIRE(H >= MT_WIN && W >= MT_WIN, "ld_metric_sums: H %d, W %d: the 11 x 11 SSIM window does not fit", H, W);
  LD_REQUIRE(isfinite(data_range) && data_range > 0.0f, "ld_metric_sums: data_range %g must be finite and positive",
             (double)data_range);
  LD_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0 && (reinterpret_cast<uintptr_t>(work) & 7) == 0,
             "ld_metric_sums: out and work must be 8-byte aligned");
  LD_REQUIRE(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(ref) | reinterpret_cast<uintptr_t>(mask)) & 3) == 0,
             "ld_metric_sums: pred, ref and mask must be 4-byte aligned");
  int nty, ntx;
  long long wgs;
  LD_REQUIRE(mt_shape(B, C, H, W, nty, ntx, wgs), "ld_metric_sums: B %d, C %d, H %d, W %d is more than 2^31 - 1 tiles", B, C, H, W);
  MtTaps taps;
  mt_taps(taps.w);
  const double l = (double)data_range;
  const float c1 = (float)((0.01 * l) * (0.01 * l)), c2 = (float)((0.03 * l) * (0.03 * l));     // in double, rounded once
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LD_LAUNCH(metric_tile_kernel, dim3((unsigned)wgs), dim3(MT_BS), 0, st, pred, ref, mask, work, C, H, W, nty, ntx, c1, c2, taps);
  LD_LAUNCH_CHECK("metric_tile");
  LD_LAUNCH(metric_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, (const double*)work, out, C * nty * ntx);
  LD_LAUNCH_CHECK("metric_finish");
  return LD_OK;
}
