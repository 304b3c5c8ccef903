// Device-resident training data (the reference's data.py: MNIST, MvtecDatasetSR, MedDataset_png as Trainer builds them):
// one launch turns B rows of a per-sample table into a batch -- gather from the store, RandomRotation's nearest-neighbour
// rotation, RandomVerticalFlip, the data set's normalisation and its low-resolution partner -- as contiguous fp32 NCHW.
//
//   ld_ds_mnist_batch   u8 [N, S, S]      hr = 2 (x / 255); lr = the even ROWS of the transformed image, bilinear back to S rows
//   ld_ds_sr_batch      u8 [N, C, S, S]   hr = (x / 255) 2; lr = its even rows and columns, bilinear back to S x S
//   ld_ds_mri_batch     fp32 [N, R, R] x2 centre crop, the same rotation and flip for both, (x - mean) / std, + |min| of the image
// and the two labelled data sets (MedSegDataset for SegTrainer, MNIST with its labels for MnistClassifierTrainer):
//   ld_ds_seg_batch       fp32 + u8 [N, R, R]  centre crop, the same rotation and flip for both; x = (v - mean) / std, target = label > 0
//   ld_ds_mnist_cls_batch u8 [N, S, S] + u8 [N] x = ld_ds_mnist_batch's hr; label = the sample's class as int64 (no lr)
//
// A thread produces four consecutive pixels of a plane (one 16-byte store per output); a plane has a multiple of four
// pixels (S even, crop a multiple of 4), so a group may straddle two rows and every pixel computes its own coordinates.
// The sample's table row is read through scalar loads (its index comes from blockIdx).  No LDS.  The source pixel of
// (i, j) under (cos a, sin a, flip), for an H x W image (torchvision's tensor rotate, NEAREST, expand = False, fill = None):
//   i' = flip ? H - 1 - i : i          (the flip comes after the rotation and reverses the rows)
//   xo = j - (W-1)/2, yo = i' - (H-1)/2
//   sx = cos a * xo - sin a * yo + (W-1)/2,  sy = sin a * xo + cos a * yo + (H-1)/2
//   source (rint(sy), rint(sx)), half to even; outside the image: 0
// in single, separately rounded fp32 operations (__fmul_rn / __fadd_rn: nothing contracts), as is every other operation of
// the mnist and mri paths, whose outputs are therefore those of the same chain on any IEEE machine.  Divisions are IEEE
// divisions.  There is no floating-point atomic: the mri minimum is a minimum (exact in any order), taken per image over
// LD_DS_MIN_PARTS row bands by one wave each and finished by the batch kernel.  Because (x - mean) / std is monotone in x
// for std > 0, the minimum of the normalised image is the normalised minimum of the raw one.
// The HOST validates the table's indices; the kernels clamp them to [0, N) only so that a corrupted table stays in bounds.
#include "common.hip.h"

namespace {
constexpr int DS_BLOCK = 256;
typedef ld_ds_row DsRow;

__device__ __forceinline__ int ds_index(const DsRow& r, int N) { return min(max(r.src, 0), N - 1); }

// the source pixel of output (i, j); false when it lies outside the H x W image
__device__ __forceinline__ bool ds_source(const DsRow& r, int i, int j, int H, int W, int& sy, int& sx) {
  const int ir = r.flip ? H - 1 - i : i;
  const float cx = (float)(W - 1) * 0.5f, cy = (float)(H - 1) * 0.5f;
  const float xo = (float)j - cx, yo = (float)ir - cy;
  const float fx = rintf(__fadd_rn(__fsub_rn(__fmul_rn(r.cos_a, xo), __fmul_rn(r.sin_a, yo)), cx));
  const float fy = rintf(__fadd_rn(__fadd_rn(__fmul_rn(r.sin_a, xo), __fmul_rn(r.cos_a, yo)), cy));
  if (!(fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) return false;     // (a NaN is outside)
  sx = (int)fx;
  sy = (int)fy;
  return true;
}

// 2x bilinear upsampling with align_corners = False along one axis: output index o of 2 n reads inputs a and b with weights
// wa and wb (source coordinate o / 2 - 0.25, clamped at 0; the upper neighbour clamped at n - 1)
__device__ __forceinline__ void ds_up2(int o, int n, int& a, int& b, float& wa, float& wb) {
  const int k = o >> 1;
  if (o & 1) { a = k; b = min(k + 1, n - 1); wa = 0.75f; wb = 0.25f; }
  else if (k == 0) { a = 0; b = min(1, n - 1); wa = 1.0f; wb = 0.0f; }
  else { a = k - 1; b = k; wa = 0.25f; wb = 0.75f; }
}

__device__ __forceinline__ void ds_put4(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

// ------------------------------------------------------------------------------------------------ mnist
struct DsU8 {                       // the transformed image of one plane, widened to float (0..255), 0 outside
  const unsigned char* img; DsRow r; int S;
  __device__ __forceinline__ float at(int i, int j) const {
    int sy, sx;
    return ds_source(r, i, j, S, S, sy, sx) ? (float)img[sy * S + sx] : 0.0f;
  }
};

__global__ __launch_bounds__(DS_BLOCK) void ds_mnist_kernel(const unsigned char* __restrict__ store, const DsRow* __restrict__ table,
                                                           float* hr, float* lr, int S, int N, int groups, int bpp) {
  const int b = blockIdx.x / bpp;
  const int g = (blockIdx.x - b * bpp) * DS_BLOCK + threadIdx.x;
  if (g >= groups) return;                                     // (784 pixels = 196 groups: the tail of the last wave)
  DsU8 T;
  T.r = table[b];
  T.S = S;
  T.img = store + (size_t)ds_index(T.r, N) * S * S;
  float h[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int p = 4 * g + e, i = p / S, j = p - i * S;
    int ra, rb;
    float wa, wb;
    ds_up2(i, S >> 1, ra, rb, wa, wb);
    const float v = T.at(i, j), va = T.at(2 * ra, j), vb = T.at(2 * rb, j);
    h[e] = __fmul_rn(2.0f, __fdiv_rn(v, 255.0f));
    // (0.25 / 0.75 of integers up to 255: both products and the sum are exact)
    l[e] = __fmul_rn(2.0f, __fdiv_rn(__fadd_rn(__fmul_rn(va, wa), __fmul_rn(vb, wb)), 255.0f));
  }
  const size_t at = (size_t)b * S * S + 4 * (size_t)g;
  ds_put4(hr + at, h);
  ds_put4(lr + at, l);
}

// ------------------------------------------------------------------------------------------------ sr
struct DsU8Hr {                     // the same in the hr range: (x / 255) * 2
  DsU8 t;
  __device__ __forceinline__ float at(int i, int j) const { return __fmul_rn(__fdiv_rn(t.at(i, j), 255.0f), 2.0f); }
};

__global__ __launch_bounds__(DS_BLOCK) void ds_sr_kernel(const unsigned char* __restrict__ store, const DsRow* __restrict__ table,
                                                        float* hr, float* lr, int S, int C, int N, int groups, int bpp) {
  const int plane = blockIdx.x / bpp;                          // b * C + c
  const int g = (blockIdx.x - plane * bpp) * DS_BLOCK + threadIdx.x;
  if (g >= groups) return;
  const int b = plane / C, c = plane - b * C;
  DsU8Hr T;
  T.t.r = table[b];
  T.t.S = S;
  T.t.img = store + ((size_t)ds_index(T.t.r, N) * C + c) * S * S;
  float h[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int p = 4 * g + e, i = p / S, j = p - i * S;
    int ra, rb, ca, cb;
    float wra, wrb, wca, wcb;
    ds_up2(i, S >> 1, ra, rb, wra, wrb);
    ds_up2(j, S >> 1, ca, cb, wca, wcb);
    h[e] = T.at(i, j);
    // the columns of each of the two rows first, then the rows (the order of ATen's separable kernel)
    const float r0 = __fadd_rn(__fmul_rn(T.at(2 * ra, 2 * ca), wca), __fmul_rn(T.at(2 * ra, 2 * cb), wcb));
    const float r1 = __fadd_rn(__fmul_rn(T.at(2 * rb, 2 * ca), wca), __fmul_rn(T.at(2 * rb, 2 * cb), wcb));
    l[e] = __fadd_rn(__fmul_rn(r0, wra), __fmul_rn(r1, wrb));
  }
  const size_t at = (size_t)plane * S * S + 4 * (size_t)g;
  ds_put4(hr + at, h);
  ds_put4(lr + at, l);
}

// ------------------------------------------------------------------------------------------------ mri
struct DsF32 {                      // the cropped, transformed image of one modality, 0 outside the crop
  const float* img; DsRow r; int R, crop, top;
  __device__ __forceinline__ float at(int i, int j) const {
    int sy, sx;
    return ds_source(r, i, j, crop, crop, sy, sx) ? img[(size_t)(top + sy) * R + top + sx] : 0.0f;
  }
};

// work[(b * 2 + modality) * LD_DS_MIN_PARTS + part] = the minimum of the raw transformed image over the part's rows (+inf for
// a part without rows); one wave per part
__global__ __launch_bounds__(64) void ds_mri_min_kernel(const float* __restrict__ target, const float* __restrict__ cond,
                                                       const DsRow* __restrict__ table, float* work, int R, int crop, int top, int N) {
  const int plane = blockIdx.x / LD_DS_MIN_PARTS, part = blockIdx.x - plane * LD_DS_MIN_PARTS;
  const int b = plane >> 1;
  DsF32 T;
  T.r = table[b];
  T.R = R; T.crop = crop; T.top = top;
  T.img = ((plane & 1) ? cond : target) + (size_t)ds_index(T.r, N) * R * R;
  const int p0 = (part * crop / LD_DS_MIN_PARTS) * crop, p1 = ((part + 1) * crop / LD_DS_MIN_PARTS) * crop;
  float m = __builtin_inff();
  for (int p = p0 + (int)threadIdx.x; p < p1; p += 64) {
    const int i = p / crop;
    m = fminf(m, T.at(i, p - i * crop));
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fminf(m, __shfl_xor(m, off));         // (every lane is here: the loop has ended)
  if (threadIdx.x == 0) work[blockIdx.x] = m;
}

__global__ __launch_bounds__(DS_BLOCK) void ds_mri_kernel(const float* __restrict__ target, const float* __restrict__ cond,
                                                         const DsRow* __restrict__ table, const float* __restrict__ work, float* hr,
                                                         float* lr, int R, int crop, int top, int N, float mean_t, float std_t,
                                                         float mean_c, float std_c, int groups, int bpp) {
  const int plane = blockIdx.x / bpp;                          // b * 2 + modality
  const int g = (blockIdx.x - plane * bpp) * DS_BLOCK + threadIdx.x;
  if (g >= groups) return;
  const int b = plane >> 1, mod = plane & 1;
  const float mean = mod ? mean_c : mean_t, sd = mod ? std_c : std_t;
  DsF32 T;
  T.r = table[b];
  T.R = R; T.crop = crop; T.top = top;
  T.img = (mod ? cond : target) + (size_t)ds_index(T.r, N) * R * R;
  float shift = 0.0f;
  if (work) {                                                  // translate_zero (uniform)
    const float* w = work + (size_t)plane * LD_DS_MIN_PARTS;
    float m = w[0];
#pragma unroll
    for (int k = 1; k < LD_DS_MIN_PARTS; ++k) m = fminf(m, w[k]);
    shift = fabsf(__fdiv_rn(__fsub_rn(m, mean), sd));
  }
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int p = 4 * g + e, i = p / crop;
    v[e] = __fdiv_rn(__fsub_rn(T.at(i, p - i * crop), mean), sd);
    if (work) v[e] = __fadd_rn(v[e], shift);
  }
  ds_put4((mod ? lr : hr) + (size_t)b * crop * crop + 4 * (size_t)g, v);
}

// ------------------------------------------------------------------------------------------------ seg
// MedSegDataset.__getitem__: plane b * 2 is the image (fp32, normalised), plane b * 2 + 1 the label (u8 -> {0, 1}).  ONE launch
// of B * 2 planes rather than one per output: a batch is launch-bound (a few us of kernel under tens of us of launch), the
// plane's kind is uniform over a block (no divergence), and both planes of a sample read the same table row and compute the
// same source coordinates, so image and label cannot drift apart -- the arrangement ds_mri_kernel has for its two modalities.
__global__ __launch_bounds__(DS_BLOCK) void ds_seg_kernel(const float* __restrict__ image, const unsigned char* __restrict__ label,
                                                         const DsRow* __restrict__ table, float* x, float* target, int R, int crop,
                                                         int top, int N, float mean, float sd, int groups, int bpp) {
  const int plane = blockIdx.x / bpp;                          // b * 2 + (0: image, 1: label)
  const int g = (blockIdx.x - plane * bpp) * DS_BLOCK + threadIdx.x;
  if (g >= groups) return;
  const int b = plane >> 1;
  DsF32 T;
  T.r = table[b];
  T.R = R; T.crop = crop; T.top = top;
  const size_t base = (size_t)ds_index(T.r, N) * R * R;
  T.img = image + base;
  const unsigned char* lab = label + base;
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int p = 4 * g + e, i = p / crop, j = p - i * crop;
    if (plane & 1) {                                           // (uniform)
      int sy, sx;
      v[e] = (ds_source(T.r, i, j, crop, crop, sy, sx) && lab[(size_t)(top + sy) * R + top + sx] > 0) ? 1.0f : 0.0f;
    } else {
      v[e] = __fdiv_rn(__fsub_rn(T.at(i, j), mean), sd);       // (0 outside the rotated image, then normalised)
    }
  }
  ds_put4(((plane & 1) ? target : x) + (size_t)b * crop * crop + 4 * (size_t)g, v);
}

// ------------------------------------------------------------------------------------------------ mnist with labels
// ds_mnist_kernel without lr; the sample's label is written by the owner of pixel group 0 of the sample's first block
__global__ __launch_bounds__(DS_BLOCK) void ds_mnist_cls_kernel(const unsigned char* __restrict__ store,
                                                               const unsigned char* __restrict__ labels,
                                                               const DsRow* __restrict__ table, float* x, long long* label, int S, int N,
                                                               int groups, int bpp) {
  const int b = blockIdx.x / bpp;
  const int g = (blockIdx.x - b * bpp) * DS_BLOCK + threadIdx.x;
  if (g >= groups) return;
  DsU8 T;
  T.r = table[b];
  T.S = S;
  const int src = ds_index(T.r, N);
  T.img = store + (size_t)src * S * S;
  float h[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int p = 4 * g + e, i = p / S;
    h[e] = __fmul_rn(2.0f, __fdiv_rn(T.at(i, p - i * S), 255.0f));
  }
  ds_put4(x + (size_t)b * S * S + 4 * (size_t)g, h);
  if (g == 0) label[b] = (long long)labels[src];
}

// the second output is written with 16-byte stores too, or (lr_mask = 7) is ld_ds_mnist_cls_batch's int64 labels
int ds_check_common(const char* name, const void* store, int N, const void* table, int B, const void* hr, const void* lr,
                    unsigned lr_mask = 15) {
  LD_REQUIRE(store && table && hr && lr, "%s: null pointer", name);
  LD_REQUIRE(N >= 1, "%s: the store holds N = %d images", name, N);
  LD_REQUIRE(B >= 1, "%s: B = %d (an empty batch)", name, B);
  LD_REQUIRE(((uintptr_t)hr & 15) == 0 && ((uintptr_t)lr & lr_mask) == 0 && ((uintptr_t)table & 3) == 0,
             lr_mask == 15 ? "%s: hr and lr must be 16-byte aligned, the table 4-byte"
                           : "%s: x must be 16-byte aligned, label 8-byte, the table 4-byte", name);
  return 0;
}

// grid of `planes` planes of `pixels` pixels each (a multiple of 4): groups of four per plane, blocks per plane
int ds_grid(const char* name, long planes, long pixels, int& groups, int& bpp, unsigned& blocks) {
  groups = (int)(pixels / 4);
  bpp = (groups + DS_BLOCK - 1) / DS_BLOCK;
  LD_REQUIRE(planes * bpp <= 0x7fffffffL && planes * pixels <= 0x7fffffffL * 4, "%s: %ld planes of %ld pixels exceed the grid", name,
             planes, pixels);
  blocks = (unsigned)(planes * bpp);
  return 0;
}
}  // namespace

extern "C" int ld_ds_mnist_batch(const void* store_u8, int N, int S, const ld_ds_row* table, int B, float* hr, float* lr, void* stream) {
  if (int rc = ds_check_common("ld_ds_mnist_batch", store_u8, N, table, B, hr, lr)) return rc;
  LD_REQUIRE(S >= 2 && S % 2 == 0 && S <= 16384, "ld_ds_mnist_batch: S = %d must be even (2..16384)", S);
  int groups, bpp;
  unsigned blocks;
  if (int rc = ds_grid("ld_ds_mnist_batch", B, (long)S * S, groups, bpp, blocks)) return rc;
  LD_LAUNCH(ds_mnist_kernel, dim3(blocks), dim3(DS_BLOCK), 0, (hipStream_t)stream, (const unsigned char*)store_u8, table, hr, lr, S, N,
            groups, bpp);
  LD_LAUNCH_CHECK("ds_mnist_kernel");
  return 0;
}

extern "C" int ld_ds_sr_batch(const void* store_u8, int N, int C, int S, const ld_ds_row* table, int B, float* hr, float* lr,
                              void* stream) {
  if (int rc = ds_check_common("ld_ds_sr_batch", store_u8, N, table, B, hr, lr)) return rc;
  LD_REQUIRE(C == 1 || C == 3, "ld_ds_sr_batch: C = %d (1 or 3)", C);
  LD_REQUIRE(S >= 2 && S % 2 == 0 && S <= 16384, "ld_ds_sr_batch: S = %d must be even (2..16384)", S);
  int groups, bpp;
  unsigned blocks;
  if (int rc = ds_grid("ld_ds_sr_batch", (long)B * C, (long)S * S, groups, bpp, blocks)) return rc;
  LD_LAUNCH(ds_sr_kernel, dim3(blocks), dim3(DS_BLOCK), 0, (hipStream_t)stream, (const unsigned char*)store_u8, table, hr, lr, S, C, N,
            groups, bpp);
  LD_LAUNCH_CHECK("ds_sr_kernel");
  return 0;
}

extern "C" int ld_ds_mri_batch(const float* target, const float* cond, int N, int R, int crop, const ld_ds_row* table, int B,
                               float mean_target, float std_target, float mean_cond, float std_cond, int translate_zero,
                               float* work, float* hr, float* lr, void* stream) {
  if (int rc = ds_check_common("ld_ds_mri_batch", target, N, table, B, hr, lr)) return rc;
  LD_REQUIRE(cond, "ld_ds_mri_batch: null pointer");
  LD_REQUIRE(R >= 1 && R <= 16384, "ld_ds_mri_batch: R = %d (1..16384)", R);
  LD_REQUIRE(crop >= 4 && crop <= R, "ld_ds_mri_batch: crop = %d does not fit R = %d", crop, R);
  LD_REQUIRE(crop % 4 == 0, "ld_ds_mri_batch: crop = %d must be a multiple of 4", crop);
  LD_REQUIRE(std_target > 0.0f && std_cond > 0.0f && std_target <= 3.0e38f && std_cond <= 3.0e38f && mean_target == mean_target &&
             mean_cond == mean_cond, "ld_ds_mri_batch: std must be positive and finite, mean a number");
  LD_REQUIRE(!translate_zero || work, "ld_ds_mri_batch: translate_zero needs work (B * 2 * %d floats)", LD_DS_MIN_PARTS);
  LD_REQUIRE((long)B * 2 * LD_DS_MIN_PARTS <= 0x7fffffffL, "ld_ds_mri_batch: B = %d exceeds the grid", B);
  int groups, bpp;
  unsigned blocks;
  if (int rc = ds_grid("ld_ds_mri_batch", (long)B * 2, (long)crop * crop, groups, bpp, blocks)) return rc;
  // CenterCrop: top = left = int(round((R - crop) / 2)), Python's round (half to even)
  const int d = R - crop, top = (d & 1) ? ((d / 2) & 1 ? d / 2 + 1 : d / 2) : d / 2;
  if (translate_zero) {
    LD_LAUNCH(ds_mri_min_kernel, dim3((unsigned)(B * 2 * LD_DS_MIN_PARTS)), dim3(64), 0, (hipStream_t)stream, target, cond, table, work, R,
              crop, top, N);
    LD_LAUNCH_CHECK("ds_mri_min_kernel");
  }
  LD_LAUNCH(ds_mri_kernel, dim3(blocks), dim3(DS_BLOCK), 0, (hipStream_t)stream, target, cond, table,
            (const float*)(translate_zero ? work : nullptr), hr, lr, R, crop, top, N, mean_target, std_target, mean_cond, std_cond, groups,
            bpp);
  LD_LAUNCH_CHECK("ds_mri_kernel");
  return 0;
}

extern "C" int ld_ds_seg_batch(const float* image, const void* label_u8, int N, int R, int crop, const ld_ds_row* table, int B,
                               float mean, float sd, float* x, float* target, void* stream) {
  if (int rc = ds_check_common("ld_ds_seg_batch", image, N, table, B, x, target)) return rc;
  LD_REQUIRE(label_u8, "ld_ds_seg_batch: null pointer");
  LD_REQUIRE(R >= 1 && R <= 16384, "ld_ds_seg_batch: R = %d (1..16384)", R);
  LD_REQUIRE(crop >= 4 && crop <= R, "ld_ds_seg_batch: crop = %d does not fit R = %d", crop, R);
  LD_REQUIRE(crop % 4 == 0, "ld_ds_seg_batch: crop = %d must be a multiple of 4", crop);
  LD_REQUIRE(sd > 0.0f && sd <= 3.0e38f && mean == mean, "ld_ds_seg_batch: std must be positive and finite, mean a number");
  int groups, bpp;
  unsigned blocks;
  if (int rc = ds_grid("ld_ds_seg_batch", (long)B * 2, (long)crop * crop, groups, bpp, blocks)) return rc;
  const int d = R - crop, top = (d & 1) ? ((d / 2) & 1 ? d / 2 + 1 : d / 2) : d / 2;      // ld_ds_mri_batch's CenterCrop
  LD_LAUNCH(ds_seg_kernel, dim3(blocks), dim3(DS_BLOCK), 0, (hipStream_t)stream, image, (const unsigned char*)label_u8, table, x, target,
            R, crop, top, N, mean, sd, groups, bpp);
  LD_LAUNCH_CHECK("ds_seg_kernel");
  return 0;
}

extern "C" int ld_ds_mnist_cls_batch(const void* store_u8, const void* labels_u8, int N, int S, const ld_ds_row* table, int B, float* x,
                                     long long* label, void* stream) {
  if (int rc = ds_check_common("ld_ds_mnist_cls_batch", store_u8, N, table, B, x, label, 7)) return rc;
  LD_REQUIRE(labels_u8, "ld_ds_mnist_cls_batch: null pointer");
  LD_REQUIRE(S >= 2 && S % 2 == 0 && S <= 16384, "ld_ds_mnist_cls_batch: S = %d must be even (2..16384)", S);
  int groups, bpp;
  unsigned blocks;
  if (int rc = ds_grid("ld_ds_mnist_cls_batch", B, (long)S * S, groups, bpp, blocks)) return rc;
  LD_LAUNCH(ds_mnist_cls_kernel, dim3(blocks), dim3(DS_BLOCK), 0, (hipStream_t)stream, (const unsigned char*)store_u8,
            (const unsigned char*)labels_u8, table, x, label, S, N, groups, bpp);
  LD_LAUNCH_CHECK("ds_mnist_cls_kernel");
  return 0;
}
