// torch.optim.Adam's update of one element (no weight decay, no amsgrad), shared by ld_seg_adam (segtrain.hip) and the
// denoiser's fused step (denoiser_opt.hip): built with -ffp-contract=off, it gives the same bits wherever it is inlined.
#pragma once

// p, m, v are updated in place.  omb = 1 - beta, rounded to fp32 from the host's double as torch rounds the Python scalar
// (1 - 0.999f is 4.7e-5 off 0.001f); step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)
__device__ __forceinline__ void ld_adam_update(float& p, float g, float& m, float& v, float omb1, float beta2, float omb2,
                                               float eps, float step_size, float bc2_sqrt) {
  const float mi = m + omb1 * (g - m);                            // exp_avg.lerp_(grad, 1 - beta1)
  const float vi = v * beta2 + omb2 * g * g;                      // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  m = mi;
  v = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p = p + (-step_size) * (mi / denom);
}
