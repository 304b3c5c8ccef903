#!/usr/bin/env python3
"""Times one training step of the denoiser -- ``ldh.DenoiserTrainer.train_step`` on one batch: ``q_sample``, forward, loss,
backward, and the fused clip / Adam / zero_grad / EMA launch pair -- against the same step in eager PyTorch on the same GPU in
one process: the eager ``Unet`` of tools/bench_unet_grad.py under autograd, ``clip_grad_norm_``, ``torch.optim.Adam`` in its
default mode and a per-tensor ``lerp_`` EMA.  fp32, ms per step.

  python tools/bench_denoiser_train.py [--iters 20] [--warmup 3] [--cases data:H:B,...] [--timeout 300]
                                       [--conv-precision fp32|bf16]   (the HIP trainer's convolutions; eager stays fp32)
                                       [--amp no|fp16]   (fp16: DenoiserTrainer(amp=True): fp16 convolutions and the loss scaler)
                                       [--amp-attn fp32|fp16]   (fp16, with --amp fp16: the attention cores on the fp16 matrix cores)
                                       [--act-storage fp32|bf16]      (bf16 storage of conv-only activations; peak_mb shows it)
                                       [--conv-out-storage fp32|bf16] (bf16 storage of the convolution outputs GroupNorm reads)
A case is data:H = W:batch; the default cases are those of tools/bench_unet_grad.py (cfg3 = mvtec 3 x 256^2 B = 8, mri 256^2
B = 8, mnist 28^2 B = 64).  Every case runs in a child process of its own under ``--timeout``, and the first case that fails
or runs out of time ends the run.  Per case: 3 warm-up steps, then the median of 20.  The EMA lerps at every step on both
sides (the most expensive of its three modes).

The optimiser alone is timed too: ``apply()`` -- ``ld_dn_opt_sqnorm`` and ``ld_dn_opt_step`` of csrc/denoiser_opt.hip --
against eager's clip + Adam + EMA on gradients that are already there, and its memory traffic: 4 bytes x (p, g, m, v, ema read;
p, m, v, ema, g written) per parameter (the norm's second read of the gradient is not counted) over the GPU time of its three
launches (the median of five runs under the library's per-launch timing session; ``apply()`` itself also pays the host's walk
over the parameters).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_bench                                                 # noqa: E402  (puts the repository root on sys.path)
import bench_unet_grad as U                                       # noqa: E402
import localdiffusion_hallucination_amd as ldh                    # noqa: E402

OPTS = dict(branch_out=False, start_intermediate=False, start_timestep=2, mask_x=False, ood_AD=False, ood_confidence=False,
            classifier=False, use_gt=False)
LR, BETAS, MAX_NORM, EMA_W = 1e-4, (0.9, 0.99), 1.0, 0.005


def run_case(data, H, B, a):
    ldh.configure_runtime()
    torch.manual_seed(0)
    inf = ldh.Unet(dim=32, init_dim=32, **U.KWARGS[data])
    gd = ldh.GaussianDiffusion(dict(OPTS, data=data), inf, image_size=H, timesteps=1000, objective="pred_v").cuda()
    tr = ldh.DenoiserTrainer(gd, train_lr=LR, adam_betas=BETAS, max_grad_norm=MAX_NORM, ema_update_every=1, ema_update_after_step=0,
                             **grad_bench.switch_values(a, U.SWITCHES), amp=a.amp == "fp16", amp_attn=a.amp_attn)
    tr.ema_initted = True                                         # (every call lerps)
    cfg = tr.online_model.cfg
    hr = torch.rand(B, cfg.channels, H, H, device="cuda")
    lr = torch.rand(B, cfg.cond_in_channels, H, H, device="cuda") * 2
    t = torch.randint(0, 1000, (B,), device="cuda")
    noise = torch.randn(B, cfg.channels, H, H, device="cuda")

    def hip_step():
        tr.accumulate(hr, lr, t=t, noise=noise)
        tr.apply()

    torch.cuda.reset_peak_memory_stats()
    hip = grad_bench.time_ms(hip_step, a.iters, a.warmup)
    peak = torch.cuda.max_memory_allocated()                      # (of the timed HIP steps: before the eager side exists)
    tr.accumulate(hr, lr, t=t, noise=noise)
    hip_opt = grad_bench.time_ms(tr.apply, a.iters, a.warmup)     # (the gradients are zero after the first: the traffic is the same)
    kern = []
    for _ in range(5):                                            # the two launches alone, under the library's timing session
        split, _ = grad_bench.kernel_split(lambda set_phase: tr.apply())
        kern.append(sum(v[0] for k, v in split.items() if k.startswith("dn_opt_")))
    hip_kern = sorted(kern)[2]
    n_all = sum(p.numel() for p in tr.online_model.parameters())
    nbytes = 4 * 10 * n_all
    row = dict(data=data, H=H, B=B, **grad_bench.switch_values(a, U.SWITCHES), amp=a.amp, amp_attn=a.amp_attn, peak_mb=peak / 2 ** 20, hip_ms=hip, hip_opt_ms=hip_opt,
               hip_opt_kernels_ms=hip_kern, params=n_all, tensors=len(tr.names),
               opt_bytes=nbytes, opt_gbs=nbytes / (hip_kern * 1e-3) / 1e9, eager_ms=None, eager_opt_ms=None, eager_over_hip=None,
               eager_opt_over_hip=None)
    if a.no_eager:
        return row
    net = tr.online_model
    p = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    ema = {k: v.detach().clone() for k, v in p.items()}
    freqs = net.time_mlp.freqs
    opt = torch.optim.Adam(list(p.values()), lr=LR, betas=BETAS)
    sab, s1m, lw = gd.sqrt_alphas_cumprod[t], gd.sqrt_one_minus_alphas_cumprod[t], gd.loss_weight[t]
    ext = (slice(None), None, None, None)

    def eager_opt():
        torch.nn.utils.clip_grad_norm_(list(p.values()), MAX_NORM)
        opt.step()
        with torch.no_grad():
            for k, e in ema.items():
                e.lerp_(p[k], EMA_W)

    def eager_step():
        opt.zero_grad()
        x = sab[ext] * hr + s1m[ext] * noise
        out = U.eager_unet(p, cfg, freqs, x, lr, t)
        target = sab[ext] * noise - s1m[ext] * hr
        loss = (((out - target) ** 2).reshape(B, -1).mean(dim=1) * lw).mean()
        loss.backward()
        eager_opt()

    row["eager_ms"] = grad_bench.time_ms(eager_step, a.iters, a.warmup)
    row["eager_opt_ms"] = grad_bench.time_ms(eager_opt, a.iters, a.warmup)
    row["eager_over_hip"] = row["eager_ms"] / hip
    row["eager_opt_over_hip"] = row["eager_opt_ms"] / hip_opt
    return row


def report(r):
    eg = ""
    if r["eager_ms"] is not None:
        eg = (f"; eager PyTorch step {r['eager_ms']:9.3f} ms ({r['eager_over_hip']:.2f} x), clip + Adam + EMA "
              f"{r['eager_opt_ms']:8.3f} ms ({r['eager_opt_over_hip']:.1f} x)")
    print(f"{r['data']:5s} @{r['H']:3d}^2 B={r['B']:<2d} {r['conv_precision']} / act {r['act_storage']} / conv out {r['conv_out_storage']} / attn {r['attn_precision']} / full attn {r['full_attn_precision']}{grad_bench.amp_tag(r)}: HIP step {r['hip_ms']:9.3f} ms, peak "
          f"{r['peak_mb']:8.1f} MiB, apply() {r['hip_opt_ms']:7.3f} ms (its 3 "
          f"launches {1e3 * r['hip_opt_kernels_ms']:6.1f} us) over {r['tensors']} tensors / {r['params'] / 1e6:.1f} M floats = "
          f"{r['opt_gbs']:7.1f} GB/s ({100 * r['opt_gbs'] / grad_bench.HBM_PEAK_GBS:.1f} % of {grad_bench.HBM_PEAK_GBS:.0f}){eg}")


if __name__ == "__main__":
    sys.exit(grad_bench.main(__file__, U.CASES, run_case, report, switches=U.SWITCHES, amp=True, amp_attn=True))
