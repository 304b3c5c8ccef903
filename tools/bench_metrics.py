#!/usr/bin/env python3
"""Times the quality-metric kernel (``metrics.quality_sums``, csrc/metrics.hip) against the same sums in eager PyTorch on the
same GPU, and one sharded against one unsharded evaluation of a small test set.

  python tools/bench_metrics.py [--iters 20] [--warmup 3] [--no-eval]
``hip`` is the whole ``quality_sums`` call (two launches and its two allocations), ``torch`` the restatement: the five
moments through separable fp32 ``F.conv2d`` (1 x 11, then 11 x 1), the SSIM map, and the region sums in fp64; both timed with
events around the call, median of ``iters`` after ``warmup`` calls, with a region mask.  The evaluation: the MNIST-sized
denoiser of the tests (procedural weights), T = 4, test batches of 3 and 2 images; ``DenoiserTrainer.evaluate`` unsharded and
``sharded=True`` at world 1 -- the overhead of the new path where it cannot help (on one GPU there is nothing to shard: the
saving of a multi-GPU run is not measured by this tool).  Prints one line per case and a JSON list at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import metrics_ref as R                                             # noqa: E402
import localdiffusion_hallucination_amd as ldh                      # noqa: E402
from localdiffusion_hallucination_amd import metrics, rng, weights  # noqa: E402

SHAPES = [(8, 3, 256, 256), (1, 1, 512, 512)]
KWARGS = dict(dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist")


def time_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(iters):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(times))


def torch_sums(pred, ref, mask, L):
    """The [B, 3, 4] table in eager PyTorch on the device: separable fp32 convolutions, fp64 sums."""
    B, C, H, W = pred.shape
    t = torch.from_numpy(R.taps32()).to(pred.device)
    kh, kv = t.view(1, 1, 1, -1), t.view(1, 1, -1, 1)

    def blur(a):
        return F.conv2d(F.conv2d(a.reshape(B * C, 1, H, W), kh), kv).reshape(B, C, H - 10, W - 10)
    mx, my, exx, eyy, exy = blur(pred), blur(ref), blur(pred * pred), blur(ref * ref), blur(pred * ref)
    c1, c2 = R.constants(L)
    sx, sy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    s = (((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sx + sy + c2))).double()
    d = (pred - ref).double()
    sq = d * d
    ood = mask >= 1.0
    rows = []
    for m in (torch.ones_like(ood), ood, ~ood):
        mc = m[:, :, 5:H - 5, 5:W - 5]
        rows.append(torch.stack([m.sum(dim=(1, 2, 3)).double() * C, (sq * m).sum(dim=(1, 2, 3)),
                                 mc.sum(dim=(1, 2, 3)).double() * C, (s * mc).sum(dim=(1, 2, 3))], dim=1))
    return torch.stack(rows, dim=1)


def bench_kernel(shape, L, iters, warmup):
    pred, ref = (x.cuda() for x in R.images(shape, L))
    mask = R.make_mask("rect", shape).cuda()
    hip = time_ms(lambda: metrics.quality_sums(pred, ref, mask, data_range=L), iters, warmup)

    def eager():
        return torch_sums(pred, ref, mask, L)
    tor = time_ms(eager, iters, warmup)
    got, want = metrics.quality_sums(pred, ref, mask, data_range=L).cpu(), eager().cpu()
    d = float((R.per_image_ssim(got) - R.per_image_ssim(want)).abs().max())
    return dict(case="kernel", shape=list(shape), hip_ms=hip, torch_ms=tor, ssim_distance_to_torch=d)


def bench_eval(iters, warmup):
    net = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **KWARGS)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_state_dict(net.cfg, 0).items()})
    config = dict(branch_out=False, start_intermediate=False, start_timestep=2, data="mnist", mask_x=False, ood_AD=False,
                  ood_confidence=False, classifier=False, use_gt=False)
    gd = ldh.GaussianDiffusion(config, net, image_size=28, timesteps=4, objective="pred_v").to("cuda")
    tr = ldh.DenoiserTrainer(gd)
    hr = torch.from_numpy(rng.uniform((5, 1, 28, 28), 7, 1, 0.0, 1.0)).cuda()
    lr = torch.from_numpy(rng.uniform((5, 1, 28, 28), 7, 2, 0.0, 1.0)).cuda()
    batches = [(hr[:3], lr[:3]), (hr[3:], lr[3:])]

    def wall(fn):
        for _ in range(warmup):
            fn()
        times = []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times))
    plain = wall(lambda: tr.evaluate(batches, (0.0, 1.0)))
    shard = wall(lambda: tr.evaluate(batches, (0.0, 1.0), sharded=True))
    a, b = tr.evaluate(batches, (0.0, 1.0)), tr.evaluate(batches, (0.0, 1.0), sharded=True)
    return dict(case="evaluate", batches=[3, 2], timesteps=4, unsharded_ms=plain, sharded_world1_ms=shard, unsharded_loss=a,
                sharded_loss=b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eval", action="store_true")
    a = ap.parse_args()
    ldh.configure_runtime()
    rows = []
    for shape in SHAPES:
        r = bench_kernel(shape, 2.0, a.iters, a.warmup)
        print(f"quality_sums {tuple(shape)}: hip {r['hip_ms']:.4f} ms, torch {r['torch_ms']:.4f} ms "
              f"({r['torch_ms'] / r['hip_ms']:.1f}x), per-image SSIM distance to torch {r['ssim_distance_to_torch']:.2e}")
        rows.append(r)
    if not a.no_eval:
        r = bench_eval(a.iters, a.warmup)
        print(f"evaluate, batches of 3 and 2 at 28^2, T = 4: unsharded {r['unsharded_ms']:.3f} ms, sharded at world 1 "
              f"{r['sharded_world1_ms']:.3f} ms; losses {r['unsharded_loss']!r} / {r['sharded_loss']!r}")
        rows.append(r)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
