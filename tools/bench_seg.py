#!/usr/bin/env python3
"""Times the segmentation U-Net alone (the OOD-mask producer, unet_model.py:140-243): SegUNet on the HIP kernels against
the same network as eager PyTorch on the same GPU, ms per image, for each size / batch / storage dtype.

  python tools/bench_seg.py [--sizes 256,512] [--batches 1,8] [--dtypes fp32,bf16,fp16] [--iters 20] [--warmup 5]
Prints one line per case and a JSON list at the end.  The eager leg runs torch's own modules (conv2d / batch_norm /
max_pool2d / conv_transpose2d on MIOpen) in the matching dtype, channels-first, in eval mode under no_grad.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import localdiffusion_hallucination_amd as ldh                    # noqa: E402
from localdiffusion_hallucination_amd import weights             # noqa: E402

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def eager_forward(sd, x):
    """The network op by op in eager PyTorch (the comparison leg)."""
    def dconv(p, h):
        for i in (0, 3):
            h = F.conv2d(h, sd[f"{p}double_conv.{i}.weight"], padding=1)
            bn = f"{p}double_conv.{i + 1}."
            h = F.relu(F.batch_norm(h, sd[bn + "running_mean"], sd[bn + "running_var"], sd[bn + "weight"], sd[bn + "bias"],
                                    training=False, eps=1e-5))
        return h
    skips = [dconv("inc.", x)]
    for i in range(1, 5):
        skips.append(dconv(f"down{i}.maxpool_conv.1.", F.max_pool2d(skips[-1], 2)))
    h = skips[-1]
    for i in range(1, 5):
        up = F.conv_transpose2d(h, sd[f"up{i}.up.weight"], sd[f"up{i}.up.bias"], stride=2)
        h = dconv(f"up{i}.conv.", torch.cat([skips[4 - i], up], dim=1))
    return F.conv2d(h, sd["outc.conv.weight"], sd["outc.conv.bias"])


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--dtypes", default="fp32,bf16,fp16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    ldh.configure_runtime()
    sd_np = weights.procedural_seg_state_dict(0)
    net = ldh.SegUNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()})
    net = net.cuda().eval()
    rows = []
    for dt in a.dtypes.split(","):
        net.set_compute_dtype(dt)
        sd = {k: torch.from_numpy(np.asarray(v)).cuda().to(TDT[dt] if v.dtype == np.float32 else torch.int64)
              for k, v in sd_np.items()}
        for H in (int(s) for s in a.sizes.split(",")):
            for B in (int(b) for b in a.batches.split(",")):
                x = torch.randn(B, 1, H, H, device="cuda")
                xe = x.to(TDT[dt])
                with torch.no_grad():
                    hip = time_ms(lambda: net(x), a.iters, a.warmup)
                    eager = time_ms(lambda: eager_forward(sd, xe), a.iters, a.warmup)
                net.invalidate()                      # free this shape's activations before the next one
                torch.cuda.empty_cache()
                row = dict(dtype=dt, H=H, B=B, hip_ms_per_image=hip / B, eager_ms_per_image=eager / B,
                           eager_over_hip=eager / hip)
                rows.append(row)
                print(f"{dt:5s} {H:4d}^2 B={B}: HIP {hip / B:8.3f} ms/image   eager PyTorch {eager / B:8.3f} ms/image   "
                      f"(eager / HIP = {eager / hip:.2f})", flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
