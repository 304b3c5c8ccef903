#!/usr/bin/env python3
"""Times one training step of the segmentation U-Net (train_seg.py:78-95): SegTrainer.step on the HIP kernels against the
same step in eager PyTorch (autograd + torch.optim.Adam, MIOpen convolutions) on the same GPU, fp32, ms per step.

  python tools/bench_segtrain.py [--sizes 128,256] [--batches 8,32] [--iters 10] [--warmup 3] [--no-eager]
One process; per case a warm-up, then the median of ``iters`` steps timed with events around the whole step.  Then one
more HIP step under the library's per-launch timing session gives the split of the step over its kernels and the
weight-gradient kernel's TFLOP/s (of the 157 TFLOP/s exact-f32 MFMA peak).  Prints one line per case, the split, and a
JSON list at the end.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import localdiffusion_hallucination_amd as ldh                    # noqa: E402
from localdiffusion_hallucination_amd import _cabi as cabi       # noqa: E402
from localdiffusion_hallucination_amd import segtrain, weights   # noqa: E402

F32_MFMA_PEAK_TFLOPS = 157.0


def eager_forward(p, bufs, x):
    def dconv(pre, h):
        for i in (0, 3):
            h = F.conv2d(h, p[f"{pre}double_conv.{i}.weight"], padding=1)
            bn = f"{pre}double_conv.{i + 1}."
            h = F.relu(F.batch_norm(h, bufs[bn + "running_mean"], bufs[bn + "running_var"], p[bn + "weight"], p[bn + "bias"],
                                    training=True, momentum=0.1, eps=1e-5))
        return h
    skips = [dconv("inc.", x)]
    for i in range(1, 5):
        skips.append(dconv(f"down{i}.maxpool_conv.1.", F.max_pool2d(skips[-1], 2)))
    h = skips[-1]
    for i in range(1, 5):
        up = F.conv_transpose2d(h, p[f"up{i}.up.weight"], p[f"up{i}.up.bias"], stride=2)
        h = dconv(f"up{i}.conv.", torch.cat([skips[4 - i], up], dim=1))
    return F.conv2d(h, p["outc.conv.weight"], p["outc.conv.bias"])


def eager_stepper(sd_np):
    p, bufs = {}, {}
    for k, v in sd_np.items():
        t = torch.from_numpy(np.asarray(v)).cuda()
        if "running_" in k:
            bufs[k] = t
        elif not k.endswith("num_batches_tracked"):
            p[k] = t.requires_grad_(True)
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)
    pw = torch.tensor([10.0], device="cuda")

    def step(x, t):
        opt.zero_grad(set_to_none=True)
        z = eager_forward(p, bufs, x)
        pr = torch.sigmoid(z).view(-1)
        tt = t.view(-1)
        loss = F.binary_cross_entropy_with_logits(z, t, pos_weight=pw) + \
            (1.0 - (2.0 * (pr * tt).sum() + 1e-5) / (pr.sum() + tt.sum() + 1e-5))
        loss.backward()
        opt.step()
        return loss
    return step


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


class _TimedLib:
    """The library with every entry point's launches attributed to a label (forward / backward told apart by ld_seg_loss)."""

    def __init__(self, lib):
        self._lib, self.calls, self.phase, self.wgrad_flop = lib, [], "forward", 0.0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(("ld_seg_", "ld_pc_conv")) or name == "ld_seg_wgrad_splits":
            return fn

        def wrapped(*args):
            if name == "ld_seg_loss":
                self.phase = "backward"
            label = name[3:]
            if name == "ld_pc_conv":
                label = "pc_conv (forward)" if self.phase == "forward" else "pc_conv (data gradient)"
            if name == "ld_seg_wgrad":
                B, H, W, cin, cout, ks = args[4:10]
                self.wgrad_flop += 2.0 * B * H * W * cin * cout * ks * ks
            n0 = self._lib.ld_timing_count()
            rc = fn(*args)
            self.calls.append((label, n0, self._lib.ld_timing_count()))
            return rc
        return wrapped


def kernel_split(trainer, x, t):
    lib = cabi.lib()
    timed = _TimedLib(lib)
    real = segtrain.cabi.lib
    cabi.check(lib.ld_timing_begin(4096), "timing_begin")
    try:
        segtrain.cabi.lib = lambda: timed
        trainer.step(x, t)
        torch.cuda.synchronize()
    finally:
        segtrain.cabi.lib = real
        n = max(1, lib.ld_timing_count())
        ms, cnt = (C.c_float * n)(), C.c_int()
        rc = lib.ld_timing_end(ms, n, C.byref(cnt))
    cabi.check(rc, "timing_end")
    split = {}
    for label, a, b in timed.calls:
        e = split.setdefault(label, [0.0, 0])
        e[0] += float(sum(ms[a:b]))
        e[1] += b - a
    return split, timed.wgrad_flop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    ldh.configure_runtime()
    sd_np = weights.procedural_seg_state_dict(0)
    rows = []
    for H in (int(s) for s in a.sizes.split(",")):
        for B in (int(b) for b in a.batches.split(",")):
            x = torch.randn(B, 1, H, H, device="cuda")
            t = (torch.rand(B, 1, H, H, device="cuda") < 0.03).float()
            net = ldh.SegUNet()
            net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()})
            net = net.cuda().train()
            trainer = ldh.SegTrainer(net)
            hip = time_ms(lambda: trainer.step(x, t), a.iters, a.warmup)
            split, flop = kernel_split(trainer, x, t)
            del trainer, net
            torch.cuda.empty_cache()
            eager = None
            if not a.no_eager:
                step = eager_stepper(sd_np)
                eager = time_ms(lambda: step(x, t), a.iters, a.warmup)
                del step
                torch.cuda.empty_cache()
            kernels_ms = sum(v[0] for v in split.values())
            wg_ms = split.get("seg_wgrad", [0.0, 0])[0]
            row = dict(H=H, B=B, hip_ms_per_step=hip, eager_ms_per_step=eager, eager_over_hip=(eager / hip if eager else None),
                       kernels_ms=kernels_ms, wgrad_ms=wg_ms, wgrad_tflops=flop / (wg_ms * 1e9) if wg_ms else None,
                       split={k: dict(ms=v[0], launches=v[1]) for k, v in split.items()})
            rows.append(row)
            eg = f"eager PyTorch {eager:9.2f} ms/step   (eager / HIP = {eager / hip:.2f})" if eager else ""
            print(f"{H:4d}^2 B={B:2d}: HIP {hip:9.2f} ms/step   {eg}", flush=True)
            for k, v in sorted(split.items(), key=lambda kv: -kv[1][0]):
                print(f"      {k:28s} {v[0]:9.3f} ms  {100 * v[0] / kernels_ms:5.1f} %  ({v[1]} launches)")
            if wg_ms:
                tf = flop / (wg_ms * 1e9)
                print(f"      weight gradient: {flop / 1e12:.2f} TFLOP in {wg_ms:.2f} ms = {tf:.1f} TFLOP/s "
                      f"({100 * tf / F32_MFMA_PEAK_TFLOPS:.0f} % of the {F32_MFMA_PEAK_TFLOPS:.0f} TFLOP/s f32 peak)", flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
