#!/usr/bin/env python3
"""Times the MNIST digit classifier: one training step (MnistClassifierTrainer.step) and one forward on the HIP kernels
against the same in eager PyTorch (autograd + torch.optim.Adam, MIOpen convolutions) on the same GPU, fp32, ms.

  python tools/bench_mnistcls.py [--batches 64,512] [--iters 10] [--warmup 3] [--no-eager]
One process; per case a warm-up, then the median of ``iters`` calls timed with events around the whole call.  Then one
more HIP step under the library's per-launch timing session gives the split of the step over its kernels.  Prints one line
per case, the split, and a JSON list at the end.
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
from localdiffusion_hallucination_amd import mnistcls, weights   # noqa: E402


def eager_forward(p, x):
    h = F.max_pool2d(F.relu(F.conv2d(x, p["conv1.weight"], p["conv1.bias"], padding=1)), 2)
    h = F.max_pool2d(F.relu(F.conv2d(h, p["conv2.weight"], p["conv2.bias"], padding=1)), 2)
    h = F.relu(F.linear(h.view(-1, 64 * 7 * 7), p["fc1.weight"], p["fc1.bias"]))
    return F.linear(h, p["fc2.weight"], p["fc2.bias"])


def eager(sd_np):
    p = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in sd_np.items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-3)

    def step(x, y):
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(eager_forward(p, x), y)
        loss.backward()
        opt.step()
        return loss

    def forward(x):
        with torch.no_grad():
            return eager_forward(p, x)
    return step, forward


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
    """The library with every entry point's launches attributed to a label (the pc_conv launches told apart by order)."""

    def __init__(self, lib):
        self._lib, self.calls, self.n_conv, self.n_gemm = lib, [], 0, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(("ld_mc_", "ld_seg_", "ld_pc_conv")) or name.endswith(("_splits", "_work_floats")):
            return fn

        def wrapped(*args):
            label = name[3:]
            if name == "ld_pc_conv":
                label = ("conv2 forward (pc_conv)", "conv2 data gradient (pc_conv)")[min(self.n_conv, 1)]
                self.n_conv += 1
            if name == "ld_mc_gemm":
                label = ("fc1 forward (mc_gemm)", "fc1 weight gradient (mc_gemm)", "fc1 data gradient (mc_gemm)")[min(self.n_gemm, 2)]
                self.n_gemm += 1
            n0 = self._lib.ld_timing_count()
            rc = fn(*args)
            self.calls.append((label, n0, self._lib.ld_timing_count()))
            return rc
        return wrapped


def kernel_split(trainer, x, y):
    lib = cabi.lib()
    timed = _TimedLib(lib)
    real = mnistcls.cabi.lib
    cabi.check(lib.ld_timing_begin(256), "timing_begin")
    try:
        mnistcls.cabi.lib = lambda: timed
        trainer.step(x, y)
        torch.cuda.synchronize()
    finally:
        mnistcls.cabi.lib = real
        n = max(1, lib.ld_timing_count())
        ms, cnt = (C.c_float * n)(), C.c_int()
        rc = lib.ld_timing_end(ms, n, C.byref(cnt))
    cabi.check(rc, "timing_end")
    split = {}
    for label, a, b in timed.calls:
        e = split.setdefault(label, [0.0, 0])
        e[0] += float(sum(ms[a:b]))
        e[1] += b - a
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,512")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    ldh.configure_runtime()
    sd_np = weights.procedural_mnistcls_state_dict(0)
    rows = []
    for B in (int(b) for b in a.batches.split(",")):
        x = 2.0 * torch.rand(B, 1, 28, 28, device="cuda")
        y = torch.randint(0, 10, (B,), device="cuda")
        net = ldh.MnistClassifier()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
        net = net.cuda()
        trainer = ldh.MnistClassifierTrainer(net)
        hip_step = time_ms(lambda: trainer.step(x, y), a.iters, a.warmup)
        hip_fwd = time_ms(lambda: net(x), a.iters, a.warmup)
        split = kernel_split(trainer, x, y)
        eager_step = eager_fwd = None
        if not a.no_eager:
            step, forward = eager(sd_np)
            eager_step = time_ms(lambda: step(x, y), a.iters, a.warmup)
            eager_fwd = time_ms(lambda: forward(x), a.iters, a.warmup)
        kernels_ms = sum(v[0] for v in split.values())
        rows.append(dict(B=B, hip_ms_per_step=hip_step, eager_ms_per_step=eager_step, hip_ms_per_forward=hip_fwd,
                         eager_ms_per_forward=eager_fwd, kernels_ms=kernels_ms, launches=sum(v[1] for v in split.values()),
                         split={k: dict(ms=v[0], launches=v[1]) for k, v in split.items()}))
        eg = f"   eager PyTorch {eager_step:7.3f} / {eager_fwd:7.3f}" if eager_step else ""
        print(f"B={B:4d}: HIP step {hip_step:7.3f} ms, forward {hip_fwd:7.3f} ms{eg}", flush=True)
        for k, v in sorted(split.items(), key=lambda kv: -kv[1][0]):
            print(f"      {k:34s} {v[0]:8.4f} ms  {100 * v[0] / kernels_ms:5.1f} %  ({v[1]} launches)")
        print(f"      kernels {kernels_ms:.4f} ms in {rows[-1]['launches']} launches", flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
