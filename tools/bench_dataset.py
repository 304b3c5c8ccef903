#!/usr/bin/env python3
"""Times the device-resident data path (``DeviceDataset.batch``, csrc/dataset.hip) with augmentation on: ms per batch for
mnist 28^2 B = 64, SR 112^2 x 3 B = 32 and mri 256 -> 224 B = 32, against the same transform in eager PyTorch on the same GPU
(batched: ``grid_sample(mode="nearest")`` on torchvision's affine grid, ``torch.where`` for the flips, ``F.interpolate``) and
against the per-sample host restatement of the reference's ``__getitem__`` (tests/dataset_ref.py) on 16 CPU threads.

  python tools/bench_dataset.py [--iters 20] [--warmup 5] [--no-eager] [--no-host]
One process.  ``hip call`` is the whole ``batch()`` call (table build, pinned upload, launch) timed with events around it,
median of ``iters``; ``hip kernels`` is the launches alone (the library's per-launch timing session) and gives the GB/s,
counted over the bytes WRITTEN (hr and lr, fp32).  The random angles are not screened for rotation ties, so each line also
counts the pixels at which hr or lr differs from the host restatement (any bit; the SR lr beyond 1e-6): a source coordinate
within fp32 rounding of a half-integer picks the neighbouring pixel.  Prints one line per case and a JSON list at the end.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import dataset_ref as D                                             # noqa: E402
import localdiffusion_hallucination_amd as ldh                      # noqa: E402
from localdiffusion_hallucination_amd import _cabi as cabi         # noqa: E402
from localdiffusion_hallucination_amd import rng                   # noqa: E402
from localdiffusion_hallucination_amd.dataset import DeviceDataset, cos_sin, crop_offset     # noqa: E402

MRI_KW = dict(mean_target=412.7, std_target=151.3, mean_cond=388.1, std_cond=97.6, translate_zero=True, crop=224)
HOST_THREADS = 16


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


def kernel_ms(fn, iters):
    """Median over ``iters`` calls of the summed execution time of the call's launches."""
    lib, out = cabi.lib(), []
    for _ in range(iters):
        cabi.check(lib.ld_timing_begin(8), "timing_begin")
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            n = max(1, lib.ld_timing_count())
            ms, cnt = (C.c_float * n)(), C.c_int()
            rc = lib.ld_timing_end(ms, n, C.byref(cnt))
        cabi.check(rc, "timing_end")
        out.append(float(sum(ms[:cnt.value])))
    return float(np.median(out))


def eager_augment(x, cs, flips):
    """x [B, C, H, W] on the GPU, cs [B, 2] (cos, sin), flips [B] bool: rotation (torchvision's grid) and flip, batched."""
    B, _, H, W = x.shape
    theta = torch.stack([torch.stack([cs[:, 0], -cs[:, 1], torch.zeros_like(cs[:, 0])], 1),
                         torch.stack([cs[:, 1], cs[:, 0], torch.zeros_like(cs[:, 0])], 1)], 1)          # [B, 2, 3]
    base = torch.empty(1, H, W, 3, device=x.device)
    base[..., 0].copy_(torch.linspace(-W * 0.5 + 0.5, W * 0.5 - 0.5, steps=W, device=x.device))
    base[..., 1].copy_(torch.linspace(-H * 0.5 + 0.5, H * 0.5 - 0.5, steps=H, device=x.device).unsqueeze(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * W, 0.5 * H], device=x.device)
    grid = base.view(1, H * W, 3).expand(B, H * W, 3).bmm(rescaled).view(B, H, W, 2)
    x = F.grid_sample(x, grid, mode="nearest", padding_mode="zeros", align_corners=False)
    return torch.where(flips[:, None, None, None], x.flip(-2), x)


def eager_batch(kind, stores, idx, cs, flips):
    if kind == "mnist":
        x = eager_augment(stores[0][idx][:, None].float(), cs, flips)
        S = x.shape[-1]
        down = F.interpolate(x[:, :, ::2, :], size=(S, S), mode="bilinear", align_corners=False)
        return 2 * (x / 255.0), 2 * (down / 255.0)
    if kind == "sr":
        x = eager_augment(stores[0][idx].float() / 255, cs, flips) * 2
        S = x.shape[-1]
        down = F.interpolate(F.interpolate(x, size=(S // 2, S // 2), mode="nearest"), size=(S, S), mode="bilinear", align_corners=False)
        return x, down
    out, top, crop = [], crop_offset(stores[0].shape[-1], MRI_KW["crop"]), MRI_KW["crop"]
    for s, mean, std in ((stores[0], MRI_KW["mean_target"], MRI_KW["std_target"]), (stores[1], MRI_KW["mean_cond"], MRI_KW["std_cond"])):
        x = eager_augment(s[idx][:, None, top:top + crop, top:top + crop], cs, flips)
        x = (x - mean) / std
        out.append(x + x.amin(dim=(1, 2, 3), keepdim=True).abs())
    return tuple(out)


def host_batch(kind, stores, idx, angles, flips, pool):
    if kind == "mnist":
        items = pool.map(lambda a: D.mnist_item(stores[0][a[0]], a[1], bool(a[2])), zip(idx, angles, flips))
    elif kind == "sr":
        items = pool.map(lambda a: D.sr_item(stores[0][a[0]], a[1], bool(a[2])), zip(idx, angles, flips))
    else:
        items = pool.map(lambda a: D.mri_item(stores[0][a[0]], stores[1][a[0]], angle_deg=a[1], flip=bool(a[2]), **MRI_KW),
                         zip(idx, angles, flips))
    items = list(items)
    return torch.stack([h for h, _ in items]), torch.stack([l for _, l in items])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    ldh.configure_runtime()
    torch.set_num_threads(1)                                       # the host path's parallelism is its 16 worker threads

    def u8(shape, key):
        return (rng.bits64(int(np.prod(shape)), 5, key) >> np.uint64(56)).astype(np.uint8).reshape(shape)
    cases = [("mnist", 64, (u8((200, 28, 28), 1),), lambda s: DeviceDataset.mnist(s[0], augmentations=True)),
             ("sr", 32, (u8((256, 3, 112, 112), 2),), lambda s: DeviceDataset.sr(s[0], augmentations=True)),
             ("mri", 32, (rng.uniform((256, 256, 256), 5, 3, 0.0, 4096.0), rng.uniform((256, 256, 256), 5, 4, 0.0, 4096.0)),
              lambda s: DeviceDataset.mri(s[0], s[1], augmentations=True, **MRI_KW))]
    rows = []
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        for kind, B, stores, make in cases:
            ds = make(stores)
            n = len(ds)
            idx = np.argsort(rng.bits64(n, 5, 10), kind="stable")[:B]
            angles = rng.uniform((B,), 5, 11, -15.0, 15.0).astype(np.float64)
            flips = (rng.bits64(B, 5, 12) >> np.uint64(63)) != 0
            hr, lr = ds.batch(idx, angles, flips)
            written = 2 * hr.numel() * 4
            call = time_ms(lambda: ds.batch(idx, angles, flips), a.iters, a.warmup)
            kern = kernel_ms(lambda: ds.batch(idx, angles, flips), a.iters)
            row = dict(data=kind, B=B, shape=list(hr.shape), hip_call_ms=call, hip_kernels_ms=kern,
                       gbps_written=written / (kern * 1e-3) / 1e9, eager_ms=None, host_ms=None, max_abs_diff_vs_eager=None)
            if not a.no_eager:
                dev_stores = tuple(torch.from_numpy(s).cuda() for s in stores)
                didx = torch.from_numpy(idx).cuda()
                cs = torch.tensor([[float(c), float(s)] for c, s in map(cos_sin, angles)], device="cuda")
                dfl = torch.from_numpy(flips).cuda()
                row["eager_ms"] = time_ms(lambda: eager_batch(kind, dev_stores, didx, cs, dfl), a.iters, a.warmup)
                ehr, elr = eager_batch(kind, dev_stores, didx, cs, dfl)
                # (random angles are not screened for rotation ties: a few pixels may come from a neighbouring source)
                row["max_abs_diff_vs_eager"] = max(float((ehr - hr).abs().max()), float((elr - lr).abs().max()))
                row["frac_equal_vs_eager"] = float(((ehr == hr) & (elr == lr)).float().mean())
            if not a.no_host:
                hhr, hlr = host_batch(kind, stores, idx, angles, flips, pool)
                # (fp64 rotation against the kernel's fp32: unscreened angles may disagree at a handful of rotation ties)
                same = (hhr == hr.cpu()) & ((hlr - lr.cpu()).abs() <= (1e-6 if kind == "sr" else 0.0))
                row["values_differing_vs_host"] = int((~same).sum())
                times = []
                for _ in range(max(3, a.iters // 4)):
                    t0 = time.perf_counter()
                    host_batch(kind, stores, idx, angles, flips, pool)
                    times.append(1e3 * (time.perf_counter() - t0))
                row["host_ms"] = float(np.median(times))
            rows.append(row)
            fmt = lambda v: "      -" if v is None else f"{v:7.3f}"                      # noqa: E731
            print(f"{kind:5s} B={B:2d} {tuple(hr.shape)}: hip call {call:7.3f} ms, kernels {kern:7.4f} ms "
                  f"({row['gbps_written']:.1f} GB/s written), eager torch {fmt(row['eager_ms'])} ms, host x{HOST_THREADS} "
                  f"{fmt(row['host_ms'])} ms ({row.get('values_differing_vs_host')} of {hr.numel()} pixels differ from it)", flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
