#!/usr/bin/env python3
"""Times forward + backward of one trainable ResnetBlock: ``ldh.ResnetBlock`` on the HIP kernels against the same block
restated in eager PyTorch (autograd, MIOpen convolutions) on the same GPU in one process, fp32, ms per forward + backward.

  python tools/bench_resblock_grad.py [--batch 8] [--iters 20] [--warmup 3] [--cases 32:256,64:128,128:64,256:32]
The default cases are cfg3's four levels (dim -> dim at H = W).  Per case: 3 warm-up calls, then the median of 20 calls
timed with events around forward + backward.  The HIP block reads x and the upstream gradient in channels_last (its own
layout; a channel count that is not a multiple of 64 is repacked with padding either way); eager PyTorch is timed in both
memory formats.  One more HIP call under the library's per-launch timing session gives the split of the time over the
entry points, and the achieved bandwidth of the two GroupNorm-backward passes against 8 TB/s (bytes: dout and y read by
each pass, dy written once; padded channels are written but never read).  Prints one line per case, the split, and a JSON
list at the end.
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
from localdiffusion_hallucination_amd import resblock             # noqa: E402

HBM_PEAK_GBS = 8000.0
TIME_DIM = 128


def eager_block(p, x, temb, groups=8):
    e = F.linear(F.silu(temb), p["mlp.1.weight"], p["mlp.1.bias"])[:, :, None, None]
    scale, shift = e.chunk(2, dim=1)
    h = F.conv2d(x, p["block1.proj.weight"], p["block1.proj.bias"], padding=1)
    h = F.silu(F.group_norm(h, groups, p["block1.norm.weight"], p["block1.norm.bias"], eps=1e-5) * (scale + 1) + shift)
    h = F.conv2d(h, p["block2.proj.weight"], p["block2.proj.bias"], padding=1)
    h = F.silu(F.group_norm(h, groups, p["block2.norm.weight"], p["block2.norm.bias"], eps=1e-5))
    if "res_conv.weight" in p:
        x = F.conv2d(x, p["res_conv.weight"], p["res_conv.bias"])
    return h + x


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
    """The library with the launches of every entry point attributed to a label; forward and backward are told apart by
    ``phase``, and the three launches of ld_dn_gn_backward (sums, finalisation, dy) are kept apart."""

    def __init__(self, lib):
        self._lib, self.calls, self.phase = lib, [], "forward"

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(("ld_dn_", "ld_seg_", "ld_pc_conv")) or name in ("ld_seg_wgrad_splits", "ld_dn_gn_work_bytes"):
            return fn

        def wrapped(*args):
            label = name[3:]
            if name == "ld_pc_conv":
                label = "pc_conv (forward)" if self.phase == "forward" else "pc_conv (data gradient)"
            if name == "ld_dn_pack_nhwc":
                label = f"dn_pack_nhwc ({self.phase})"
            n0 = self._lib.ld_timing_count()
            rc = fn(*args)
            self.calls.append((label, n0, self._lib.ld_timing_count()))
            return rc
        return wrapped


def kernel_split(run):
    """run(set_phase) does one forward + backward; returns {label: [ms, launches]} and the GroupNorm-backward pass times."""
    lib = cabi.lib()
    timed = _TimedLib(lib)
    real = resblock.cabi.lib
    cabi.check(lib.ld_timing_begin(4096), "timing_begin")
    try:
        resblock.cabi.lib = lambda: timed
        run(lambda phase: setattr(timed, "phase", phase))
        torch.cuda.synchronize()
    finally:
        resblock.cabi.lib = real
        n = max(1, lib.ld_timing_count())
        ms, cnt = (C.c_float * n)(), C.c_int()
        rc = lib.ld_timing_end(ms, n, C.byref(cnt))
    cabi.check(rc, "timing_end")
    split, gn_pass_ms = {}, 0.0
    for label, a, b in timed.calls:
        e = split.setdefault(label, [0.0, 0])
        e[0] += float(sum(ms[a:b]))
        e[1] += b - a
        if label == "dn_gn_backward" and b - a == 3:
            gn_pass_ms += float(ms[a]) + float(ms[a + 2])
    return split, gn_pass_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="32:256,64:128,128:64,256:32")
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    ldh.configure_runtime()
    B, rows = a.batch, []
    for case in a.cases.split(","):
        dim, H = (int(v) for v in case.split(":"))
        torch.manual_seed(0)
        blk = ldh.ResnetBlock(dim, dim, time_emb_dim=TIME_DIM).cuda()
        x = torch.randn(B, dim, H, H, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
        temb = torch.randn(B, TIME_DIM, device="cuda").requires_grad_(True)
        dout = (torch.randn(B, dim, H, H, device="cuda") / (B * H * H)).contiguous(memory_format=torch.channels_last)

        def hip_step(set_phase=None):
            blk.zero_grad(set_to_none=True)
            x.grad = temb.grad = None
            out = blk(x, temb)
            if set_phase:
                set_phase("backward")
            out.backward(dout)

        hip = time_ms(hip_step, a.iters, a.warmup)
        split, gn_pass_ms = kernel_split(hip_step)
        kernels_ms = sum(v[0] for v in split.values())
        # two GroupNorms x (dout and y read by each of the two passes: the real channels; dy written: the padded pixel)
        gn_bytes = 2 * (4 * dim + blk.cop) * B * H * H * 4
        gn_gbs = gn_bytes / (gn_pass_ms * 1e6) if gn_pass_ms else None
        eager = {}
        if not a.no_eager:
            p = {k: v.detach().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
            for fmt, name in ((torch.contiguous_format, "nchw"), (torch.channels_last, "nhwc")):
                xe = x.detach().contiguous(memory_format=fmt).requires_grad_(True)
                te = temb.detach().clone().requires_grad_(True)
                de = dout.contiguous(memory_format=fmt)

                def eager_step():
                    for v in p.values():
                        v.grad = None
                    xe.grad = te.grad = None
                    eager_block(p, xe, te).backward(de)

                eager[name] = time_ms(eager_step, a.iters, a.warmup)
        best = min(eager.values()) if eager else None
        rows.append(dict(dim=dim, H=H, B=B, hip_ms=hip, eager_nchw_ms=eager.get("nchw"), eager_nhwc_ms=eager.get("nhwc"),
                         eager_over_hip=(best / hip if best else None), kernels_ms=kernels_ms, gn_backward_passes_ms=gn_pass_ms,
                         gn_backward_gbs=gn_gbs, split={k: dict(ms=v[0], launches=v[1]) for k, v in split.items()}))
        eg = "" if not eager else (f"eager PyTorch NCHW {eager['nchw']:8.3f} ms, channels_last {eager['nhwc']:8.3f} ms   "
                                   f"(best eager / HIP = {best / hip:.2f})")
        print(f"{dim:4d}->{dim:<4d} @{H:3d}^2 B={B}: HIP {hip:8.3f} ms   {eg}", flush=True)
        for k, v in sorted(split.items(), key=lambda kv: -kv[1][0]):
            print(f"      {k:28s} {v[0]:9.3f} ms  {100 * v[0] / kernels_ms:5.1f} %  ({v[1]} launches)")
        if gn_gbs:
            print(f"      GroupNorm backward passes: {gn_bytes / 1e6:.1f} MB in {gn_pass_ms:.3f} ms = {gn_gbs:.0f} GB/s "
                  f"({100 * gn_gbs / HBM_PEAK_GBS:.0f} % of {HBM_PEAK_GBS / 1000:.0f} TB/s)", flush=True)
        del blk, x, temb, dout
        torch.cuda.empty_cache()
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
