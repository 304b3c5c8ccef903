#!/usr/bin/env python3
"""Times forward + backward of one trainable ResnetBlock: ``ldh.ResnetBlock`` on the HIP kernels against the same block
restated in eager PyTorch (autograd, MIOpen convolutions) on the same GPU in one process, fp32, ms per forward + backward.

  python tools/bench_resblock_grad.py [--batch 8] [--iters 20] [--warmup 3] [--cases 32:256,64:128,128:64,256:32]
                                      [--timeout 300] [--conv-precision fp32|bf16] [--act-storage fp32|bf16]
                                      [--conv-out-storage fp32|bf16]
The default cases are cfg3's four levels (dim -> dim at H = W).  Every case runs in a child process of its own under a time
limit (``--timeout`` seconds; the HIP and the eager block share that process), and the first case that fails or runs out of
time ends the run: nothing more is started on the GPU after it.  Per case: 3 warm-up calls, then the median of 20 calls
timed with events around forward + backward.  The HIP block reads x and the upstream gradient in channels_last (its own
layout; a channel count that is not a multiple of 64 is repacked with padding either way); eager PyTorch is timed in both
memory formats.  One more HIP call under the library's per-launch timing session gives the split of the time over the
entry points, and the achieved bandwidth of the two GroupNorm-backward passes against 8 TB/s (bytes: dout and y read by
each pass, dy written once; padded channels are written but never read).  Prints one line per case, the split, and a JSON
list at the end.  ``--conv-precision bf16`` runs the HIP block's convolutions on the bf16 matrix cores and ``--act-storage
bf16`` (with it) keeps block1's activation as bf16 (``ResnetBlock.act_storage``; dim -> dim blocks have no ``res_conv``, so x
stays fp32); eager PyTorch stays fp32.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_bench                                                 # noqa: E402  (puts the repository root on sys.path)
from grad_bench import HBM_PEAK_GBS                               # noqa: E402
import localdiffusion_hallucination_amd as ldh                    # noqa: E402

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


def gn_bytes(dim, B, H, y_bytes=4):
    """two GroupNorms x (dout and y read by each of the two passes: the real channels; dy written: the padded pixel); y has
    ``y_bytes`` bytes per element (2 at ``--conv-out-storage bf16``)"""
    return 2 * ((2 * 4 + 2 * y_bytes) * dim + (dim + 63) // 64 * 64 * 4) * B * H * H

SWITCHES = ("conv_precision", "act_storage", "conv_out_storage")


def run_case(dim, H, a):
    ldh.configure_runtime()
    B = a.batch
    torch.manual_seed(0)
    blk = ldh.ResnetBlock(dim, dim, time_emb_dim=TIME_DIM).cuda()
    switches = grad_bench.switch_values(a, SWITCHES)
    for s, v in switches.items():
        setattr(blk, s, v)
    blk.amp = a.amp
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

    hip = grad_bench.time_ms(hip_step, a.iters, a.warmup)
    split, calls = grad_bench.kernel_split(hip_step)
    # the three launches of ld_dn_gn_backward are sums, finalisation, dy: the two passes are the first and the last
    gn_pass_ms = sum((ms[0] + ms[2] for label, ms in calls if label.startswith("dn_gn_backward") and len(ms) == 3), 0.0)
    y_bytes = 2 if a.conv_out_storage == "bf16" else 4
    # every GroupNorm call's launches in order (forward: statistics, finalisation, apply), by entry point
    gn_launches = [(label, ms) for label, ms in calls if label.startswith("dn_gn_")]
    eager = {} if a.no_eager else grad_bench.eager_ms(blk, eager_block, x, [temb], dout, a.iters, a.warmup)
    best = min(eager.values()) if eager else None
    return dict(dim=dim, H=H, B=B, **switches, amp=a.amp, hip_ms=hip, eager_nchw_ms=eager.get("nchw"), eager_nhwc_ms=eager.get("nhwc"),
                eager_over_hip=(best / hip if best else None), kernels_ms=sum(v[0] for v in split.values()),
                gn_backward_passes_ms=gn_pass_ms, gn_backward_mb=gn_bytes(dim, B, H, y_bytes) / 1e6, gn_launches_ms=gn_launches,
                gn_backward_gbs=(gn_bytes(dim, B, H, y_bytes) / (gn_pass_ms * 1e6) if gn_pass_ms else None),
                split={k: dict(ms=v[0], launches=v[1]) for k, v in split.items()})


def report(r):
    eg = ""
    if r["eager_nchw_ms"] is not None:
        eg = (f"eager PyTorch NCHW {r['eager_nchw_ms']:8.3f} ms, channels_last {r['eager_nhwc_ms']:8.3f} ms   "
              f"(best eager / HIP = {r['eager_over_hip']:.2f})")
    print(f"{r['dim']:4d}->{r['dim']:<4d} @{r['H']:3d}^2 B={r['B']} {r['conv_precision']} / act {r['act_storage']} / conv out {r['conv_out_storage']}{grad_bench.amp_tag(r)}: HIP {r['hip_ms']:8.3f} ms   "
          f"{eg}")
    grad_bench.print_split(r["split"], r["kernels_ms"])
    if r["gn_backward_gbs"]:
        for label, ms in r["gn_launches_ms"]:
            print(f"      {label:28s} launches: " + "  ".join(f"{v:.4f}" for v in ms) + " ms")
        print(f"      GroupNorm backward passes: {r['gn_backward_mb']:.1f} MB in {r['gn_backward_passes_ms']:.3f} ms = "
              f"{r['gn_backward_gbs']:.0f} GB/s ({100 * r['gn_backward_gbs'] / HBM_PEAK_GBS:.0f} % of "
              f"{HBM_PEAK_GBS / 1000:.0f} TB/s)")


if __name__ == "__main__":
    sys.exit(grad_bench.main(__file__, "32:256,64:128,128:64,256:32", run_case, report, switches=SWITCHES, amp=True))
