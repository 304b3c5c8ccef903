#!/usr/bin/env python3
"""Times forward + backward of one trainable LinearAttention: ``ldh.LinearAttention`` on the HIP kernels against the same
module restated in eager PyTorch (autograd) on the same GPU in one process, fp32, ms per forward + backward.

  python tools/bench_linattn_grad.py [--batch 8] [--heads 4] [--iters 20] [--warmup 3] [--cases 32:256,64:128,128:64]
                                     [--timeout 300] [--attn-precision {fp32,bf16}] [--amp-attn {fp32,fp16}]
The default cases are the three levels of cfg3 that use linear attention (dim at H = W).  Every case runs in a child
process of its own under a time limit (``--timeout`` seconds; the HIP and the eager module share that process), and the
first case that fails or runs out of time ends the run: nothing more is started on the GPU after it.  Per case: 3 warm-up
calls, then the median of 20 calls timed with events around forward + backward.  The HIP module reads x and the upstream
gradient in channels_last (its own layout; a channel count that is not a multiple of 64 is repacked with padding either
way); eager PyTorch is timed in both memory formats.  One more HIP call under the library's per-launch timing session gives
the split of the time over the entry points (at ``--attn-precision bf16`` the four passes are the ``...16`` entry points of
csrc/linattn16.hip and are listed under those names), and the achieved bandwidth of the four attention passes against 8 TB/s.

How the bytes are counted -- what the pass has to move, each tensor once, the real channels only (hidden = 32 heads floats
per pixel and tensor): context = k and v read (its second look at k, for the part's maximum, is not counted); output = q
read, out written; reduce = q and dO read; apply = q, k, v and dO read, dq, dk, dv written.  The time is that of the pass's
main launch; the merges of the parts are listed with the split.  Prints one line per case, the split, and a JSON list at
the end.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_bench                                                 # noqa: E402  (puts the repository root on sys.path)
from grad_bench import HBM_PEAK_GBS                               # noqa: E402
import localdiffusion_hallucination_amd as ldh                    # noqa: E402

# label -> (index of the pass's main launch inside the entry point, tensors of `hidden` floats per pixel it moves)
PASSES = {"dn_la_context": (0, 2), "dn_la_out": (0, 2), "dn_la_backward_reduce": (0, 2), "dn_la_backward_apply": (0, 7)}
PASSES.update({k + s: v for k, v in list(PASSES.items()) for s in ("16", "_f16")})    # --attn-precision bf16, --amp-attn fp16


def eager_attention(p, x, heads):
    b, c, h, w = x.shape

    def rms(t, g):
        return F.normalize(t, dim=1) * g * c ** 0.5

    qkv = F.conv2d(rms(x, p["norm.g"]), p["to_qkv.weight"])
    q, k, v = [t.reshape(b, heads, 32, h * w) for t in qkv.chunk(3, dim=1)]
    q = q.softmax(dim=-2) * 32 ** -0.5
    k = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(b, heads * 32, h, w)
    return rms(F.conv2d(out, p["to_out.0.weight"], p["to_out.0.bias"]), p["to_out.1.g"])


def run_case(dim, H, a):
    ldh.configure_runtime()
    B, heads = a.batch, a.heads
    torch.manual_seed(0)
    mod = ldh.LinearAttention(dim, heads=heads).cuda()
    mod.attn_precision = a.attn_precision
    mod.amp_attn = a.amp_attn
    x = torch.randn(B, dim, H, H, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dout = (torch.randn(B, dim, H, H, device="cuda") / (B * H * H)).contiguous(memory_format=torch.channels_last)

    def hip_step(set_phase=None):
        mod.zero_grad(set_to_none=True)
        x.grad = None
        out = mod(x)
        if set_phase:
            set_phase("backward")
        out.backward(dout)

    hip = grad_bench.time_ms(hip_step, a.iters, a.warmup)
    split, calls = grad_bench.kernel_split(hip_step)
    passes = {label: ms[PASSES[label][0]] for label, ms in calls if label in PASSES and ms}
    gbs = {k: PASSES[k][1] * mod.hidden * 4 * B * H * H / (ms * 1e6) for k, ms in passes.items() if ms > 0}
    eager = {} if a.no_eager else grad_bench.eager_ms(mod, lambda p, xe: eager_attention(p, xe, heads), x, [], dout, a.iters,
                                                      a.warmup)
    best = min(eager.values()) if eager else None
    return dict(dim=dim, H=H, B=B, heads=heads, attn_precision=a.attn_precision, amp_attn=a.amp_attn, hip_ms=hip, eager_nchw_ms=eager.get("nchw"), eager_nhwc_ms=eager.get("nhwc"),
                eager_over_hip=(best / hip if best else None), kernels_ms=sum(v[0] for v in split.values()), pass_ms=passes,
                pass_gbs=gbs, split={k: dict(ms=v[0], launches=v[1]) for k, v in split.items()})


def report(r):
    eg = ""
    if r["eager_nchw_ms"] is not None:
        eg = (f"eager PyTorch NCHW {r['eager_nchw_ms']:8.3f} ms, channels_last {r['eager_nhwc_ms']:8.3f} ms   "
              f"(best eager / HIP = {r['eager_over_hip']:.2f})")
    print(f"dim {r['dim']:4d} heads {r['heads']} @{r['H']:3d}^2 B={r['B']} attn {r['attn_precision']}{grad_bench.amp_tag(r)}: HIP {r['hip_ms']:8.3f} ms   {eg}")
    grad_bench.print_split(r["split"], r["kernels_ms"])
    for k, g in r["pass_gbs"].items():
        print(f"      {k:28s} main launch {r['pass_ms'][k]:.3f} ms = {g:.0f} GB/s ({100 * g / HBM_PEAK_GBS:.0f} % of "
              f"{HBM_PEAK_GBS / 1000:.0f} TB/s)")


if __name__ == "__main__":
    sys.exit(grad_bench.main(__file__, "32:256,64:128,128:64", run_case, report, heads=True, switches=("attn_precision",), amp_attn=True))
