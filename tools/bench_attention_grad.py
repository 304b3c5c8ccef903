#!/usr/bin/env python3
"""Times forward + backward of one trainable full Attention: ``ldh.Attention`` on the HIP kernels against the same module
restated in eager PyTorch (autograd) on the same GPU in one process, fp32, ms per forward + backward.

  python tools/bench_attention_grad.py [--batch 8] [--heads 4] [--iters 20] [--warmup 3] [--cases 128:32,256:32]
                                       [--timeout 300] [--full-attn-precision fp32|bf16] [--amp-attn fp32|fp16]
The default cases are cfg3's two uses of full attention (dim at H = W): the last stage of the down and up paths and
``mid_attn``.  Every case runs in a child process of its own under a time limit (``--timeout`` seconds; the HIP and the eager
module share that process), and the first case that fails or runs out of time ends the run: nothing more is started on the
GPU after it.  Per case: 3 warm-up calls, then the median of 20 calls timed with events around forward + backward.  The HIP
module reads x and the upstream gradient in channels_last (its own layout); eager PyTorch is timed in two forms -- the
reference's einsum / softmax lines and ``F.scaled_dot_product_attention`` -- each in both memory formats, and the best of
the four is quoted.  One more HIP call under the library's per-launch timing session gives the split of the time over the
entry points, and the achieved FLOP/s of the three attention passes against the 157 TFLOP/s fp32 matrix peak.

How the FLOPs are counted -- tile products of 2 n^2 32 FLOP per (sample, head), exponentials and rescales not counted: the
forward has two (q k^T, p v), the backward's row pass three (q k^T, dO v^T, ds k), its column pass four (k q^T, v dO^T, p^T
dO, ds^T q).  ``--full-attn-precision bf16`` times the module with its core on the bf16 matrix cores
(``Attention.full_attn_precision``; the eager side stays fp32, and the percentage stays against the fp32 matrix peak so that
the two settings' rows compare).  Prints one line per case, the split, and a JSON list at the end.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_bench                                                 # noqa: E402  (puts the repository root on sys.path)
from grad_bench import HBM_PEAK_GBS                               # noqa: E402
import localdiffusion_hallucination_amd as ldh                    # noqa: E402

FP32_MATRIX_PEAK_TFLOPS = 157.0
# pass -> (entry point's label, index of its launch inside the entry point, tile products)
PASSES = {"forward": ("dn_fa_forward", 0, 2), "backward rows (dq)": ("dn_fa_backward", 0, 3),
          "backward columns (dk, dv)": ("dn_fa_backward", 1, 4)}


def eager_attention(p, x, heads, sdpa):
    b, c, h, w = x.shape
    qkv = F.conv2d(F.normalize(x, dim=1) * p["norm.g"] * c ** 0.5, p["to_qkv.weight"])
    q, k, v = [t.reshape(b, heads, 32, h * w).transpose(-1, -2) for t in qkv.chunk(3, dim=1)]
    if sdpa:
        out = F.scaled_dot_product_attention(q, k, v)
    else:
        sim = torch.einsum("bhid,bhjd->bhij", q, k) * 32 ** -0.5
        out = torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), v)
    out = out.transpose(-1, -2).reshape(b, heads * 32, h, w)
    return F.conv2d(out, p["to_out.weight"], p["to_out.bias"])


def run_case(dim, H, a):
    ldh.configure_runtime()
    B, heads = a.batch, a.heads
    torch.manual_seed(0)
    mod = ldh.Attention(dim, heads=heads).cuda()
    mod.full_attn_precision = a.full_attn_precision
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
    passes = {name: ms[idx] for label, ms in calls for name, (lab, idx, _) in PASSES.items() if label in (lab, lab + "16", lab + "_f16") and len(ms) > idx}
    n = H * H
    tflops = {k: PASSES[k][2] * 2 * n * n * 32 * B * heads / (ms * 1e9) for k, ms in passes.items() if ms > 0}
    eager = {}
    for sdpa in () if a.no_eager else (False, True):
        res = grad_bench.eager_ms(mod, lambda p, xe: eager_attention(p, xe, heads, sdpa), x, [], dout, a.iters, a.warmup)
        eager.update({("sdpa_" if sdpa else "einsum_") + k: v for k, v in res.items()})
    best = min(eager.values()) if eager else None
    return dict(dim=dim, H=H, B=B, heads=heads, full_attn_precision=a.full_attn_precision, amp_attn=a.amp_attn, hip_ms=hip, eager_ms=eager, eager_over_hip=(best / hip if best else None),
                kernels_ms=sum(v[0] for v in split.values()), pass_ms=passes, pass_tflops=tflops,
                split={k: dict(ms=v[0], launches=v[1]) for k, v in split.items()})


def report(r):
    eg = ""
    if r["eager_ms"]:
        eg = "eager PyTorch " + ", ".join(f"{k} {v:.3f} ms" for k, v in r["eager_ms"].items()) + \
            f"   (best eager / HIP = {r['eager_over_hip']:.2f})"
    print(f"dim {r['dim']:4d} heads {r['heads']} @{r['H']:3d}^2 B={r['B']} full attn {r['full_attn_precision']}{grad_bench.amp_tag(r)}: HIP {r['hip_ms']:8.3f} ms   {eg}")
    grad_bench.print_split(r["split"], r["kernels_ms"])
    for k, t in r["pass_tflops"].items():
        print(f"      {k:28s} {r['pass_ms'][k]:.3f} ms = {t:.1f} TFLOP/s ({100 * t / FP32_MATRIX_PEAK_TFLOPS:.0f} % of "
              f"{FP32_MATRIX_PEAK_TFLOPS:.0f})")
    mb = 3 * 32 * r["heads"] * 4 * r["B"] * r["H"] ** 2 / 1e6
    print(f"      qkv is {mb:.1f} MB = {mb / HBM_PEAK_GBS:.4f} ms at {HBM_PEAK_GBS / 1000:.0f} TB/s, what a pass would take were it memory-bound")


if __name__ == "__main__":
    sys.exit(grad_bench.main(__file__, "128:32,256:32", run_case, report, heads=True, switches=("full_attn_precision",), amp_attn=True))
