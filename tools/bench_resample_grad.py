#!/usr/bin/env python3
"""Times forward + backward of the trainable layers between the denoiser's blocks -- ``ldh.Downsample``, ``ldh.Upsample`` and
``ldh.Conv2d`` (3x3, the 7x7 stem, the 1x1 head) on the HIP kernels -- against the same layer in eager PyTorch (autograd,
MIOpen convolutions) on the same GPU in one process, fp32, ms per forward + backward.

  python tools/bench_resample_grad.py [--batch 8] [--iters 20] [--warmup 3] [--cases kind:cin:cout:H,...] [--timeout 300]
A case is kind:in channels:out channels:input H = W, kind one of down, up, conv3, stem, head; the default cases are cfg3's
instances of the five layers.  Every case runs in a child process of its own under a time limit (``--timeout`` seconds; the
HIP and the eager layer share that process), and the first case that fails or runs out of time ends the run: nothing more is
started on the GPU after it.  Per case: 3 warm-up calls, then the median of 20 calls timed with events around forward +
backward.  The HIP layer reads x and the upstream gradient in its own layout (channels_last; the stem's image and the head's
gradient NCHW); eager PyTorch is timed in both memory formats, without an input gradient for the stem.  One more HIP call
under the library's per-launch timing session gives the split of the time over the entry points, and the achieved bandwidth
of each new layout and head kernel against 8 TB/s (bytes: the real channels read, the padded pixel written).  Prints one line
per case, the split, and a JSON list at the end.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_bench                                                 # noqa: E402  (puts the repository root on sys.path)
from grad_bench import HBM_PEAK_GBS                               # noqa: E402
import localdiffusion_hallucination_amd as ldh                    # noqa: E402

CASES = ("down:32:32:256,down:32:64:128,down:64:128:64,up:256:128:32,up:128:64:64,up:64:32:128,conv3:128:256:32,"
         "conv3:32:32:256,stem:1:32:256,head:32:1:256")


def pad64(c):
    return (c + 63) // 64 * 64


def build(kind, cin, cout):
    if kind == "down":
        return ldh.Downsample(cin, cout)
    if kind == "up":
        return ldh.Upsample(cin, cout)
    k = {"conv3": 3, "stem": 7, "head": 1}[kind]
    return ldh.Conv2d(cin, cout, k, padding=k // 2)


def eager_layer(kind, p, x):
    if kind == "down":
        b, c, h, w = x.shape
        y = x.reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(b, 4 * c, h // 2, w // 2)
        return F.conv2d(y, p["1.weight"], p["1.bias"])
    if kind == "up":
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), p["1.weight"], p["1.bias"], padding=1)
    return F.conv2d(x, p["weight"], p["bias"], padding={"conv3": 1, "stem": 3, "head": 0}[kind])


def eager_ms(kind, mod, x, dout, iters, warmup):
    """{"nchw": ms, "nhwc": ms} of forward + backward of the layer in eager PyTorch on clones of its parameters."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
    res = {}
    for fmt, name in ((torch.contiguous_format, "nchw"), (torch.channels_last, "nhwc")):
        xin = x.detach().contiguous(memory_format=fmt).requires_grad_(kind != "stem")
        de = dout.contiguous(memory_format=fmt)
        leaves = list(p.values()) + [xin]

        def step():
            for v in leaves:
                v.grad = None
            eager_layer(kind, p, xin).backward(de)

        res[name] = grad_bench.time_ms(step, iters, warmup)
    return res


def kernel_bytes(kind, cin, cout, B, H):
    """{entry point: bytes it must move} of the new kernels of one forward + backward (H = the input's)."""
    px, ci, cp = B * H * H * 4, cin, pad64(cin)
    if kind == "down":
        return {"dn_space_to_depth": 2 * (2 * ci * px), "dn_depth_to_space": (ci + cp) * px}      # (forward and recompute)
    if kind == "up":
        return {"dn_upsample2x": 2 * (ci + 4 * cp) * px, "dn_upsample2x_backward": (4 * ci + cp) * px}
    if kind == "stem":
        return {"dn_im2col": 2 * (ci + pad64(49 * ci)) * px}
    if kind == "head":
        return {"dn_head_forward": (ci + cout) * px, "dn_head_backward": (ci + cp + cout) * px}
    return {}


def run_case(kind, cin, cout, H, a):
    ldh.configure_runtime()
    B = a.batch
    torch.manual_seed(0)
    mod = build(kind, cin, cout).cuda()
    own = torch.contiguous_format if kind == "stem" else torch.channels_last
    x = torch.randn(B, cin, H, H, device="cuda").contiguous(memory_format=own).requires_grad_(kind != "stem")
    with torch.no_grad():
        oshape = tuple(mod(x).shape)
    dout = (torch.randn(*oshape, device="cuda") / (B * oshape[2] * oshape[3]))
    dout = dout.contiguous(memory_format=torch.contiguous_format if kind == "head" else torch.channels_last)

    def hip_step(set_phase=None):
        mod.zero_grad(set_to_none=True)
        x.grad = None
        out = mod(x)
        if set_phase:
            set_phase("backward")
        out.backward(dout)

    hip = grad_bench.time_ms(hip_step, a.iters, a.warmup)
    split, _ = grad_bench.kernel_split(hip_step)
    eager = {} if a.no_eager else eager_ms(kind, mod, x, dout, a.iters, a.warmup)
    best = min(eager.values()) if eager else None
    gbs = {k: dict(mb=nb / 1e6, ms=split[k][0], gbs=nb / (split[k][0] * 1e6))
           for k, nb in kernel_bytes(kind, cin, cout, B, H).items() if k in split and split[k][0] > 0}
    return dict(kind=kind, cin=cin, cout=cout, H=H, B=B, hip_ms=hip, eager_nchw_ms=eager.get("nchw"),
                eager_nhwc_ms=eager.get("nhwc"), eager_over_hip=(best / hip if best else None),
                kernels_ms=sum(v[0] for v in split.values()), new_kernels=gbs,
                split={k: dict(ms=v[0], launches=v[1]) for k, v in split.items()})


def report(r):
    eg = ""
    if r["eager_nchw_ms"] is not None:
        eg = (f"eager PyTorch NCHW {r['eager_nchw_ms']:8.3f} ms, channels_last {r['eager_nhwc_ms']:8.3f} ms   "
              f"(best eager / HIP = {r['eager_over_hip']:.2f})")
    print(f"{r['kind']:5s} {r['cin']:3d}->{r['cout']:<3d} @{r['H']:3d}^2 B={r['B']}: HIP {r['hip_ms']:8.3f} ms   {eg}")
    grad_bench.print_split(r["split"], r["kernels_ms"])
    for k, v in r["new_kernels"].items():
        print(f"      {k}: {v['mb']:.1f} MB in {v['ms']:.3f} ms = {v['gbs']:.0f} GB/s ({100 * v['gbs'] / HBM_PEAK_GBS:.0f} % of "
              f"{HBM_PEAK_GBS / 1000:.0f} TB/s)")


if __name__ == "__main__":
    sys.exit(grad_bench.main(__file__, CASES, run_case, report))
