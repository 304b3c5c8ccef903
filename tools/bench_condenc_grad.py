#!/usr/bin/env python3
"""Times forward + backward of the trainable condition encoder -- ``ldh.BasicBlock`` and ``ldh.ResUnet`` on the HIP kernels --
against the same module in eager PyTorch (autograd, MIOpen convolutions, ``F.group_norm``, ``F.max_pool2d``) on the same GPU
in one process, fp32, ms per forward + backward.

  python tools/bench_condenc_grad.py [--batch 8] [--iters 20] [--warmup 3] [--cases kind:data:H,...] [--timeout 300]
A case is kind:data:input H = W of the whole encoder, kind one of block1, block2, block3, block4 (the block alone, at the map
size it has inside the encoder) and encoder; the default cases are the mri encoder at 256^2 and its four blocks.  Every case
runs in a child process of its own under a time limit (``--timeout`` seconds; the HIP and the eager module share that
process), and the first case that fails or runs out of time ends the run: nothing more is started on the GPU after it.  Per
case: 3 warm-up calls, then the median of 20 calls timed with events around forward + backward.  The HIP module reads x and
the upstream gradient in its own layout (channels_last; the image NCHW); eager PyTorch is timed in both memory formats,
without an input gradient where the input is the image.  One more HIP call under the library's per-launch timing session
gives the split of the time over the entry points, and the achieved bandwidth of the new GroupNorm and im2col kernels against
8 TB/s (bytes: the real channels read, the padded pixel written).  Prints one line per case, the split, and a JSON list at the
end.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_bench                                                 # noqa: E402  (puts the repository root on sys.path)
from grad_bench import HBM_PEAK_GBS                               # noqa: E402
import localdiffusion_hallucination_amd as ldh                    # noqa: E402

CASES = "block1:mri:256,block2:mri:256,block3:mri:256,block4:mri:256,encoder:mri:256"
NAMES = ("residual_conv1", "residual_conv2", "residual_conv3", "mid_conv")


def pad64(c):
    return (c + 63) // 64 * 64


def eager_block(p, pre, x, pool):
    y = F.conv2d(x, p[pre + "convblock.0.weight"], p[pre + "convblock.0.bias"], padding=1)
    y = F.relu(F.group_norm(y, 16, p[pre + "convblock.1.weight"], p[pre + "convblock.1.bias"]))
    y = F.conv2d(y, p[pre + "convblock.3.weight"], p[pre + "convblock.3.bias"], padding=1)
    y = F.group_norm(y, 16, p[pre + "convblock.4.weight"], p[pre + "convblock.4.bias"])
    i = F.conv2d(x, p[pre + "identity.0.weight"], p[pre + "identity.0.bias"], padding=1)
    out = F.relu(y + F.group_norm(i, 16, p[pre + "identity.1.weight"], p[pre + "identity.1.bias"]))
    return F.max_pool2d(out, 2) if pool else out


def eager_module(mod, p, x):
    if isinstance(mod, ldh.BasicBlock):
        return eager_block(p, "", x, mod.pool)
    for name in NAMES:
        if hasattr(mod, name):
            x = eager_block(p, name + ".0.", x, getattr(mod, name)[0].pool)
    return x


def eager_ms(mod, x, dout, x_grad, iters, warmup):
    """{"nchw": ms, "nhwc": ms} of forward + backward of the module in eager PyTorch on clones of its parameters."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
    res = {}
    for fmt, name in ((torch.contiguous_format, "nchw"), (torch.channels_last, "nhwc")):
        xin = x.detach().contiguous(memory_format=fmt).requires_grad_(x_grad)
        de = dout.contiguous(memory_format=fmt)
        leaves = list(p.values()) + [xin]

        def step():
            for v in leaves:
                v.grad = None
            eager_module(mod, p, xin).backward(de)

        res[name] = grad_bench.time_ms(step, iters, warmup)
    return res


def kernel_bytes(blocks, B):
    """{entry point: bytes it must move} of the new kernels of one forward + backward of ``blocks`` = [(block, input H)]."""
    nb = {"dn_gnr_forward": 0, "dn_gnr_backward": 0, "dn_im2col3": 0}
    for blk, H in blocks:
        px = B * H * H * 4
        for c, cp, nop in ((blk.mid_dim, blk.cmp, 1), (blk.dim_out, blk.cop, 2)):
            nb["dn_gnr_forward"] += (2 * nop * c + cp) * px           # statistics pass and apply pass read y, out written
            nb["dn_gnr_backward"] += (2 * (2 + nop) * c + nop * cp) * px   # both passes read dout, act and y; dy written
        if blk.image:
            nb["dn_im2col3"] += 2 * (blk.dim + blk.cik) * px           # (forward and recompute)
    return {k: v for k, v in nb.items() if v}


def run_case(kind, data, H, a):
    ldh.configure_runtime()
    B = a.batch
    torch.manual_seed(0)
    net = ldh.ResUnet(data)
    if kind == "encoder":
        mod, Hin = net, H
        blocks = [(getattr(net, n)[0], H >> i) for i, n in enumerate(NAMES) if hasattr(net, n)]
    else:
        i = int(kind[len("block"):]) - 1
        mod, Hin = getattr(net, NAMES[i])[0], H >> i
        blocks = [(mod, Hin)]
    mod = mod.cuda()
    cin = blocks[0][0].dim
    x_grad = cin > 4
    own = torch.channels_last if x_grad else torch.contiguous_format
    x = torch.rand(B, cin, Hin, Hin, device="cuda") * 2 if not x_grad else torch.randn(B, cin, Hin, Hin, device="cuda")
    x = x.contiguous(memory_format=own).requires_grad_(x_grad)
    with torch.no_grad():
        oshape = tuple(mod(x).shape)
    dout = (torch.randn(*oshape, device="cuda") / (B * oshape[2] * oshape[3])).contiguous(memory_format=torch.channels_last)

    def hip_step(set_phase=None):
        mod.zero_grad(set_to_none=True)
        x.grad = None
        out = mod(x)
        if set_phase:
            set_phase("backward")
        out.backward(dout)

    hip = grad_bench.time_ms(hip_step, a.iters, a.warmup)
    split, _ = grad_bench.kernel_split(hip_step)
    eager = {} if a.no_eager else eager_ms(mod, x, dout, x_grad, a.iters, a.warmup)
    best = min(eager.values()) if eager else None
    gbs = {k: dict(mb=nb / 1e6, ms=split[k][0], gbs=nb / (split[k][0] * 1e6))
           for k, nb in kernel_bytes(blocks, B).items() if k in split and split[k][0] > 0}
    return dict(kind=kind, data=data, cin=cin, cout=oshape[1], H=Hin, B=B, hip_ms=hip, eager_nchw_ms=eager.get("nchw"),
                eager_nhwc_ms=eager.get("nhwc"), eager_over_hip=(best / hip if best else None),
                kernels_ms=sum(v[0] for v in split.values()), new_kernels=gbs,
                split={k: dict(ms=v[0], launches=v[1]) for k, v in split.items()})


def report(r):
    eg = ""
    if r["eager_nchw_ms"] is not None:
        eg = (f"eager PyTorch NCHW {r['eager_nchw_ms']:8.3f} ms, channels_last {r['eager_nhwc_ms']:8.3f} ms   "
              f"(best eager / HIP = {r['eager_over_hip']:.2f})")
    print(f"{r['kind']:7s} {r['data']} {r['cin']:3d}->{r['cout']:<3d} @{r['H']:3d}^2 B={r['B']}: HIP {r['hip_ms']:8.3f} ms   {eg}")
    grad_bench.print_split(r["split"], r["kernels_ms"])
    for k, v in r["new_kernels"].items():
        print(f"      {k}: {v['mb']:.1f} MB in {v['ms']:.3f} ms = {v['gbs']:.0f} GB/s ({100 * v['gbs'] / HBM_PEAK_GBS:.0f} % of "
              f"{HBM_PEAK_GBS / 1000:.0f} TB/s)")


if __name__ == "__main__":
    sys.exit(grad_bench.main(__file__, CASES, run_case, report))
