#!/usr/bin/env python3
"""Times forward + backward of the whole trainable denoiser -- ``ldh.TrainableUnet`` on the HIP kernels -- against the same net
restated in eager PyTorch (autograd, MIOpen convolutions, ``F.group_norm``, einsum attention) on the same GPU in one process,
fp32, ms per forward + backward.

  python tools/bench_unet_grad.py [--iters 20] [--warmup 3] [--cases data:H:B,...] [--timeout 300] [--conv-precision fp32|bf16]
                                  [--amp no|fp16] [--amp-attn fp32|fp16]
                                  [--act-storage fp32|bf16] [--conv-out-storage fp32|bf16]
A case is data:H = W:batch; the default cases are cfg3 (mvtec, 3 x 256^2, B = 8), mri at 256^2 with B = 8 and mnist at 28^2
with B = 64.  Every case runs in a child process of its own under a time limit (``--timeout`` seconds; the HIP and the eager
net share that process), and the first case that fails or runs out of time ends the run: nothing more is started on the GPU
after it.  Per case: 3 warm-up calls, then the median of 20 calls timed with events around forward + backward (the upstream
gradient is a fixed tensor).  Eager PyTorch is timed with its inputs in NCHW and in channels_last.  One more HIP call under
the library's per-launch timing session gives the launch count and the split of the kernel time over the kernel families,
with the boundary repacks (``dn_pack_nhwc``), the glue (``dn_join``) and the time MLP each named.  Prints one line per case,
the split, and a JSON list at the end.  ``--conv-precision bf16`` times the HIP net with its convolutions on the bf16 matrix
cores (``TrainableUnet(conv_precision="bf16")``); eager PyTorch stays fp32, and the printed output difference then holds the
operands' rounding.  ``--amp fp16`` times it with the same launches on the fp16 matrix cores (``TrainableUnet(amp="fp16")``; no
loss scaling here: the gradients of sum(out * dout) stay in fp16's range).  ``--act-storage bf16`` (with ``--conv-precision bf16``) keeps the activations that only convolutions read
as bf16 (``TrainableUnet(act_storage="bf16")``): the same results; the row's ``peak_mb`` (``torch.cuda.max_memory_allocated`` over
the timed HIP calls) shows what it saves.  ``--conv-out-storage bf16`` (with ``--conv-precision bf16`` as well) keeps the
convolution outputs that the ``ResnetBlock``s' GroupNorms read as bf16 (``TrainableUnet(conv_out_storage="bf16")``); every row
prints what that takes off the tensors autograd keeps, from the blocks' shapes, to hold against the fall of ``peak_mb``.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_bench                                                 # noqa: E402  (puts the repository root on sys.path)
import localdiffusion_hallucination_amd as ldh                    # noqa: E402

CASES = "mvtec:256:8,mri:256:8,mnist:28:64"
KWARGS = {"mri": dict(mode="mri"), "mnist": dict(dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist"),
          "mvtec": dict(channels=3, out_dim=3, mode="mvtec")}
# entry point (without ld_) -> kernel family of the split; the first prefix that matches
FAMILIES = (("dn_pack_nhwc", "dn_pack_nhwc (boundary repacks)"), ("dn_join", "dn_join (cat, attn(x) + x)"),
            ("dn_time_mlp", "time MLP"), ("dn_time_proj", "time projections"), ("pc_conv (forward)", "convolutions, forward"),
            ("pc_conv (data gradient)", "convolutions, data gradient"), ("seg_wgrad", "convolutions, weight gradient"),
            ("dn_conv16 (forward)", "convolutions, forward"), ("dn_conv16 (data gradient)", "convolutions, data gradient"),
            ("dn_conv16_from16 (forward)", "convolutions, forward"), ("dn_conv16_from16 (data gradient)", "convolutions, data gradient"),
            ("dn_conv16_to16 (forward)", "convolutions, forward"), ("dn_conv16_from16_to16 (forward)", "convolutions, forward"),
            ("dn_wgrad16", "convolutions, weight gradient"), ("dn_pack_conv16", "weight packing (bf16)"),
            ("dn_conv_f16 (forward)", "convolutions, forward"), ("dn_conv_f16 (data gradient)", "convolutions, data gradient"),
            ("dn_wgrad_f16", "convolutions, weight gradient"), ("dn_pack_conv_f16", "weight packing (fp16)"),
            ("dn_colsum", "bias gradients"), ("dn_gn", "GroupNorm"), ("dn_la_", "linear attention"), ("dn_fa_", "full attention"),
            ("dn_rms_", "RMSNorm"), ("dn_head_", "head"), ("seg_pool", "max pool"))
SWITCHES = tuple(grad_bench.SWITCH_HELP)            # every training precision switch: all are TrainableUnet arguments


# ---------------------------------------------------------------------------------------------------- the net in eager PyTorch
def _rms(x, g):
    return F.normalize(x, dim=1) * g * (x.shape[1] ** 0.5)


def _block(p, pre, x, temb, groups):
    film = None
    if temb is not None:
        film = F.linear(F.silu(temb), p[pre + ".mlp.1.weight"], p[pre + ".mlp.1.bias"])[:, :, None, None].chunk(2, dim=1)
    h = F.group_norm(F.conv2d(x, p[pre + ".block1.proj.weight"], p[pre + ".block1.proj.bias"], padding=1), groups,
                     p[pre + ".block1.norm.weight"], p[pre + ".block1.norm.bias"])
    if film is not None:
        h = h * (film[0] + 1) + film[1]
    h = F.silu(h)
    h = F.silu(F.group_norm(F.conv2d(h, p[pre + ".block2.proj.weight"], p[pre + ".block2.proj.bias"], padding=1), groups,
                            p[pre + ".block2.norm.weight"], p[pre + ".block2.norm.bias"]))
    if pre + ".res_conv.weight" in p:
        x = F.conv2d(x, p[pre + ".res_conv.weight"], p[pre + ".res_conv.bias"])
    return h + x


def _attention(p, pre, x, heads, full):
    b, c, hh, ww = x.shape
    qkv = F.conv2d(_rms(x, p[pre + ".norm.g"]), p[pre + ".to_qkv.weight"])
    q, k, v = [t.reshape(b, heads, 32, hh * ww) for t in qkv.chunk(3, dim=1)]
    if full:
        att = (torch.einsum("bhdi,bhdj->bhij", q, k) * 32 ** -0.5).softmax(dim=-1)
        out = torch.einsum("bhij,bhdj->bhdi", att, v).reshape(b, heads * 32, hh, ww)
        return F.conv2d(out, p[pre + ".to_out.weight"], p[pre + ".to_out.bias"])
    q, k = q.softmax(dim=-2) * 32 ** -0.5, k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(b, heads * 32, hh, ww)
    return _rms(F.conv2d(out, p[pre + ".to_out.0.weight"], p[pre + ".to_out.0.bias"]), p[pre + ".to_out.1.g"])


def _basic(p, pre, x):
    y = F.relu(F.group_norm(F.conv2d(x, p[pre + ".convblock.0.weight"], p[pre + ".convblock.0.bias"], padding=1), 16,
                            p[pre + ".convblock.1.weight"], p[pre + ".convblock.1.bias"]))
    y = F.group_norm(F.conv2d(y, p[pre + ".convblock.3.weight"], p[pre + ".convblock.3.bias"], padding=1), 16,
                     p[pre + ".convblock.4.weight"], p[pre + ".convblock.4.bias"])
    i = F.group_norm(F.conv2d(x, p[pre + ".identity.0.weight"], p[pre + ".identity.0.bias"], padding=1), 16,
                     p[pre + ".identity.1.weight"], p[pre + ".identity.1.bias"])
    return F.relu(y + i)


def eager_unet(p, cfg, freqs, x, cond, time):
    """ddpm.py:404-451 on a dict of parameters with the reference's names."""
    g, hd, n, fa = cfg.resnet_block_groups, cfg.attn_heads, len(cfg.dim_mults), cfg.full_attn
    x = F.conv2d(x, p["init_conv.weight"], p["init_conv.bias"], padding=3)
    r = x
    ang = time[:, None] * freqs[None, :]
    t = F.linear(torch.cat((ang.sin(), ang.cos()), dim=-1), p["time_mlp.1.weight"], p["time_mlp.1.bias"])
    t = F.linear(F.gelu(t), p["time_mlp.3.weight"], p["time_mlp.3.bias"])
    h = []
    for i in range(n):
        pre = f"downs.{i}"
        x = _block(p, pre + ".0", x, t, g)
        h.append(x)
        x = _block(p, pre + ".1", x, t, g)
        x = _attention(p, pre + ".2", x, hd, fa[i]) + x
        h.append(x)
        if i < n - 1:
            b, c, hh, ww = x.shape
            y = x.reshape(b, c, hh // 2, 2, ww // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(b, 4 * c, hh // 2, ww // 2)
            x = F.conv2d(y, p[pre + ".3.1.weight"], p[pre + ".3.1.bias"])
        else:
            x = F.conv2d(x, p[pre + ".3.weight"], p[pre + ".3.bias"], padding=1)
    x = _block(p, "mid_block1", x, t, g)
    x = _attention(p, "mid_attn", x, hd, True) + x
    x = _block(p, "mid_block2", x, t, g)
    f = F.max_pool2d(_basic(p, "cond_model.residual_conv1.0", cond), 2)
    f = F.max_pool2d(_basic(p, "cond_model.residual_conv2.0", f), 2)
    f = _basic(p, "cond_model.residual_conv3.0", f)
    if not cfg.cond_early_exit:
        f = _basic(p, "cond_model.mid_conv.0", F.max_pool2d(f, 2))
    x = _block(p, "conv_fusion", torch.cat((x, f), dim=1), None, g)
    for j in range(n):
        pre = f"ups.{j}"
        x = _block(p, pre + ".0", torch.cat((x, h.pop()), dim=1), t, g)
        x = _block(p, pre + ".1", torch.cat((x, h.pop()), dim=1), t, g)
        x = _attention(p, pre + ".2", x, hd, fa[n - 1 - j]) + x
        if j < n - 1:
            x = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), p[pre + ".3.1.weight"], p[pre + ".3.1.bias"], padding=1)
        else:
            x = F.conv2d(x, p[pre + ".3.weight"], p[pre + ".3.bias"], padding=1)
    x = _block(p, "final_res_block", torch.cat((x, r), dim=1), t, g)
    return F.conv2d(x, p["final_conv.weight"], p["final_conv.bias"])


def eager_ms(net, x, cond, time, dout, iters, warmup):
    """{"nchw": ms, "nhwc": ms} of forward + backward of the net in eager PyTorch on clones of its parameters."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    freqs = net.time_mlp.freqs
    res, check = {}, None
    for fmt, name in ((torch.contiguous_format, "nchw"), (torch.channels_last, "nhwc")):
        xin, cin, de = (t.detach().contiguous(memory_format=fmt) for t in (x, cond, dout))

        def step():
            for v in p.values():
                v.grad = None
            out = eager_unet(p, net.cfg, freqs, xin, cin, time)
            out.backward(de)
            return out

        res[name] = grad_bench.time_ms(step, iters, warmup)
        check = step().detach()
    return res, check


def families(split):
    out = {}
    for label, (ms, launches) in split.items():
        fam = next((name for prefix, name in FAMILIES if label.startswith(prefix)), "layout (s2d, upsample, im2col, gather)")
        e = out.setdefault(fam, dict(ms=0.0, launches=0))
        e["ms"] += ms
        e["launches"] += launches
    return out


def run_case(data, H, B, a):
    ldh.configure_runtime()
    torch.manual_seed(0)
    net = ldh.TrainableUnet(dim=32, **grad_bench.switch_values(a, SWITCHES), amp=a.amp, amp_attn=a.amp_attn, **KWARGS[data]).cuda()
    cfg = net.cfg
    x = torch.randn(B, cfg.channels, H, H, device="cuda")
    cond = torch.rand(B, cfg.cond_in_channels, H, H, device="cuda") * 2
    time = torch.randint(0, 1000, (B,), device="cuda")
    dout = torch.randn(B, cfg.out_dim, H, H, device="cuda") / (B * H * H)

    def hip_step(set_phase=None):
        net.zero_grad(set_to_none=True)
        out = net(x, cond, time)
        if set_phase:
            set_phase("backward")
        out.backward(dout)
        return out

    # what conv_out_storage "bf16" takes off the tensors autograd keeps: y1 and y2 of every ResnetBlock, 2 bytes an element
    seen = []
    hooks = [m.register_forward_pre_hook(lambda m, args: seen.append(args[0].shape[0] * args[0].shape[2] * args[0].shape[3] * m.cop))
             for m in net.modules() if isinstance(m, ldh.ResnetBlock)]
    with torch.no_grad():
        net(x, cond, time)
    for h in hooks:
        h.remove()
    y_saving = 2 * 2 * sum(seen)

    torch.cuda.reset_peak_memory_stats()
    hip = grad_bench.time_ms(hip_step, a.iters, a.warmup)
    peak = torch.cuda.max_memory_allocated()
    split, _ = grad_bench.kernel_split(hip_step)
    fam = families(split)
    eager, diff = {}, None
    if not a.no_eager:
        eager, ref = eager_ms(net, x, cond, time, dout, a.iters, a.warmup)
        diff = float((hip_step().detach() - ref).abs().max())
    best = min(eager.values()) if eager else None
    return dict(data=data, H=H, B=B, **grad_bench.switch_values(a, SWITCHES), amp=a.amp, amp_attn=a.amp_attn, peak_mb=peak / 2 ** 20,
                conv_out_bf16_saves_mb=y_saving / 2 ** 20, resnet_blocks=len(seen), hip_ms=hip, eager_nchw_ms=eager.get("nchw"),
                eager_nhwc_ms=eager.get("nhwc"),
                eager_over_hip=(best / hip if best else None), out_diff_to_eager=diff,
                kernels_ms=sum(v[0] for v in split.values()), launches=sum(v[1] for v in split.values()), split=fam)


def report(r):
    eg = ""
    if r["eager_nchw_ms"] is not None:
        eg = (f"eager PyTorch NCHW {r['eager_nchw_ms']:9.3f} ms, channels_last {r['eager_nhwc_ms']:9.3f} ms   "
              f"(best eager / HIP = {r['eager_over_hip']:.2f}; outputs differ by {r['out_diff_to_eager']:.1e})")
    print(f"{r['data']:5s} @{r['H']:3d}^2 B={r['B']:<2d} {r['conv_precision']} / act {r['act_storage']} / conv out {r['conv_out_storage']} / attn {r['attn_precision']} / full attn {r['full_attn_precision']}{grad_bench.amp_tag(r)}: HIP {r['hip_ms']:9.3f} ms, "
          f"peak {r['peak_mb']:8.1f} MiB (y1 / y2 of the {r['resnet_blocks']} ResnetBlocks as bf16 {'save' if r['conv_out_storage'] == 'bf16' else 'would save'} "
          f"{r['conv_out_bf16_saves_mb']:.1f} MiB of what autograd keeps), {r['launches']} launches, kernels {r['kernels_ms']:9.3f} ms   {eg}")
    grad_bench.print_split(r["split"], r["kernels_ms"])


if __name__ == "__main__":
    sys.exit(grad_bench.main(__file__, CASES, run_case, report, switches=SWITCHES, amp=True, amp_attn=True))
