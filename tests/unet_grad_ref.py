"""Helpers of the whole-denoiser gradient tests: a restatement of ``oracle.unet_ref.unet_forward`` (ddpm.py:404-451) that runs
in any dtype under ``torch.autograd`` -- the oracle casts ``cond`` to fp32 and multiplies an integer ``time`` by an fp32 table,
so it cannot give an fp64 yardstick as it stands -- on the oracle's own blocks, which take any dtype; the inputs of the three
small cases; and the yardsticks (every parameter's gradient of sum(out * dout), and plain SGD on the training loss).  CPU only.
The bounds are ``resblock_ref``'s.

In fp32 the restatement is the oracle bit for bit (test_unet_grad.py).  In fp64 the angle of the sinusoidal embedding is
``double(t) * double(freq_fp32)``: the frequency table stays the fp32 table the reference and the kernels read."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from localdiffusion_hallucination_amd import rng, weights
from oracle import unet_ref

import condenc_ref
from resblock_ref import reduction_bound, rel_err, uniform  # noqa: F401  (re-exported)

CONFIGS = condenc_ref.CONFIGS
KWARGS = {"mri": dict(mode="mri"), "mnist": dict(dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist"),
          "mvtec": dict(channels=3, out_dim=3, mode="mvtec")}
CASES = condenc_ref.ENCODER_CASES              # (data, B, H, W): mri (2, 8, 16), mnist (2, 12, 12), mvtec (1, 16, 8)
TIMES = {"mri": [999, 0], "mnist": [3, 417], "mvtec": [250]}


def freqs(dim, theta=10000.0):
    """The fp32 frequency table of ddpm.py:145-146, as unet_ref.time_embedding makes it."""
    half = dim // 2
    step = math.log(theta) / (half - 1)
    return torch.exp(torch.arange(half) * -step)


def time_mlp(sd, time, dim, dtype=torch.float32, p="time_mlp.", parts=None):
    """unet_ref.time_embedding's sinusoidal branch in ``dtype``; ``parts`` (a dict) receives emb and the pre-GELU h1."""
    f = freqs(dim)
    ang = time[:, None] * f[None, :] if dtype == torch.float32 else time.to(dtype)[:, None] * f.to(dtype)[None, :]
    emb = torch.cat([ang.sin(), ang.cos()], dim=-1)
    h1 = F.linear(emb, sd[p + "1.weight"], sd[p + "1.bias"])
    if parts is not None:
        parts.update(emb=emb, h1=h1)
    return F.linear(F.gelu(h1), sd[p + "3.weight"], sd[p + "3.bias"])


def unet_forward(sd, cfg, x, cond, time, dtype=torch.float32):
    """ddpm.py:404-451 on the oracle's blocks, everything in ``dtype`` (``sd``, ``x`` and ``cond`` are in it already)."""
    g, hd, dh = cfg.resnet_block_groups, cfg.attn_heads, cfg.attn_dim_head
    n_stage, fa = len(cfg.dim_mults), tuple(cfg.full_attn)

    def attn(p, t, full):
        return (unet_ref.full_attention if full else unet_ref.linear_attention)(sd, p, t, hd, dh)

    x = F.conv2d(x, sd["init_conv.weight"], sd["init_conv.bias"], padding=3)
    r = x
    temb = time_mlp(sd, time, cfg.dim, dtype)
    skips = []
    for i in range(n_stage):
        p = f"downs.{i}"
        x = unet_ref.resnet_block(sd, p + ".0", x, temb, g)
        skips.append(x)
        x = unet_ref.resnet_block(sd, p + ".1", x, temb, g)
        x = attn(p + ".2", x, fa[i]) + x
        skips.append(x)
        if i < n_stage - 1:
            x = unet_ref.pixel_unshuffle_conv(sd, p + ".3", x)
        else:
            x = F.conv2d(x, sd[p + ".3.weight"], sd[p + ".3.bias"], padding=1)
    x = unet_ref.resnet_block(sd, "mid_block1", x, temb, g)
    x = unet_ref.full_attention(sd, "mid_attn", x, hd, dh) + x
    x = unet_ref.resnet_block(sd, "mid_block2", x, temb, g)
    feat = unet_ref.cond_encoder(sd, cond, cfg.mode)
    x = unet_ref.resnet_block(sd, "conv_fusion", torch.cat([x, feat], 1), None, g)
    for j in range(n_stage):
        p = f"ups.{j}"
        x = unet_ref.resnet_block(sd, p + ".0", torch.cat([x, skips.pop()], 1), temb, g)
        x = unet_ref.resnet_block(sd, p + ".1", torch.cat([x, skips.pop()], 1), temb, g)
        x = attn(p + ".2", x, fa[n_stage - 1 - j]) + x
        if j < n_stage - 1:
            x = unet_ref.upsample_conv(sd, p + ".3", x)
        else:
            x = F.conv2d(x, sd[p + ".3.weight"], sd[p + ".3.bias"], padding=1)
    x = unet_ref.resnet_block(sd, "final_res_block", torch.cat([x, r], 1), temb, g)
    return F.conv2d(x, sd["final_conv.weight"], sd["final_conv.bias"])


# ------------------------------------------------------------------------------------------------ inputs
def state(data, seed=0):
    return OrderedDict((k, torch.from_numpy(v)) for k, v in weights.procedural_state_dict(CONFIGS[data], seed).items())


def inputs(case):
    """sd, x, cond, time, dout of one case: the procedural weights, the condition image for which no ReLU or pool tie of the
    encoder lies within the margin (condenc_ref.ENCODER_KEYS), per-sample times that differ, dout = uniform / (B H W)."""
    data, B, H, W = case
    cfg = CONFIGS[data]
    key = condenc_ref.ENCODER_KEYS[case]
    x = torch.from_numpy(rng.randn((B, cfg.channels, H, W), 7, 200 + key))
    cond = condenc_ref.encoder_input(data, B, H, W, key)
    time = torch.tensor(TIMES[data], dtype=torch.long)
    assert time.numel() == B
    return state(data), x, cond, time, condenc_ref.dout_for((B, cfg.out_dim, H, W), 50 * key + 17)


# ------------------------------------------------------------------------------------------------ the yardsticks
def leaves_of(sd, dtype):
    return OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in sd.items())


def yardstick(cfg, sd, x, cond, time, dout, dtype=torch.float64):
    """out and {parameter name: gradient of sum(out * dout), or None where the parameter is not used (conv_fusion.mlp.1.*)}."""
    leaves = leaves_of(sd, dtype)
    out = unet_forward(leaves, cfg, x.to(dtype), cond.to(dtype), time, dtype)
    grads = torch.autograd.grad(out, list(leaves.values()), grad_outputs=dout.to(dtype), allow_unused=True)
    return out.detach(), OrderedDict(zip(leaves, grads))


def time_mlp_yardstick(sd, time, dim, dtemb, dtype):
    """emb, h1, temb and the four parameter gradients of sum(temb * dtemb) of the time MLP alone (``sd`` without a prefix)."""
    leaves = leaves_of(sd, dtype)
    parts = {}
    temb = time_mlp(leaves, time, dim, dtype, p="", parts=parts)
    grads = torch.autograd.grad(temb, list(leaves.values()), grad_outputs=dtemb.to(dtype))
    return parts["emb"].detach(), parts["h1"].detach(), temb.detach(), OrderedDict(zip(leaves, grads))


def loss(model_out, x0, noise, t, sab, s1m, lw, objective, dtype):
    """ddpm.py:1186-1201: the batch mean of loss_weight[t] times the per-sample mean squared error against the target."""
    sab, s1m, lw = (v.to(dtype)[t] for v in (sab, s1m, lw))
    ext = (slice(None),) + (None,) * (x0.dim() - 1)
    x0, noise = x0.to(dtype), noise.to(dtype)
    target = noise if objective == "pred_noise" else (x0 if objective == "pred_x0" else sab[ext] * noise - s1m[ext] * x0)
    return (((model_out.to(dtype) - target) ** 2).reshape(model_out.shape[0], -1).mean(dim=1) * lw).mean()


def sgd_losses(cfg, sd, x, cond, time, x0, noise, schedule, objective, lr, steps, dtype):
    """The losses of ``steps`` plain SGD steps (p -= lr * grad) on a fixed batch, and the parameters after them."""
    leaves = leaves_of(sd, dtype)
    opt = torch.optim.SGD(list(leaves.values()), lr=lr)
    out = []
    for _ in range(steps):
        opt.zero_grad()
        value = loss(unet_forward(leaves, cfg, x.to(dtype), cond.to(dtype), time, dtype), x0, noise, time, *schedule, objective,
                     dtype)
        out.append(float(value.detach()))
        value.backward()
        opt.step()
    return out, leaves
