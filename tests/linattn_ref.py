"""Helpers of the LinearAttention gradient tests: procedural weights on ``rng.uniform`` with fixed keys, and the yardstick --
``torch.autograd.grad`` through ``oracle.unet_ref.linear_attention`` / ``oracle.unet_ref.rms_norm`` with the weight dict and
the inputs cast to the dtype asked for (fp64 for the yardstick, fp32 for eager torch's own distance to it) -- plus the
attention core's formulas restated from a ``qkv`` tensor, so that ctx, (m, Z) and dctx can be looked at.  CPU only.  The
bounds are ``resblock_ref``'s."""
from collections import OrderedDict

import torch

from localdiffusion_hallucination_amd import rng, weights
from oracle import unet_ref

from resblock_ref import SEED, elementwise_bound, reduction_bound, rel_err, uniform  # noqa: F401  (re-exported)

PREFIX = "attn"
DIM_HEAD = 32


def key_shapes(dim, heads):
    """The module's ``state_dict`` names and shapes from the package's restatement of the reference's key list."""
    sh = OrderedDict()
    weights._attn(sh, PREFIX, dim, heads * DIM_HEAD, full=False)
    return OrderedDict((k[len(PREFIX) + 1:], v) for k, v in sh.items())


def make_attn(dim, heads, key=0):
    """Weights of one module (fp32 CPU tensors, state_dict names): convolution weights uniform in +-1 / sqrt(fan in), the
    RMSNorm gains in [0.5, 1.5), the bias in +-0.2."""
    sd = OrderedDict()
    for i, (name, shape) in enumerate(key_shapes(dim, heads).items()):
        k = 1000 * key + 100 + i
        if name.endswith(".g"):
            v = rng.uniform(shape, SEED, k, 0.5, 1.5)
        elif name.endswith(".bias"):
            v = rng.uniform(shape, SEED, k, -0.2, 0.2)
        else:
            v = rng.uniform(shape, SEED, k, -1.0, 1.0) / shape[1] ** 0.5
        sd[name] = torch.from_numpy(v).float()
    return sd


def forward(sd, x, heads, dtype=torch.float32):
    """The oracle's module on ``sd`` (state_dict names) in ``dtype``."""
    full = {PREFIX + "." + k: v.to(dtype) for k, v in sd.items()}
    return unet_ref.linear_attention(full, PREFIX, x.to(dtype), heads, DIM_HEAD)


def yardstick(sd, x, dout, heads, dtype=torch.float64):
    """out and {"x", every parameter name: gradient} of sum(out * dout), in ``dtype``."""
    leaves = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in sd.items())
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    out = unet_ref.linear_attention({PREFIX + "." + k: v for k, v in leaves.items()}, PREFIX, xin, heads, DIM_HEAD)
    grads = torch.autograd.grad(out, [xin] + list(leaves.values()), grad_outputs=dout.to(dtype))
    return out.detach(), OrderedDict(zip(["x"] + list(leaves), grads))


def rms(x, g, dout, dtype):
    """oracle.unet_ref.rms_norm and its gradients: dict(out, x, g)."""
    xin, gin = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, g))
    out = unet_ref.rms_norm(xin, gin.reshape(1, -1, 1, 1))
    dx, dg = torch.autograd.grad(out, [xin, gin], grad_outputs=dout.to(dtype))
    return dict(out=out.detach(), x=dx, g=dg)


def core(qkv, heads, dout, dtype):
    """The attention core of oracle.unet_ref.linear_attention (its lines between to_qkv and to_out) from qkv [B, 3 hidden,
    H, W]: dict(out, ctx [B, heads, 32, 32], m, Z [B, heads, 32]) and, with dout, dqkv and dctx by autograd."""
    leaf = qkv.detach().to(dtype).clone().requires_grad_(True)
    b, _, hh, ww = leaf.shape
    q, k, v = [t.reshape(b, heads, DIM_HEAD, hh * ww) for t in leaf.chunk(3, dim=1)]
    qs = q.softmax(dim=-2) * (DIM_HEAD ** -0.5)
    ctx = torch.einsum("bhdn,bhen->bhde", k.softmax(dim=-1), v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, qs).reshape(b, heads * DIM_HEAD, hh, ww)
    m = k.amax(dim=-1)
    res = dict(out=out.detach(), ctx=ctx.detach(), m=m.detach(), Z=(k - m[..., None]).exp().sum(dim=-1).detach())
    if dout is not None:
        res["dqkv"], res["dctx"] = torch.autograd.grad(out, [leaf, ctx], grad_outputs=dout.to(dtype))
    return res
