"""Helpers of the full-Attention gradient tests: procedural weights on ``rng.uniform`` with fixed keys, and the yardstick --
``torch.autograd.grad`` through ``oracle.unet_ref.full_attention`` with the weight dict and the inputs cast to the dtype
asked for (fp64 for the yardstick, fp32 for eager torch's own distance to it) -- plus the lines between ``to_qkv`` and
``to_out`` restated from a ``qkv`` tensor, so that out, lse and dqkv can be looked at.  CPU only.  The bounds are
``resblock_ref``'s."""
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
    weights._attn(sh, PREFIX, dim, heads * DIM_HEAD, full=True)
    return OrderedDict((k[len(PREFIX) + 1:], v) for k, v in sh.items())


def make_attn(dim, heads, key=0):
    """Weights of one module (fp32 CPU tensors, state_dict names): convolution weights uniform in +-1 / sqrt(fan in), the
    RMSNorm gain in [0.5, 1.5), the bias in +-0.2."""
    sd = OrderedDict()
    for i, (name, shape) in enumerate(key_shapes(dim, heads).items()):
        k = 1000 * key + 200 + i
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
    return unet_ref.full_attention(full, PREFIX, x.to(dtype), heads, DIM_HEAD)


def yardstick(sd, x, dout, heads, dtype=torch.float64):
    """out and {"x", every parameter name: gradient} of sum(out * dout), in ``dtype``."""
    leaves = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in sd.items())
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    out = unet_ref.full_attention({PREFIX + "." + k: v for k, v in leaves.items()}, PREFIX, xin, heads, DIM_HEAD)
    grads = torch.autograd.grad(out, [xin] + list(leaves.values()), grad_outputs=dout.to(dtype))
    return out.detach(), OrderedDict(zip(["x"] + list(leaves), grads))


def core(qkv, heads, dout, dtype):
    """The lines of oracle.unet_ref.full_attention between to_qkv and to_out from qkv [B, 3 hidden, H, W]: dict(out [B,
    hidden, H, W], lse [B, heads, n] = logsumexp of the scaled logits over the keys) and, with dout, dqkv by autograd."""
    leaf = qkv.detach().to(dtype).clone().requires_grad_(True)
    b, _, hh, ww = leaf.shape
    q, k, v = [t.reshape(b, heads, DIM_HEAD, hh * ww).transpose(-1, -2) for t in leaf.chunk(3, dim=1)]
    sim = torch.einsum("bhid,bhjd->bhij", q, k) * (DIM_HEAD ** -0.5)
    att = sim.softmax(dim=-1)
    out = torch.einsum("bhij,bhjd->bhid", att, v)
    out = out.transpose(-1, -2).reshape(b, heads * DIM_HEAD, hh, ww)
    res = dict(out=out.detach(), lse=torch.logsumexp(sim.detach(), dim=-1))
    if dout is not None:
        (res["dqkv"],) = torch.autograd.grad(out, [leaf], grad_outputs=dout.to(dtype))
    return res
