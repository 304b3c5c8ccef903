"""Helpers of the ResnetBlock gradient tests: procedural blocks on ``rng.uniform`` with fixed keys, and the yardstick --
``torch.autograd.grad`` through ``oracle.unet_ref.resnet_block`` (pinned bit-exact to the reference's forward by
tools/make_goldens.py) with the weight dict and the inputs cast to the dtype asked for (fp64 for the yardstick, fp32 for
eager torch's own distance to it).  CPU only."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from localdiffusion_hallucination_amd import rng, weights
from oracle import unet_ref

SEED = 4321
PREFIX = "blk"


def key_shapes(dim, dim_out, time_emb_dim):
    """The block's ``state_dict`` names and shapes from the package's restatement of the reference's key list."""
    sh = OrderedDict()
    weights._resblock(sh, PREFIX, dim, dim_out, time_emb_dim if time_emb_dim is not None else 1)
    return OrderedDict((k[len(PREFIX) + 1:], v) for k, v in sh.items() if time_emb_dim is not None or ".mlp." not in k)


def make_block(dim, dim_out, time_emb_dim=None, key=0):
    """Weights of one block (fp32 CPU tensors, state_dict names): convolution / linear weights uniform in +-1 / sqrt(fan
    in), GroupNorm weights in [0.5, 1.5), every bias in +-0.2."""
    sd = OrderedDict()
    for i, (name, shape) in enumerate(key_shapes(dim, dim_out, time_emb_dim).items()):
        k = 1000 * key + i
        if name.endswith("norm.weight"):
            v = rng.uniform(shape, SEED, k, 0.5, 1.5)
        elif name.endswith(".bias"):
            v = rng.uniform(shape, SEED, k, -0.2, 0.2)
        else:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            v = rng.uniform(shape, SEED, k, -1.0, 1.0) / fan_in ** 0.5
        sd[name] = torch.from_numpy(v).float()
    return sd


def uniform(shape, key, lo=-1.0, hi=1.0):
    return torch.from_numpy(rng.uniform(shape, SEED, 500000 + key, lo, hi))


def forward(sd, x, temb, groups=8, dtype=torch.float32):
    """The oracle's block on ``sd`` (state_dict names) in ``dtype``."""
    full = {PREFIX + "." + k: v.to(dtype) for k, v in sd.items()}
    return unet_ref.resnet_block(full, PREFIX, x.to(dtype), None if temb is None else temb.to(dtype), groups)


def yardstick(sd, x, temb, dout, groups=8, dtype=torch.float64):
    """out and {"x", "time_emb", every parameter name: gradient} of sum(out * dout), in ``dtype``."""
    leaves = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in sd.items())
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    tin = None if temb is None else temb.detach().to(dtype).clone().requires_grad_(True)
    full = {PREFIX + "." + k: v for k, v in leaves.items()}
    out = unet_ref.resnet_block(full, PREFIX, xin, tin, groups)
    names = ["x"] + ([] if tin is None else ["time_emb"]) + [k for k in leaves if tin is not None or not k.startswith("mlp.")]
    inputs = [xin] + ([] if tin is None else [tin]) + [leaves[k] for k in names if k in leaves]
    grads = torch.autograd.grad(out, inputs, grad_outputs=dout.to(dtype))
    return out.detach(), OrderedDict(zip(names, grads))


def gn_film_silu(y, gamma, beta, film, groups, dtype):
    """F.group_norm -> FiLM -> F.silu of an NCHW tensor with autograd leaves: (out, leaves dict)."""
    leaves = OrderedDict(y=y, gamma=gamma, beta=beta)
    if film is not None:
        leaves["film"] = film
    leaves = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in leaves.items())
    n = F.group_norm(leaves["y"], groups, leaves["gamma"], leaves["beta"], eps=1e-5)
    if film is not None:
        s, sh = leaves["film"][:, :, None, None].chunk(2, dim=1)
        n = n * (s + 1) + sh
    return F.silu(n), leaves


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max()) / max(1e-300, float(ref.double().abs().max()))


def reduction_bound(got, ref64, torch32, what):
    """Long reductions (test_hip_segtrain.reduction_bound's rule): rel err to the fp64 value at most max(1e-5, 4 d), d =
    fp32 eager torch's own rel err to it on the same inputs."""
    d = rel_err(torch32, ref64)
    e = rel_err(got, ref64)
    print(f"{what}: HIP rel err {e:.2e}, fp32 torch {d:.2e}, bound {max(1e-5, 4 * d):.2e}")
    assert e <= max(1e-5, 4 * d), (what, e, d)
    return e, d


def elementwise_bound(got, torch32, ref64, what, rtol=2e-5):
    """Element-wise outputs: max-abs difference to fp32 torch relative to its max-abs at most RTOL["fp32"]."""
    e = rel_err(got, torch32)
    print(f"{what}: HIP vs fp32 torch {e:.2e} (bound {rtol:.0e}); to fp64: HIP {rel_err(got, ref64):.2e}, "
          f"torch {rel_err(torch32, ref64):.2e}")
    assert e <= rtol, (what, e)
    return e
