"""Helpers of the Downsample / Upsample / Conv2d gradient tests: procedural weights on ``rng.uniform`` with fixed keys in
``resblock_ref.make_block``'s manner (key names checked against ``weights.unet_param_shapes``), and the yardstick --
``torch.autograd.grad`` through ``oracle.unet_ref.pixel_unshuffle_conv``, ``oracle.unet_ref.upsample_conv`` and ``F.conv2d``
with the weights and the input cast to the dtype asked for (fp64 for the yardstick, fp32 for eager torch's own distance to
it) -- plus the torch restatements of the layout kernels.  CPU only.  The bounds are ``resblock_ref``'s."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from localdiffusion_hallucination_amd import rng, weights
from oracle import unet_ref

from resblock_ref import SEED, reduction_bound, rel_err, uniform  # noqa: F401  (re-exported)

PREFIX = "lay"
KINDS = ("down", "up", "conv3", "stem", "head")
CFG = weights.UnetConfig(dim=32, init_dim=32, out_dim=3, channels=3, mode="mvtec")     # cfg3's parameter set
# the five layers in a cfg3-like Unet: (kind, cin, cout) under the reference's state_dict prefix
IN_UNET = {"downs.0.3": ("down", 32, 32), "ups.0.3": ("up", 256, 128), "downs.3.3": ("conv3", 128, 256),
           "init_conv": ("stem", 3, 32), "final_conv": ("head", 32, 3)}


def key_shapes(kind, cin, cout):
    """The layer's ``state_dict`` names and shapes from the package's restatement of the reference's key list."""
    sh = OrderedDict()
    if kind == "down":
        weights._conv(sh, PREFIX + ".1", cout, 4 * cin, 1)
    elif kind == "up":
        weights._conv(sh, PREFIX + ".1", cout, cin, 3)
    else:
        weights._conv(sh, PREFIX, cout, cin, {"conv3": 3, "stem": 7, "head": 1}[kind])
    return OrderedDict((k[len(PREFIX) + 1:], v) for k, v in sh.items())


def make_layer(kind, cin, cout, key=0):
    """Weights of one layer (fp32 CPU tensors, state_dict names): the weight uniform in +-1 / sqrt(fan in), the bias in
    +-0.2."""
    sd = OrderedDict()
    for i, (name, shape) in enumerate(key_shapes(kind, cin, cout).items()):
        k = 1000 * key + 200 + i
        if name.endswith("bias"):
            v = rng.uniform(shape, SEED, k, -0.2, 0.2)
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            v = rng.uniform(shape, SEED, k, -1.0, 1.0) / fan_in ** 0.5
        sd[name] = torch.from_numpy(v).float()
    return sd


def apply(kind, sd, x):
    """The layer on a dict of tensors with state_dict names (any dtype, autograd leaves or not)."""
    if kind == "down":
        return unet_ref.pixel_unshuffle_conv({PREFIX + "." + k: v for k, v in sd.items()}, PREFIX, x)
    if kind == "up":
        return unet_ref.upsample_conv({PREFIX + "." + k: v for k, v in sd.items()}, PREFIX, x)
    return F.conv2d(x, sd["weight"], sd["bias"], padding={"conv3": 1, "stem": 3, "head": 0}[kind])


def forward(kind, sd, x, dtype=torch.float32):
    return apply(kind, {k: v.to(dtype) for k, v in sd.items()}, x.to(dtype))


def yardstick(kind, sd, x, dout, dtype=torch.float64, x_grad=True):
    """out and {"x" (unless x_grad is False: the stem), every parameter name: gradient} of sum(out * dout), in ``dtype``."""
    leaves = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in sd.items())
    xin = x.detach().to(dtype).clone().requires_grad_(x_grad)
    out = apply(kind, leaves, xin)
    names = (["x"] if x_grad else []) + list(leaves)
    grads = torch.autograd.grad(out, ([xin] if x_grad else []) + list(leaves.values()), grad_outputs=dout.to(dtype))
    return out.detach(), OrderedDict(zip(names, grads))


# ------------------------------------------------------------------------------------------------ the layout kernels in torch
def space_to_depth(x):
    """NCHW [B, C, 2H, 2W] -> NHWC [B, H, W, 4 C] with channel (p1 2 + p2) C + c: ld_dn_space_to_depth's order."""
    b, c, h, w = x.shape
    return x.reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(b, h // 2, w // 2, 4 * c).contiguous()


def depth_to_space(g, c):
    """NHWC [B, H, W, 4 C] -> NCHW [B, C, 2H, 2W]: the inverse."""
    b, h, w, _ = g.shape
    return g.reshape(b, h, w, 2, 2, c).permute(0, 5, 1, 3, 2, 4).reshape(b, c, 2 * h, 2 * w).contiguous()


def upsample2x(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def window_sum(g):
    """NCHW [B, C, 2H, 2W] -> [B, C, H, W], the four terms added in ld_dn_upsample2x_backward's documented order."""
    return ((g[:, :, 0::2, 0::2] + g[:, :, 0::2, 1::2]) + g[:, :, 1::2, 0::2]) + g[:, :, 1::2, 1::2]


def im2col(x, ldk):
    """NCHW [B, Cin, H, W] -> [B, H, W, ldk]: F.unfold(x, 7, padding=3) rearranged (column (ci 7 + ky) 7 + kx), zero behind."""
    b, c, h, w = x.shape
    cols = F.unfold(x, 7, padding=3).reshape(b, 49 * c, h, w).permute(0, 2, 3, 1)
    out = torch.zeros(b, h, w, ldk, dtype=x.dtype)
    out[..., :49 * c] = cols
    return out
