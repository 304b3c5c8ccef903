"""Helpers of the condition-encoder gradient tests: a torch restatement (``F.conv2d``, ``F.group_norm``, ``F.relu``,
``F.max_pool2d``) of ``BasicBlock`` and ``ResUnet`` (unet_model.py:8-51, :91-137) on a dict of tensors with the reference's
``state_dict`` names, procedural weights and inputs on ``rng.uniform`` with fixed keys, and the yardstick --
``torch.autograd.grad`` through the restatement with everything cast to the dtype asked for (fp64 for the yardstick, fp32 for
eager torch's own distance to it).  CPU only.  The bounds are ``resblock_ref``'s.

**The margin condition.**  A ReLU's gradient is a step at 0 and a pool's gradient jumps where the two largest entries of a
window meet, so a forward that is right to 1e-5 can still give a gradient that is wrong by a whole element if a
pre-activation lies within 1e-5 of 0 or a window's maximum within 1e-5 of its runner-up.  The restatement therefore reports,
per ReLU, the smallest |pre-ReLU value| and, per pool, the smallest gap between the two largest entries of any window whose
maximum is positive (a window of zeros passes its gradient to a zero of the next convolution's input either way), each
relative to that tensor's max-abs (``margins``).  The inputs of every GPU comparison of a gradient are chosen so that both
are at least ``MARGIN`` = 2e-5, twice the 1e-5 forward bound: the ``rng`` keys below were found by ``python
tests/condenc_ref.py`` (a CPU search over keys 0..; most keys do not qualify) and test_condenc_grad.py asserts the condition
for every one of them, so no element is excluded from any comparison."""
import os
import sys
from collections import OrderedDict

if __name__ == "__main__":                                  # (the search, run as a script: the package is one level up)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from localdiffusion_hallucination_amd import rng, weights

from resblock_ref import SEED, reduction_bound, rel_err, uniform  # noqa: F401  (re-exported)

GROUPS = 16
MARGIN = 2e-5
PREFIX = "blk"
CONFIGS = {"mri": weights.UnetConfig(mode="mri"), "mnist": weights.UnetConfig(mode="mnist", dim_mults=(1, 2, 4),
                                                                             full_attn=(False, False, True)),
           "mvtec": weights.UnetConfig(mode="mvtec", channels=3, out_dim=3)}

# ---- the cases of the GPU tests and the keys the search found for them (python tests/condenc_ref.py prints these tables)
# GroupNorm kernels alone: (C, ldc, B, H, W)
GN_CASES = [(C, ldc, B, H, W) for C, ldc in ((32, 64), (32, 32), (64, 64), (128, 128), (256, 256))
            for B, H, W in ((2, 5, 6), (1, 12, 12))] + [(32, 64, 1, 40, 40)]
GN_KEYS = {}            # filled below: (C, B, H, W, operands) -> key
# modules: (input_dim, mid_dim, output_dim, pool, B, H, W)
BLOCK_CASES = [(1, 32, 32, True, 2, 6, 10), (3, 32, 32, True, 1, 8, 6), (32, 32, 64, True, 2, 6, 6), (64, 64, 128, False, 2, 4, 6),
               (128, 128, 256, False, 1, 3, 5)]
BLOCK_KEYS = {}         # (input_dim, mid_dim, output_dim, pool, B, H, W) -> key
# the whole encoder on the procedural weights: (data, B, H, W)
ENCODER_CASES = [("mri", 2, 8, 16), ("mnist", 2, 12, 12), ("mvtec", 1, 16, 8)]
ENCODER_KEYS = {}       # (data, B, H, W) -> key
CHAIN_KEYS = {}         # "chain" -> key (ResUnet('mri') -> cat -> conv_fusion-sized ResnetBlock under an MSE, B = 2, 8 x 16)

# RECORDED KEYS (printed by `python tests/condenc_ref.py`, the first key of 0.. that meets the margin condition)
GN_KEYS.update({(32, 2, 5, 6, 1): 0, (32, 2, 5, 6, 2): 0, (32, 1, 12, 12, 1): 0, (32, 1, 12, 12, 2): 0, (64, 2, 5, 6, 1): 0,
                (64, 2, 5, 6, 2): 0, (64, 1, 12, 12, 1): 0, (64, 1, 12, 12, 2): 0, (128, 2, 5, 6, 1): 0, (128, 2, 5, 6, 2): 1,
                (128, 1, 12, 12, 1): 6, (128, 1, 12, 12, 2): 1, (256, 2, 5, 6, 1): 1, (256, 2, 5, 6, 2): 2, (256, 1, 12, 12, 1): 4,
                (256, 1, 12, 12, 2): 4, (32, 1, 40, 40, 1): 0, (32, 1, 40, 40, 2): 10})
BLOCK_KEYS.update({(1, 32, 32, True, 2, 6, 10): 0, (3, 32, 32, True, 1, 8, 6): 1, (32, 32, 64, True, 2, 6, 6): 1,
                   (64, 64, 128, False, 2, 4, 6): 3, (128, 128, 256, False, 1, 3, 5): 1})
# (mri: keys 8 and 10 come to 1.97e-5 and 1.99e-5 at the first block's tail, just under the 2e-5 asked for; 12 is the first)
ENCODER_KEYS.update({("mri", 2, 8, 16): 12, ("mnist", 2, 12, 12): 0, ("mvtec", 1, 16, 8): 1})
CHAIN_KEYS.update({"chain": 12})


# ------------------------------------------------------------------------------------------------ names and weights
def key_shapes(cin, cmid, cout):
    """The block's ``state_dict`` names and shapes from the package's restatement of the reference's key list."""
    sh = OrderedDict()
    weights._basic_block(sh, PREFIX, cin, cmid, cout)
    return OrderedDict((k[len(PREFIX) + 1:], v) for k, v in sh.items())


def make_block(cin, cmid, cout, key=0):
    """Weights of one block (fp32 CPU tensors, state_dict names): convolution weights uniform in +-1 / sqrt(fan in),
    GroupNorm weights in [0.5, 1.5), every bias in +-0.2."""
    sd = OrderedDict()
    for i, (name, shape) in enumerate(key_shapes(cin, cmid, cout).items()):
        k = 1000 * key + 300 + i
        if len(shape) == 1 and name.endswith(".weight"):
            v = rng.uniform(shape, SEED, k, 0.5, 1.5)
        elif name.endswith(".bias"):
            v = rng.uniform(shape, SEED, k, -0.2, 0.2)
        else:
            v = rng.uniform(shape, SEED, k, -1.0, 1.0) / (shape[1] * shape[2] * shape[3]) ** 0.5
        sd[name] = torch.from_numpy(v).float()
    return sd


def encoder_state(data, seed=0):
    """The ``cond_model.`` slice of ``weights.procedural_state_dict(CONFIGS[data], seed)``, prefix stripped, in order."""
    full = weights.procedural_state_dict(CONFIGS[data], seed)
    return OrderedDict((k[len("cond_model."):], torch.from_numpy(v)) for k, v in full.items() if k.startswith("cond_model."))


def encoder_input(data, B, H, W, key):
    """``rng.uniform((B, in_channels, H, W), 7, key, 0, 2)``: a condition image in the callers' [0, 2] window."""
    return torch.from_numpy(rng.uniform((B, CONFIGS[data].cond_in_channels, H, W), 7, key, 0.0, 2.0))


# ------------------------------------------------------------------------------------------------ the restatement
def _note(margins, kind, t, value):
    if margins is not None:
        margins.setdefault(kind, []).append(float(value) / max(1e-300, float(t.detach().abs().max())))


def relu(a, margins=None):
    _note(margins, "relu", a, a.detach().abs().min())
    return F.relu(a)


def max_pool(a, margins=None):
    if margins is not None:
        b, c, h, w = a.shape
        win = a.detach().reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, h // 2, w // 2, 4)
        top = win.sort(dim=-1, descending=True).values
        gap = (top[..., 0] - top[..., 1])[top[..., 0] > 0]
        _note(margins, "pool", a, gap.min() if gap.numel() else float("inf"))
    return F.max_pool2d(a, 2)


def gn_act(y, gamma, beta, y2=None, gamma2=None, beta2=None, act=True, margins=None):
    """act(GN(y) (+ GN(y2))), 16 groups: what ld_dn_gnr_forward computes, on NCHW tensors."""
    a = F.group_norm(y, GROUPS, gamma, beta, eps=1e-5)
    if y2 is not None:
        a = a + F.group_norm(y2, GROUPS, gamma2, beta2, eps=1e-5)
    return relu(a, margins) if act else a


def basic_block(sd, x, pool=False, p="", margins=None):
    """unet_model.py:38-51 on ``sd[p + name]`` (any dtype, autograd leaves or not), then MaxPool2d(2) when ``pool``."""
    y = F.conv2d(x, sd[p + "convblock.0.weight"], sd[p + "convblock.0.bias"], padding=1)
    y = gn_act(y, sd[p + "convblock.1.weight"], sd[p + "convblock.1.bias"], margins=margins)
    y = F.conv2d(y, sd[p + "convblock.3.weight"], sd[p + "convblock.3.bias"], padding=1)
    i = F.conv2d(x, sd[p + "identity.0.weight"], sd[p + "identity.0.bias"], padding=1)
    out = gn_act(y, sd[p + "convblock.4.weight"], sd[p + "convblock.4.bias"], i, sd[p + "identity.1.weight"],
                 sd[p + "identity.1.bias"], margins=margins)
    return max_pool(out, margins) if pool else out


def encoder(sd, x, data, margins=None):
    """unet_model.py:122-137 on a state_dict without the ``cond_model.`` prefix."""
    early = data in ("mnist", "mvtecSR")
    x = basic_block(sd, x, True, "residual_conv1.0.", margins)
    x = basic_block(sd, x, True, "residual_conv2.0.", margins)
    x = basic_block(sd, x, not early, "residual_conv3.0.", margins)
    return x if early else basic_block(sd, x, False, "mid_conv.0.", margins)


# ------------------------------------------------------------------------------------------------ the yardstick
def _grads(fn, sd, x, dout, dtype, x_grad):
    leaves = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in sd.items())
    xin = x.detach().to(dtype).clone().requires_grad_(x_grad)
    margins = {}
    out = fn(leaves, xin, margins)
    names = (["x"] if x_grad else []) + list(leaves)
    grads = torch.autograd.grad(out, ([xin] if x_grad else []) + list(leaves.values()), grad_outputs=dout.to(dtype))
    return out.detach(), OrderedDict(zip(names, grads)), {k: min(v) for k, v in margins.items()}


def yardstick(sd, x, dout, dtype=torch.float64, pool=False, data=None, x_grad=True):
    """out, {"x" (unless x_grad is False), every parameter name: gradient} of sum(out * dout), and {"relu": the smallest
    relative |pre-ReLU value|, "pool": the smallest relative gap at the top of a pool window}, in ``dtype``: of the block
    (``sd`` a block's state_dict, ``pool``) or, with ``data``, of the whole encoder (``sd`` without the ``cond_model.``
    prefix)."""
    if data is not None:
        return _grads(lambda l, xin, mg: encoder(l, xin, data, mg), sd, x, dout, dtype, x_grad)
    return _grads(lambda l, xin, mg: basic_block(l, xin, pool, "", mg), sd, x, dout, dtype, x_grad)


def out_shape(sd, x, pool=False, data=None):
    with torch.no_grad():
        return tuple((encoder(sd, x, data) if data is not None else basic_block(sd, x, pool)).shape)


def dout_for(shape, key):
    return uniform(shape, key) / (shape[0] * shape[2] * shape[3])


# ---- the inputs of each kind of case, as functions of the key the search varies
def gn_inputs(C, B, H, W, nop, key):
    """y (and y2), gamma(s) in [0.5, 1.5), beta(s) in +-0.2, dout = uniform / (B H W) of one GroupNorm case."""
    t = OrderedDict(y=uniform((B, C, H, W), 10 * key + 1, -2.0, 2.0), gamma=uniform((C,), 10 * key + 2, 0.5, 1.5),
                    beta=uniform((C,), 10 * key + 3, -0.2, 0.2))
    if nop == 2:
        t.update(y2=uniform((B, C, H, W), 10 * key + 4, -1.0, 3.0), gamma2=uniform((C,), 10 * key + 5, 0.5, 1.5),
                 beta2=uniform((C,), 10 * key + 6, -0.2, 0.2))
    return t, dout_for((B, C, H, W), 10 * key + 7)


def gn_yardstick(t, dout, act, dtype):
    """out and the gradient of every entry of ``t`` of sum(act(GN(y) (+ GN(y2))) * dout), and the ReLU margin."""
    leaves = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in t.items())
    margins = {}
    out = gn_act(*leaves.values(), act=act, margins=margins)
    grads = torch.autograd.grad(out, list(leaves.values()), grad_outputs=dout.to(dtype))
    return out.detach(), OrderedDict(zip(leaves, grads)), {k: min(v) for k, v in margins.items()}


def gn_stats(y, dtype=torch.float64):
    """[B, 16, 2] = (mean, 1 / sqrt(biased var + 1e-5)) of an NCHW tensor: what ld_dn_gnr_forward writes to stat."""
    g = y.to(dtype).reshape(y.shape[0], GROUPS, -1)
    return torch.stack([g.mean(-1), (g.var(-1, unbiased=False) + 1e-5).rsqrt()], dim=-1)


def block_inputs(case, key):
    cin, cmid, cout, pool, B, H, W = case
    sd = make_block(cin, cmid, cout, key=key)
    x = uniform((B, cin, H, W), 20 * key + 11, 0.0 if cin <= 4 else -1.0, 2.0 if cin <= 4 else 1.0)
    return sd, x, dout_for(out_shape(sd, x, pool), 20 * key + 12)


def encoder_inputs(case, key):
    data, B, H, W = case
    sd = encoder_state(data)
    x = encoder_input(data, B, H, W, key)
    return sd, x, dout_for(out_shape(sd, x, data=data), 30 * key + 13)


def im2col3(x, ldk):
    """NCHW [B, Cin, H, W] -> [B, H, W, ldk]: F.unfold(x, 3, padding=1) rearranged (column (ci 3 + ky) 3 + kx), zero behind."""
    b, c, h, w = x.shape
    cols = F.unfold(x, 3, padding=1).reshape(b, 9 * c, h, w).permute(0, 2, 3, 1)
    out = torch.zeros(b, h, w, ldk, dtype=x.dtype)
    out[..., :9 * c] = cols
    return out


# ------------------------------------------------------------------------------------------------ the chain case
def chain_inputs(key):
    """ResUnet('mri') on a [2, 1, 8, 16] image -> feat [2, 256, 1, 2]; cat(feat', feat) with feat' a fixed tensor ->
    ResnetBlock(512, 256) (conv_fusion's shape, no time embedding) -> MSE against a fixed target."""
    import resblock_ref
    sd, x = encoder_state("mri"), encoder_input("mri", 2, 8, 16, key)
    blk = resblock_ref.make_block(512, 256, None, key=77)
    other, target = uniform((2, 256, 1, 2), 40 * key + 21), uniform((2, 256, 1, 2), 40 * key + 22)
    return sd, blk, x, other, target


def chain_yardstick(sd, blk, x, other, target, dtype):
    """{encoder parameter name: gradient} of mse(ResnetBlock(cat(other, encoder(x))), target) and the encoder's margins."""
    from oracle import unet_ref
    leaves = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in sd.items())
    margins = {}
    feat = encoder(leaves, x.to(dtype), "mri", margins)
    full = {"a." + k: v.to(dtype) for k, v in blk.items()}
    out = unet_ref.resnet_block(full, "a", torch.cat((other.to(dtype), feat), dim=1), None)
    loss = F.mse_loss(out, target.to(dtype))
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return float(loss.detach()), OrderedDict(zip(leaves, grads)), {k: min(v) for k, v in margins.items()}


# ------------------------------------------------------------------------------------------------ the search
def margins_ok(m):
    return all(v >= MARGIN for v in m.values())


def _first_key(margin_of, limit=400):
    for key in range(limit):
        if margins_ok(margin_of(key)):
            return key
    raise RuntimeError("no key below %d meets the margin condition" % limit)


def search():
    """The first key of each case that meets the margin condition under the fp64 yardstick; prints the tables recorded above."""
    F64 = torch.float64
    gn = OrderedDict()
    for C, _, B, H, W in GN_CASES:
        for nop in (1, 2):
            if (C, B, H, W, nop) not in gn:
                gn[(C, B, H, W, nop)] = _first_key(lambda k: gn_yardstick(*gn_inputs(C, B, H, W, nop, k), True, F64)[2])
    blocks = OrderedDict((c, _first_key(lambda k: yardstick(*block_inputs(c, k), F64, pool=c[3], x_grad=c[0] > 4)[2]))
                         for c in BLOCK_CASES)
    enc = OrderedDict((c, _first_key(lambda k: yardstick(*encoder_inputs(c, k), F64, data=c[0], x_grad=False)[2]))
                      for c in ENCODER_CASES)
    chain = {"chain": _first_key(lambda k: chain_yardstick(*chain_inputs(k), F64)[2])}
    for name, table in (("GN_KEYS", gn), ("BLOCK_KEYS", blocks), ("ENCODER_KEYS", enc), ("CHAIN_KEYS", chain)):
        print(f"{name}.update({dict(table)!r})")


if __name__ == "__main__":
    search()
