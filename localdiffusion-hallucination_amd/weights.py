"""Parameter inventory and procedural weights for the conditional denoiser.

The parameter names and shapes reproduce the ``state_dict`` of the reference ``Unet``
(/root/reference/ddpm.py:286-398) including its ``ResUnet`` conditioning encoder
(/root/reference/unet_model.py:91-116), so that real checkpoints written by the reference's
``Trainer.save`` (/root/reference/ddpm.py:1495-1507) load by name.  No checkpoint ships with the
reference, so tests/bench use *procedural* weights: every tensor is a pure function of its
parameter name and a seed (see ``procedural_state_dict``), regenerated identically in the build
container (golden generation) and on the GPU box.
"""
from collections import OrderedDict
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import rng


@dataclass(frozen=True)
class UnetConfig:
    """Constructor arguments of the reference Unet that change the parameter set
    (/root/reference/ddpm.py:287-307)."""
    dim: int = 32
    init_dim: int = 32
    out_dim: int = 1
    dim_mults: Tuple[int, ...] = (1, 2, 4, 8)
    channels: int = 1
    resnet_block_groups: int = 8
    attn_dim_head: int = 32
    attn_heads: int = 4
    full_attn: Tuple[bool, ...] = (False, False, False, True)
    mode: str = "mri"
    learned_sinusoidal_dim: int = 0       # > 0: RandomOrLearnedSinusoidalPosEmb of that dim instead of SinusoidalPosEmb (ddpm.py:330-337)

    @property
    def dims(self):
        return [self.init_dim] + [self.dim * m for m in self.dim_mults]

    @property
    def in_out(self):
        d = self.dims
        return list(zip(d[:-1], d[1:]))

    @property
    def time_dim(self):
        return self.dim * 4

    @property
    def fourier_dim(self):
        # ddpm.py:332-337: learned / random Fourier features are [t, sin, cos] (dim + 1), the sinusoidal embedding is `dim` wide
        return self.learned_sinusoidal_dim + 1 if self.learned_sinusoidal_dim else self.dim

    @property
    def hidden(self):
        return self.attn_dim_head * self.attn_heads

    @property
    def cond_in_channels(self):
        # /root/reference/unet_model.py:94-99
        if "mvtecGray" in self.mode:
            return 1
        if "mvtec" in self.mode:
            return 3
        return 1

    @property
    def cond_has_mid(self):
        # /root/reference/unet_model.py:113-115 (module exists) ...
        return self.mode in ("mri", "mvtec", "mvtecGray")

    @property
    def cond_early_exit(self):
        # ... /root/reference/unet_model.py:131-132 (forward returns after level 3)
        return self.mode in ("mnist", "mvtecSR")

    @property
    def downsample_factor(self):
        return 2 ** (len(self.dim_mults) - 1)


def _conv(sh, name, cout, cin, k, bias=True):
    sh[name + ".weight"] = (cout, cin, k, k)
    if bias:
        sh[name + ".bias"] = (cout,)


def _gn(sh, name, c):
    sh[name + ".weight"] = (c,)
    sh[name + ".bias"] = (c,)


def _resblock(sh, p, cin, cout, tdim):
    sh[p + ".mlp.1.weight"] = (2 * cout, tdim)
    sh[p + ".mlp.1.bias"] = (2 * cout,)
    _conv(sh, p + ".block1.proj", cout, cin, 3)
    _gn(sh, p + ".block1.norm", cout)
    _conv(sh, p + ".block2.proj", cout, cout, 3)
    _gn(sh, p + ".block2.norm", cout)
    if cin != cout:
        _conv(sh, p + ".res_conv", cout, cin, 1)


def _attn(sh, p, c, hidden, full):
    sh[p + ".norm.g"] = (1, c, 1, 1)
    sh[p + ".to_qkv.weight"] = (3 * hidden, c, 1, 1)
    if full:
        _conv(sh, p + ".to_out", c, hidden, 1)
    else:
        _conv(sh, p + ".to_out.0", c, hidden, 1)
        sh[p + ".to_out.1.g"] = (1, c, 1, 1)


def _basic_block(sh, p, cin, cmid, cout):
    _conv(sh, p + ".convblock.0", cmid, cin, 3)
    _gn(sh, p + ".convblock.1", cmid)
    _conv(sh, p + ".convblock.3", cout, cmid, 3)
    _gn(sh, p + ".convblock.4", cout)
    if cin != cout:
        _conv(sh, p + ".identity.0", cout, cin, 3)
        _gn(sh, p + ".identity.1", cout)


def unet_param_shapes(cfg: UnetConfig) -> "OrderedDict[str, tuple]":
    """name -> shape, in the reference's registration order."""
    sh = OrderedDict()
    f = [32, 32, 64, 128, 256]                    # unet_model.py:100
    _basic_block(sh, "cond_model.residual_conv1.0", cfg.cond_in_channels, f[0], f[1])
    _basic_block(sh, "cond_model.residual_conv2.0", f[1], f[1], f[2])
    _basic_block(sh, "cond_model.residual_conv3.0", f[2], f[2], f[3])
    if cfg.cond_has_mid:
        _basic_block(sh, "cond_model.mid_conv.0", f[3], f[3], f[4])
    _conv(sh, "init_conv", cfg.init_dim, cfg.channels, 7)
    td = cfg.time_dim
    if cfg.learned_sinusoidal_dim:
        sh["time_mlp.0.weights"] = (cfg.learned_sinusoidal_dim // 2,)            # ddpm.py:158 (requires_grad only differs)
    sh["time_mlp.1.weight"] = (td, cfg.fourier_dim)
    sh["time_mlp.1.bias"] = (td,)
    sh["time_mlp.3.weight"] = (td, td)
    sh["time_mlp.3.bias"] = (td,)
    io = cfg.in_out
    n = len(io)
    for i, (cin, cout) in enumerate(io):
        p = f"downs.{i}"
        _resblock(sh, p + ".0", cin, cin, td)
        _resblock(sh, p + ".1", cin, cin, td)
        _attn(sh, p + ".2", cin, cfg.hidden, cfg.full_attn[i])
        if i < n - 1:
            _conv(sh, p + ".3.1", cout, cin * 4, 1)
        else:
            _conv(sh, p + ".3", cout, cin, 3)
    for j, ((cin, cout), full) in enumerate(zip(reversed(io), reversed(cfg.full_attn))):
        p = f"ups.{j}"
        _resblock(sh, p + ".0", cout + cin, cout, td)
        _resblock(sh, p + ".1", cout + cin, cout, td)
        _attn(sh, p + ".2", cout, cfg.hidden, full)
        if j < n - 1:
            _conv(sh, p + ".3.1", cin, cout, 3)
        else:
            _conv(sh, p + ".3", cin, cout, 3)
    mid = cfg.dims[-1]
    _resblock(sh, "mid_block1", mid, mid, td)
    _attn(sh, "mid_attn", mid, cfg.hidden, True)
    _resblock(sh, "mid_block2", mid, mid, td)
    _resblock(sh, "conv_fusion", 2 * mid, mid, td)
    _resblock(sh, "final_res_block", 2 * cfg.dim, cfg.dim, td)
    _conv(sh, "final_conv", cfg.out_dim, cfg.dim, 1)
    return sh


def _fan_in(shape):
    if len(shape) >= 2:
        return int(np.prod(shape[1:]))
    return None


def procedural_tensor(name, shape, seed=0):
    """One parameter tensor as a pure function of (name, seed).

    conv / linear weights and biases: uniform(+-1/sqrt(fan_in)) (bias uses its layer's fan_in);
    GroupNorm gamma = 1 + 0.1 u, beta = 0.1 u;  RMSNorm g = 1 + 0.1 u  (u uniform in [-1, 1)).
    ``final_conv`` is re-centred (bias ~ 1, 3x weights) so that the predicted x0 lives inside the
    [0, 2] clamp window used by the reference's callers (test.py:30-37) instead of saturating.
    """
    key = rng.fnv1a64(name)
    u = rng.uniform(shape, seed, key, -1.0, 1.0)
    if name.endswith(".g"):
        return (1.0 + 0.1 * u).astype(np.float32)
    return u


def procedural_state_dict(cfg: UnetConfig, seed=0, final_gain=3.0):
    """``final_gain``: scale of ``final_conv.weight`` over its fan-in bound.  3.0 (the default every fixture but G16 uses)
    makes a random-init denoiser whose prediction swings over the whole [0, 2] range and whose last 100 reverse steps
    amplify any perturbation x40-70; a small gain makes the chain CONTRACTIVE there, like a trained denoiser whose
    prediction at small t stays near x_t (golden G16: the end-to-end pin of the 16-bit storage modes)."""
    shapes = unet_param_shapes(cfg)
    out = OrderedDict()
    for name, shape in shapes.items():
        u = procedural_tensor(name, shape, seed)
        is_norm = (".norm." in name and not name.endswith(".g")) or \
                  ("convblock.1." in name) or ("convblock.4." in name) or ("identity.1." in name)
        if name.endswith(".g") or name.endswith(".weights"):      # (.weights: the Fourier frequencies, any O(1) values)
            t = u
        elif is_norm:
            t = (1.0 + 0.1 * u) if name.endswith(".weight") else (0.1 * u)
        else:
            if name.endswith(".weight"):
                bound = 1.0 / np.sqrt(_fan_in(shape))
            else:
                wshape = shapes[name[:-len(".bias")] + ".weight"]
                bound = 1.0 / np.sqrt(_fan_in(wshape))
            t = u * bound
            if name == "final_conv.weight":
                t = t * float(final_gain)
            if name == "final_conv.bias":
                t = 1.0 + t
        out[name] = np.ascontiguousarray(t, dtype=np.float32)
    return out


def num_params(cfg: UnetConfig):
    return sum(int(np.prod(s)) for s in unet_param_shapes(cfg).values())


# ----------------------------------------------------------------------------- segmentation U-Net (mask producer)
SEG_WIDTHS = (64, 128, 256, 512, 1024)      # inc, down1..down4 of unet_model.py:222-229 (bilinear=False)
_BN_BUFFERS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _double_conv_shapes(sh, p, cin, cout):
    sh[p + "double_conv.0.weight"] = (cout, cin, 3, 3)
    for k in _BN_BUFFERS:
        sh[p + "double_conv.1." + k] = () if k == "num_batches_tracked" else (cout,)
    sh[p + "double_conv.3.weight"] = (cout, cout, 3, 3)
    for k in _BN_BUFFERS:
        sh[p + "double_conv.4." + k] = () if k == "num_batches_tracked" else (cout,)


def seg_param_shapes(n_channels=1, n_classes=1) -> "OrderedDict[str, tuple]":
    """name -> shape of ``unet_model.UNet(n_channels, n_classes, bilinear=False).state_dict()`` in its order (118 entries
    for one class): DoubleConv = conv3x3 (no bias) + BatchNorm2d, twice; Up = ConvTranspose2d(2, 2) + DoubleConv."""
    w = SEG_WIDTHS
    sh = OrderedDict()
    _double_conv_shapes(sh, "inc.", n_channels, w[0])
    for i in range(1, 5):
        _double_conv_shapes(sh, f"down{i}.maxpool_conv.1.", w[i - 1], w[i])
    for i in range(1, 5):
        cin = w[5 - i]
        sh[f"up{i}.up.weight"] = (cin, cin // 2, 2, 2)
        sh[f"up{i}.up.bias"] = (cin // 2,)
        _double_conv_shapes(sh, f"up{i}.conv.", cin, cin // 2)
    sh["outc.conv.weight"] = (n_classes, w[0], 1, 1)
    sh["outc.conv.bias"] = (n_classes,)
    return sh


def procedural_seg_state_dict(seed=0, bn_stats=None, n_channels=1, n_classes=1):
    """Name-keyed procedural weights of the segmentation U-Net (numpy, the reference's names and dtypes):
    convolutions uniform(+-1/sqrt(fan_in)) (a ConvTranspose2d(2, 2) output sees Cin inputs: bound 1/sqrt(Cin), its bias
    too), BatchNorm gamma = 1 + 0.1 u, beta = 0.1 u.  The running statistics are NOT invented: ``bn_stats`` maps
    ``<bn>.running_mean`` / ``.running_var`` / ``.num_batches_tracked`` -- and any other name it holds, such as the
    head bias G18 places in a gap of its logits -- to the values a calibration produced (tests/golden/g18_segunet.npz);
    without it they are the fresh-module values 0 / 1 / 0."""
    shapes = seg_param_shapes(n_channels, n_classes)
    out = OrderedDict()
    for name, shape in shapes.items():
        if bn_stats is not None and name in bn_stats:
            t = np.asarray(bn_stats[name])
            if name.endswith("num_batches_tracked"):
                out[name] = np.asarray(t, dtype=np.int64).reshape(())
            else:
                out[name] = np.ascontiguousarray(t, dtype=np.float32).reshape(shape)
            continue
        if name.endswith("num_batches_tracked"):
            out[name] = np.asarray(0, dtype=np.int64)
            continue
        if name.endswith("running_mean"):
            out[name] = np.zeros(shape, np.float32)
            continue
        if name.endswith("running_var"):
            out[name] = np.ones(shape, np.float32)
            continue
        u = procedural_tensor("seg." + name, shape, seed)
        if ".double_conv.1." in name or ".double_conv.4." in name:
            t = (1.0 + 0.1 * u) if name.endswith(".weight") else 0.1 * u
        elif ".up." in name:
            cin = shapes[name[:-len(".bias")] + ".weight"][0] if name.endswith(".bias") else shape[0]
            t = u / np.sqrt(cin)
        else:
            wshape = shapes[name[:-len(".bias")] + ".weight"] if name.endswith(".bias") else shape
            t = u / np.sqrt(_fan_in(wshape))
        out[name] = np.ascontiguousarray(t, dtype=np.float32)
    return out


# ----------------------------------------------------------------------------- MNIST digit classifier (SimpleCNN)
def mnistcls_param_shapes() -> "OrderedDict[str, tuple]":
    """name -> shape of ``SimpleCNN().state_dict()`` (train_mnist_cls.py:31-47) in its order."""
    return OrderedDict([("conv1.weight", (32, 1, 3, 3)), ("conv1.bias", (32,)), ("conv2.weight", (64, 32, 3, 3)),
                        ("conv2.bias", (64,)), ("fc1.weight", (128, 64 * 7 * 7)), ("fc1.bias", (128,)),
                        ("fc2.weight", (10, 128)), ("fc2.bias", (10,))])


def procedural_mnistcls_state_dict(seed=0):
    """Name-keyed procedural weights of the digit classifier (numpy fp32): uniform(+-1/sqrt(fan_in)) for weights and
    biases alike, PyTorch's default bounds for ``nn.Conv2d`` / ``nn.Linear``, without any torch RNG."""
    shapes = mnistcls_param_shapes()
    out = OrderedDict()
    for name, shape in shapes.items():
        wshape = shapes[name[:-len(".bias")] + ".weight"] if name.endswith(".bias") else shape
        u = procedural_tensor("mnistcls." + name, shape, seed)
        out[name] = np.ascontiguousarray(u / np.sqrt(_fan_in(wshape)), dtype=np.float32)
    return out


# ----------------------------------------------------------------------------- PatchCore backbone (wide_resnet50_2)
PC_STAGES = (("layer1", 3, 128, 256, 1), ("layer2", 4, 256, 512, 2), ("layer3", 6, 512, 1024, 2))  # blocks, width, out, stride


def _bn_shapes(sh, p, c):
    for k in _BN_BUFFERS:
        sh[p + k] = () if k == "num_batches_tracked" else (c,)


def patchcore_param_shapes() -> "OrderedDict[str, tuple]":
    """name -> shape of the torchvision / timm ``wide_resnet50_2`` state_dict up to layer3, in its order (what timm's
    ``features_only`` trunk for layers 2 and 3 keeps: conv1, bn1, layer1..3; layer4 and fc are not used)."""
    sh = OrderedDict()
    sh["conv1.weight"] = (64, 3, 7, 7)
    _bn_shapes(sh, "bn1.", 64)
    cin = 64
    for name, blocks, width, cout, _ in PC_STAGES:
        for i in range(blocks):
            p = f"{name}.{i}."
            sh[p + "conv1.weight"] = (width, cin, 1, 1)
            _bn_shapes(sh, p + "bn1.", width)
            sh[p + "conv2.weight"] = (width, width, 3, 3)
            _bn_shapes(sh, p + "bn2.", width)
            sh[p + "conv3.weight"] = (cout, width, 1, 1)
            _bn_shapes(sh, p + "bn3.", cout)
            if i == 0:
                sh[p + "downsample.0.weight"] = (cout, cin, 1, 1)
                _bn_shapes(sh, p + "downsample.1.", cout)
            cin = cout
    return sh


def procedural_patchcore_state_dict(seed=0, calib_size=48, calib_batch=2):
    """Name-keyed procedural ``wide_resnet50_2`` trunk weights (numpy, torchvision's names): convolutions
    uniform(+-sqrt(3 / fan_in)) (unit gain), BatchNorm gamma = 1 + 0.1 u, beta = 0.1 u, except the residual branches'
    last BatchNorm (bn3), which is scaled by 1/4 so the residual stream does not grow block by block.  The statistics are
    calibrated: a procedural ImageNet-normalised batch [calib_batch, 3, calib_size, calib_size] goes through the trunk in
    eval order on the CPU, and each BatchNorm gets its input's per-channel batch mean and (biased) variance, so the
    activations stay O(1) through layer3.  num_batches_tracked = 1."""
    import torch
    import torch.nn.functional as F
    shapes = patchcore_param_shapes()
    out = OrderedDict()
    for name, shape in shapes.items():
        if name.endswith(("running_mean", "running_var", "num_batches_tracked")):
            continue
        u = procedural_tensor("pc." + name, shape, seed)
        if len(shape) == 4:
            t = u * np.sqrt(3.0 / _fan_in(shape))
        else:
            t = (1.0 + 0.1 * u) if name.endswith(".weight") else 0.1 * u
            if ".bn3." in name:
                t = 0.25 * t
        out[name] = np.ascontiguousarray(t, dtype=np.float32)
    x = torch.from_numpy(rng.uniform((calib_batch, 3, calib_size, calib_size), seed, 7001, -2.0, 2.0))

    def conv_bn(x, p_conv, p_bn, stride=1, pad=0, relu=True):
        y = F.conv2d(x, torch.from_numpy(out[p_conv]), stride=stride, padding=pad)
        mean, var = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
        out[p_bn + "running_mean"] = mean.numpy().astype(np.float32)
        out[p_bn + "running_var"] = var.numpy().astype(np.float32)
        out[p_bn + "num_batches_tracked"] = np.asarray(1, dtype=np.int64)
        y = F.batch_norm(y, mean, var, torch.from_numpy(out[p_bn + "weight"]), torch.from_numpy(out[p_bn + "bias"]),
                         False, 0.0, 1e-5)
        return F.relu(y) if relu else y

    with torch.no_grad():
        x = conv_bn(x.float(), "conv1.weight", "bn1.", 2, 3)
        x = F.max_pool2d(x, 3, 2, 1)
        for name, blocks, _, _, stride in PC_STAGES:
            for i in range(blocks):
                p, s = f"{name}.{i}.", (stride if i == 0 else 1)
                idn = conv_bn(x, p + "downsample.0.weight", p + "downsample.1.", s, 0, False) if i == 0 else x
                y = conv_bn(x, p + "conv1.weight", p + "bn1.")
                y = conv_bn(y, p + "conv2.weight", p + "bn2.", s, 1)
                y = conv_bn(y, p + "conv3.weight", p + "bn3.", relu=False)
                x = F.relu(y + idn)
    return OrderedDict((k, out[k]) for k in shapes)
