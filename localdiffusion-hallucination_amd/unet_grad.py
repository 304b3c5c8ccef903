"""The time MLP and a trainable ``Unet`` (ddpm.py:286-451) on HIP kernels: the sixth slice of the denoiser's backward pass.

``TimeMLP(dim, theta=10000)`` is the reference's ``time_mlp`` -- ``SinusoidalPosEmb`` -> ``Linear(dim, 4 dim)`` -> ``GELU`` ->
``Linear(4 dim, 4 dim)`` -- with the reference's ``state_dict`` names (``1.weight``, ``1.bias``, ``3.weight``, ``3.bias``; the
embedding has no parameter, so there is no index 0): one ``autograd.Function`` over ``ld_dn_time_mlp_forward`` /
``ld_dn_time_mlp_backward`` (``csrc/unet_grad.hip``).  The forward keeps the embedding and the pre-GELU value; the frequency
table is made on the host exactly as ``unet.py`` makes it for the inference kernel and lives in a non-persistent buffer.

``TrainableUnet`` assembles ``Conv2d``, ``TimeMLP``, ``ResnetBlock``, ``LinearAttention``, ``Attention``, ``Downsample``,
``Upsample`` and ``ResUnet`` the way the reference's constructor does, so that its ``state_dict`` is, in names, shapes and
order, ``weights.unet_param_shapes(cfg)``: the inference ``Unet`` and a reference checkpoint load into it and back.  Its forward
is ddpm.py:404-451 line for line.  The glue between the blocks -- the two concatenations per up stage, the one with the
condition features, the one with ``r``, and every ``attn(x) + x`` -- is ``ld_dn_join`` on the padded NHWC tensors behind a
small ``autograd.Function`` whose backward hands out views of ``dout``: no module writes into the ``dout`` it is given (each
either reads it in place or repacks it), so autograd may hand one tensor to two consumers.  Where a tensor has two consumers
(``x`` into a block and into ``h``, ``t`` into every block) the sum of their gradients stays torch's addition.  fp32, no host
synchronisation in either direction, no atomics, the same bits on every call.

The modules still exchange [B, C, H, W] views (``Run.nhwc``'s contract): where a view's channel count is not a multiple of 64
(32 and 96 channels) the next module repacks it (``ld_dn_pack_nhwc``).

The fused clipped-Adam / EMA step and the trainer around this module are ``denoiser_train.py`` (``torch.optim.Adam`` trains
it as it is, too).  NOT covered: 16-bit storage outside the ``ResnetBlock``s (``act_storage``, ``conv_out_storage``).
"""
import math

import torch
from torch import nn

from . import _cabi as cabi
from .attention_grad import Attention
from .condenc import FILTERS, ResUnet
from .linattn_grad import LinearAttention
from .resample import Conv2d, Downsample, Upsample
from .resblock import ResnetBlock
from .trainable import (AMP_ATTN_TYPES, AMP_TYPES, SWITCHES, TrainableModule, check_amp_attn_precision, check_amp_precision,
                        check_switch, pad64, stream)
from .weights import UnetConfig


def _empty(fill, dev, *shape):
    t = torch.empty(*shape, dtype=torch.float32, device=dev)
    if fill is not None:
        t.fill_(fill)                       # (debug hook: nothing may depend on what a fresh buffer holds)
    return t


# ---------------------------------------------------------------------------------------------------- the time MLP
class _TimeFn(torch.autograd.Function):
    """``apply(mod, times, freqs, w1, b1, w3, b3)``: times [B] fp32 -> temb [B, T]."""

    @staticmethod
    def forward(ctx, mod, times, freqs, w1, b1, w3, b3):
        dev, B, dim, T = times.device, times.shape[0], mod.dim, mod.time_dim
        with torch.cuda.device(dev):
            w1, b1, w3, b3 = (t.detach().contiguous() for t in (w1, b1, w3, b3))
            emb, h1, temb = (_empty(mod.debug_fill, dev, B, n) for n in (dim, T, T))
            cabi.check(cabi.lib().ld_dn_time_mlp_forward(times.data_ptr(), freqs.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                                                         w3.data_ptr(), b3.data_ptr(), emb.data_ptr(), h1.data_ptr(),
                                                         temb.data_ptr(), B, dim, T, stream(dev)), "dn_time_mlp_forward")
        ctx.mod = mod
        ctx.save_for_backward(emb, h1, w3)
        return temb

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dtemb):
        emb, h1, w3 = ctx.saved_tensors
        mod, dev, B = ctx.mod, emb.device, emb.shape[0]
        dim, T, fill = mod.dim, mod.time_dim, mod.debug_fill
        with torch.cuda.device(dev):
            lib = cabi.lib()
            dtemb = dtemb.contiguous()
            work = _empty(fill, dev, max(int(lib.ld_dn_time_mlp_work_bytes(B, dim, T)), 4) // 4)
            dw1, db1, dw3, db3 = (_empty(fill, dev, *s) for s in ((T, dim), (T,), (T, T), (T,)))
            cabi.check(lib.ld_dn_time_mlp_backward(dtemb.data_ptr(), emb.data_ptr(), h1.data_ptr(), w3.data_ptr(), work.data_ptr(),
                                                   dw1.data_ptr(), db1.data_ptr(), dw3.data_ptr(), db3.data_ptr(), B, dim, T,
                                                   stream(dev)), "dn_time_mlp_backward")
        return None, None, None, dw1, db1, dw3, db3


class TimeMLP(nn.Module):
    """``time_mlp`` of ddpm.py:339-344 with ``SinusoidalPosEmb(dim, theta)`` (ddpm.py:136-149) in front, forward and backward
    in HIP (fp32): parameters ``1.weight`` [4 dim, dim], ``1.bias``, ``3.weight`` [4 dim, 4 dim], ``3.bias``.

    ``forward(time)``: ``time`` [B] int32, int64 or float32 on the GPU (it has no gradient); returns [B, 4 dim].  ``dim`` is
    even and at least 4."""

    debug_fill = None       # a float: every buffer the module allocates is filled with it first (tests: NaN)

    def __init__(self, dim, theta=10000):
        super().__init__()
        if not isinstance(dim, int) or isinstance(dim, bool) or dim < 4 or dim % 2:
            raise ValueError(f"TimeMLP: dim {dim} must be an even int of at least 4")
        self.dim, self.time_dim, self.theta = dim, 4 * dim, theta
        self.add_module("1", nn.Linear(dim, self.time_dim))
        self.add_module("3", nn.Linear(self.time_dim, self.time_dim))
        half = dim // 2
        step = math.log(theta) / (half - 1)
        self.register_buffer("freqs", torch.exp(torch.arange(half) * -step), persistent=False)          # ddpm.py:145-146

    def forward(self, time):
        if not isinstance(time, torch.Tensor) or time.dim() != 1 or time.numel() == 0:
            raise ValueError("TimeMLP: time must be a non-empty [B] tensor")
        if time.dtype not in (torch.int32, torch.int64, torch.float32):
            raise ValueError(f"TimeMLP: time is {time.dtype}; int32, int64 and float32 are supported")
        if time.requires_grad:
            raise ValueError("TimeMLP: time has no gradient; it must not require grad")
        if not time.is_cuda:
            raise ValueError("TimeMLP: time is a CPU tensor; the module runs on HIP kernels only (there is no CPU path)")
        lin1, lin3 = self._modules["1"], self._modules["3"]
        tensors = (self.freqs, lin1.weight, lin1.bias, lin3.weight, lin3.bias)
        for t in tensors:
            if t.device != time.device or t.dtype != torch.float32:
                raise ValueError(f"TimeMLP: a parameter is {t.dtype} on {t.device}, time is on {time.device}")
        times = time.detach().to(torch.float32).contiguous()         # (the reference: long t times an fp32 table)
        return _TimeFn.apply(self, times, self.freqs.contiguous(), *tensors[1:])


# ---------------------------------------------------------------------------------------------------- the glue
def _padded_view(t, fill, ld=None):
    """The padded NHWC memory behind ``t`` [B, C, H, W] and its pixel stride: ``t`` itself when it is a channel slice of such
    a tensor (what every module returns) -- of pixel stride ``ld`` when that is given --, a repacked copy otherwise."""
    B, C, H, W = t.shape
    sb, sc, sh, sw = t.stride()
    have = sw if W > 1 else sh if H > 1 else sb if B > 1 else (C if ld is None else ld)
    ok = (sc == 1 or C == 1) and have >= C and have % 4 == 0 and t.data_ptr() % 16 == 0 and (W == 1 or sw == have) and \
        (H == 1 or sh == W * have) and (B == 1 or sb == H * W * have) and ld in (None, have)
    if ok:
        return t, have
    ld = pad64(C) if ld is None else ld
    out = _empty(fill, t.device, B, H, W, ld)
    cabi.check(cabi.lib().ld_dn_pack_nhwc(t.data_ptr(), out.data_ptr(), B, C, H, W, sb, sc, sh, sw, ld, stream(t.device)),
               "pack_nhwc")
    return out, ld


class _JoinFn(torch.autograd.Function):
    """``apply(fill, a, a2, b)``: cat((a (+ a2), b), dim=1) of [B, C, H, W] tensors (``a2`` or ``b`` may be ``None``) as one
    ``ld_dn_join`` launch; the gradients are views of ``dout``."""

    @staticmethod
    def forward(ctx, fill, a, a2, b):
        B, ca, H, W = a.shape
        cb = 0 if b is None else b.shape[1]
        dev = a.device
        with torch.cuda.device(dev):
            ap, lda = _padded_view(a, fill)
            a2p = bp = None
            ldb = 0
            if a2 is not None:
                a2p, _ = _padded_view(a2, fill, ld=lda)          # (one stride for both)
            if b is not None:
                bp, ldb = _padded_view(b, fill)
            ldo = pad64(ca + cb)
            out = _empty(fill, dev, B, H, W, ldo)
            cabi.check(cabi.lib().ld_dn_join(ap.data_ptr(), cabi.ptr(a2p), cabi.ptr(bp), out.data_ptr(), B, H, W, ca, lda, cb, ldb,
                                             ldo, stream(dev)), "dn_join")
        ctx.ca, ctx.have = ca, (a2 is not None, b is not None)
        return out[..., :ca + cb].permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        ca = ctx.ca
        need = ctx.needs_input_grad
        da = dout[:, :ca]
        return (None, da if need[1] else None, da if ctx.have[0] and need[2] else None,
                dout[:, ca:] if ctx.have[1] and need[3] else None)


def _check_join(name, a, other):
    if a.shape[0] != other.shape[0] or a.shape[2:] != other.shape[2:]:
        raise ValueError(f"{name}: {tuple(a.shape)} and {tuple(other.shape)} do not go together")


# ---------------------------------------------------------------------------------------------------- the Unet
def _switch(name, doc):
    """``TrainableUnet``'s property for a switch of ``trainable.SWITCHES``: the setter checks the value, stores it and hands it
    to every sub-module whose class lists more than one value for the switch.  A refused value changes nothing, and no
    switch touches another: none needs another but the two storage switches (``check_storage_precision``, at the block's
    call)."""
    def get(self):
        return getattr(self, "_" + name)

    def hand_down(self, value):
        check_switch("TrainableUnet", name, value)
        if name == "conv_precision":
            check_amp_precision("TrainableUnet", getattr(self, "_amp", "no"), value)
        if name in ("attn_precision", "full_attn_precision"):
            check_amp_attn_precision("TrainableUnet", getattr(self, "_amp_attn", "fp32"), name, value)
        setattr(self, "_" + name, value)
        for m in self.modules():
            if len(getattr(type(m), SWITCHES[name], ())) > 1:
                setattr(m, name, value)
    return property(get, hand_down, doc=doc)


class TrainableUnet(nn.Module):
    """``Unet`` of ddpm.py:286-451 (the constructor arguments of ``ldh.Unet`` minus ``compute_dtype`` and ``tuning``), forward
    and backward in HIP (fp32), under ``torch.autograd``.  The ``state_dict`` is the reference's.

    ``forward(x, cond_img, time)``: ``x`` [B, channels, H, W] and ``cond_img`` [B, 1 or 3, H, W] fp32 on the GPU, both data
    (they must not require grad: the stem and the encoder's image block have no input gradient), ``time`` [B] int32, int64 or
    float32; H and W divisible by ``downsample_factor``.  Returns [B, out_dim, H, W], contiguous.

    Refused with ``ValueError``: ``self_condition``, ``learned_variance``, ``learned_sinusoidal_cond`` /
    ``random_fourier_features``, ``attn_dim_head != 32``, a ``dim`` / ``init_dim`` the blocks refuse or that does not fit the
    condition encoder's width."""

    def __init__(self, dim, init_dim=None, out_dim=None, dim_mults=(1, 2, 4, 8), channels=1, self_condition=False, cond_img=True,
                 resnet_block_groups=8, learned_variance=False, learned_sinusoidal_cond=False, random_fourier_features=False,
                 learned_sinusoidal_dim=16, sinusoidal_pos_emb_theta=10000, attn_dim_head=32, attn_heads=4,
                 full_attn=(False, False, False, True), flash_attn=False, mode="mri", conv_precision="fp32",
                 act_storage="fp32", conv_out_storage="fp32", attn_precision="fp32", full_attn_precision="fp32", amp="no",
                 amp_attn="fp32"):
        super().__init__()
        check_amp_precision("TrainableUnet", check_switch("TrainableUnet", "amp", amp, AMP_TYPES), conv_precision)
        check_switch("TrainableUnet", "amp_attn", amp_attn, AMP_ATTN_TYPES)
        switches = dict(conv_precision=conv_precision, act_storage=act_storage, conv_out_storage=conv_out_storage,
                        attn_precision=attn_precision, full_attn_precision=full_attn_precision)
        for switch in SWITCHES:
            check_switch("TrainableUnet", switch, switches[switch])
        for flag, what in ((self_condition, "self_condition"), (learned_variance, "learned_variance"),
                           (learned_sinusoidal_cond, "learned_sinusoidal_cond"), (random_fourier_features, "random_fourier_features")):
            if flag:
                raise ValueError(f"TrainableUnet: {what} is not built for training (no shipped caller of the reference sets it)")
        if attn_dim_head != 32:
            raise ValueError(f"TrainableUnet: attn_dim_head {attn_dim_head}; the attention kernels are built for 32")
        init_dim = dim if init_dim is None else init_dim
        dim_mults = tuple(dim_mults)
        if not all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in (dim, init_dim, channels) + dim_mults) or \
                not dim_mults:
            raise ValueError(f"TrainableUnet: dim {dim}, init_dim {init_dim}, channels {channels} and dim_mults {dim_mults} must be "
                             "positive ints")
        if dim % 32 or init_dim != dim:
            raise ValueError(f"TrainableUnet: dim {dim} must be a multiple of 32 and init_dim {init_dim} must equal it "
                             "(final_res_block takes cat(x, r) as 2 dim channels)")
        full_attn = tuple(full_attn) if isinstance(full_attn, (tuple, list)) else (full_attn,) * len(dim_mults)
        if len(full_attn) != len(dim_mults):
            raise ValueError(f"TrainableUnet: full_attn {full_attn} and dim_mults {dim_mults} differ in length")
        self.cfg = UnetConfig(dim=dim, init_dim=init_dim, out_dim=channels if out_dim is None else out_dim, dim_mults=dim_mults,
                              channels=channels, resnet_block_groups=resnet_block_groups, attn_dim_head=attn_dim_head,
                              attn_heads=attn_heads, full_attn=full_attn, mode=mode)
        self.mode, self.channels, self.out_dim, self.cond_img = mode, channels, self.cfg.out_dim, cond_img
        self.self_condition = self.random_or_learned_sinusoidal_cond = False
        self._debug_fill = None
        # (registration order is the reference's, ddpm.py:312-398: it is the order of the state_dict)
        self.cond_model = ResUnet(data=mode)
        feat = FILTERS[3] if self.cond_model.early_exit else FILTERS[4]
        dims = self.cfg.dims
        if dims[-1] != feat:
            raise ValueError(f"TrainableUnet: the bottleneck has dim * dim_mults[-1] = {dims[-1]} channels, the condition encoder of "
                             f"mode {mode!r} gives {feat}; conv_fusion takes twice the former")
        self.init_conv = Conv2d(channels, init_dim, 7, padding=3)
        td = self.cfg.time_dim
        self.time_mlp = TimeMLP(dim, theta=sinusoidal_pos_emb_theta)

        def block(cin, cout):
            return ResnetBlock(cin, cout, time_emb_dim=td, groups=resnet_block_groups)

        def attn(c, full):
            return (Attention if full else LinearAttention)(c, heads=attn_heads, dim_head=attn_dim_head)

        io = self.cfg.in_out
        n = len(io)
        self.downs, self.ups = nn.ModuleList([]), nn.ModuleList([])
        for i, ((cin, cout), full) in enumerate(zip(io, full_attn)):
            self.downs.append(nn.ModuleList([block(cin, cin), block(cin, cin), attn(cin, full),
                                             Downsample(cin, cout) if i < n - 1 else Conv2d(cin, cout, 3, padding=1)]))
        mid = dims[-1]
        self.mid_block1, self.mid_attn, self.mid_block2 = block(mid, mid), attn(mid, True), block(mid, mid)
        self.conv_fusion = block(2 * mid, mid)
        for j, ((cin, cout), full) in enumerate(zip(reversed(io), reversed(full_attn))):
            self.ups.append(nn.ModuleList([block(cout + cin, cout), block(cout + cin, cout), attn(cout, full),
                                           Upsample(cout, cin) if j < n - 1 else Conv2d(cout, cin, 3, padding=1)]))
        self.final_res_block = block(2 * dim, dim)
        self.final_conv = Conv2d(dim, self.out_dim, 1)
        for switch, value in switches.items():
            setattr(self, "_" + switch, "fp32")
            if value != "fp32":                      # (the default is the modules' class attribute: nothing to hand down)
                setattr(self, switch, value)
        self._amp = "no"
        if amp != "no":
            self.amp = amp
        self._amp_attn = "fp32"
        if amp_attn != "fp32":
            self.amp_attn = amp_attn

    @property
    def downsample_factor(self):
        return self.cfg.downsample_factor

    @property
    def debug_fill(self):
        return self._debug_fill

    @debug_fill.setter
    def debug_fill(self, value):
        """A float (tests: NaN): every buffer any sub-module or the glue allocates is filled with it first."""
        self._debug_fill = value
        for m in self.modules():
            if m is not self and hasattr(type(m), "debug_fill"):
                m.debug_fill = value

    conv_precision = _switch("conv_precision", """``"fp32"`` or ``"bf16"``: at ``"bf16"`` every convolution of every
        sub-module, and both of its gradients, round their operands to bf16 and multiply on the bf16 matrix cores with fp32
        accumulation (``TrainableModule``); activations, parameters, gradients, the norms, the attention cores, the head and the
        time MLP stay fp32.""")
    act_storage = _switch("act_storage", """``"fp32"`` or ``"bf16"``: at ``"bf16"`` every ``ResnetBlock`` keeps the activations
        that only its convolutions read as bf16 (``ResnetBlock``); that needs ``conv_precision = "bf16"``, where it changes no
        bit of any result.  The other modules have no such storage yet and stay fp32.""")
    conv_out_storage = _switch("conv_out_storage", """``"fp32"`` or ``"bf16"``: at ``"bf16"`` every ``ResnetBlock`` writes the
        outputs of its two 3x3 convolutions rounded to bf16, and its GroupNorms read and autograd keeps that tensor
        (``ResnetBlock``); that needs ``conv_precision = "bf16"`` and, unlike ``act_storage``, moves results.  The other modules
        have no such storage and stay fp32.""")
    attn_precision = _switch("attn_precision", """``"fp32"`` or ``"bf16"``: at ``"bf16"`` every ``LinearAttention`` runs the four
        passes of its attention core on the bf16 matrix cores (``LinearAttention.attn_precision``).  The full ``Attention``
        modules have a switch of their own (``full_attn_precision``) and are not touched.""")
    full_attn_precision = _switch("full_attn_precision", """``"fp32"`` or ``"bf16"``: at ``"bf16"`` every full-softmax
        ``Attention`` runs the three passes of its core on the bf16 matrix cores (``Attention.full_attn_precision``).""")

    @property
    def amp(self):
        """``"no"`` or ``"fp16"`` (``trainable.AMP_TYPES``; the reference's mixed-precision mode, not one of the switches): at
        ``"fp16"`` every launch that ``conv_precision = "bf16"`` would route runs on the fp16 matrix cores instead
        (``TrainableModule.amp``), everything else stays fp32.  Handed to every ``TrainableModule``; refused together with
        ``conv_precision = "bf16"``, and a refused value changes nothing."""
        return self._amp

    @amp.setter
    def amp(self, value):
        check_amp_precision("TrainableUnet", check_switch("TrainableUnet", "amp", value, AMP_TYPES), self._conv_precision)
        self._amp = value
        for m in self.modules():
            if isinstance(m, TrainableModule):
                m.amp = value

    @property
    def amp_attn(self):
        """``"fp32"`` or ``"fp16"`` (``trainable.AMP_ATTN_TYPES``; not one of the switches): at ``"fp16"`` every ``LinearAttention``
        and every ``Attention`` runs the passes of its core on the fp16 matrix cores (the modules' ``amp_attn``).  Refused
        together with ``attn_precision = "bf16"`` or ``full_attn_precision = "bf16"``, in either order; a refused value changes
        nothing.  Independent of ``amp`` here; ``DenoiserTrainer`` takes it only with ``amp=True``, for the loss scaler."""
        return self._amp_attn

    @amp_attn.setter
    def amp_attn(self, value):
        check_switch("TrainableUnet", "amp_attn", value, AMP_ATTN_TYPES)
        for switch in ("attn_precision", "full_attn_precision"):
            check_amp_attn_precision("TrainableUnet", value, switch, getattr(self, "_" + switch))
        self._amp_attn = value
        for m in self.modules():
            if isinstance(m, TrainableModule) and type(m).AMP_ATTN_RIVAL is not None:
                m.amp_attn = value

    def _join(self, a, b):
        _check_join("TrainableUnet", a, b)
        return _JoinFn.apply(self._debug_fill, a, None, b)

    def _add(self, a, a2):
        return _JoinFn.apply(self._debug_fill, a, a2, None)

    def _check(self, x, cond_img, time):
        cfg = self.cfg
        for name, t, c in (("x", x, cfg.channels), ("cond_img", cond_img, cfg.cond_in_channels)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != c or t.numel() == 0:
                raise ValueError(f"TrainableUnet: {name} must be a non-empty [B, {c}, H, W] tensor")
            if t.dtype != torch.float32:
                raise ValueError(f"TrainableUnet: {name} is {t.dtype}; only float32 is supported (no 16-bit storage in training)")
            if t.requires_grad:
                raise ValueError(f"TrainableUnet: {name} is data (the stem and the encoder's image block have no input gradient); "
                                 "it must not require grad")
        if x.shape[0] != cond_img.shape[0] or x.shape[2:] != cond_img.shape[2:]:
            raise ValueError(f"TrainableUnet: x {tuple(x.shape)} and cond_img {tuple(cond_img.shape)} differ in batch or size")
        f = self.downsample_factor
        if x.shape[2] % f or x.shape[3] % f:
            raise ValueError(f"TrainableUnet: your input dimensions {tuple(x.shape[2:])} need to be divisible by {f}, given the unet")
        if not isinstance(time, torch.Tensor) or tuple(time.shape) != (x.shape[0],):
            raise ValueError(f"TrainableUnet: time must be a [{x.shape[0]}] tensor")
        for name, t in (("x", x), ("cond_img", cond_img), ("time", time)):
            if not t.is_cuda:
                raise ValueError(f"TrainableUnet: {name} is a CPU tensor; the module runs on HIP kernels only (there is no CPU path)")
        if cond_img.device != x.device or time.device != x.device:
            raise ValueError("TrainableUnet: x, cond_img and time are on different devices")

    def forward(self, x, cond_img, time):
        self._check(x, cond_img, time)
        x = self.init_conv(x)
        r = x
        t = self.time_mlp(time)
        h = []
        for block1, block2, attn, downsample in self.downs:
            x = block1(x, t)
            h.append(x)
            x = block2(x, t)
            x = self._add(attn(x), x)
            h.append(x)
            x = downsample(x)
        x = self.mid_block1(x, t)
        x = self._add(self.mid_attn(x), x)
        x = self.mid_block2(x, t)
        cond_feat = self.cond_model(cond_img)
        x = self._join(x, cond_feat)
        x = self.conv_fusion(x)
        for block1, block2, attn, upsample in self.ups:
            x = self._join(x, h.pop())
            x = block1(x, t)
            x = self._join(x, h.pop())
            x = block2(x, t)
            x = self._add(attn(x), x)
            x = upsample(x)
        x = self._join(x, r)
        x = self.final_res_block(x, t)
        return self.final_conv(x)
