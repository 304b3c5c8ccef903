"""What the trainable pieces of the denoiser share: ``ResnetBlock`` (``resblock.py``), ``LinearAttention``
(``linattn_grad.py``), ``Attention`` (``attention_grad.py``) and ``Downsample`` / ``Upsample`` / ``Conv2d`` (``resample.py``)
are each a ``TrainableModule`` with a ``Run`` of their own.

The common layout: activations are fp32 NHWC (bf16 where a storage switch below says so) with a pixel stride of
``pad64(channels)`` elements, the upper part zero; the kernel-layout copies of the weights (``pack_conv``, ``pack_vec``) are zero there too and are cached per device, keyed on every
parameter's ``data_ptr`` and ``_version`` (``PackedWeights``).  A module's forward and backward are the two halves of one
``autograd.Function``; each half is a sequence of launches that the module's ``Run`` subclass writes down, out of the launches
every module uses (``Run``: buffers, the NHWC repack, ``ld_pc_conv``, the weight and bias gradients) and its own.

The training precision switches (``SWITCHES``).  Each is ``"fp32"``, the default, or ``"bf16"``.  A module has a switch when its
class defines the default and the tuple of the values it implements (``conv_precision`` / ``CONV_PRECISIONS``); the value is a
class attribute until it is set, is validated on assignment (``check_switch``: a refused value leaves the old one in place), is
read at every call, and is no part of the ``state_dict``.  ``TrainableUnet`` hands a value to the sub-modules whose class lists
more than one, and ``DenoiserTrainer`` passes it through.
  ``conv_precision``       every module: ``pack_conv``, ``Run.conv`` and ``Run.wgrad_packed`` route on it.  The kernel-layout
                           weights are bf16 (it is in their cache key) and the convolution and its two gradients run on
                           ``csrc/conv16.hip``: operands rounded to bf16, fp32 accumulation; what sits in memory stays fp32.
  ``act_storage``          ``ResnetBlock`` only so far: the activations that only its convolutions read are stored as bf16
                           (``Run.nhwc(dtype=)``, a producer's ``_to16`` launch; ``Run.conv`` and ``Run.wgrad_packed`` pick the
                           ``_from16`` entry point from the dtype they are handed).  Needs ``conv_precision = "bf16"``, whose
                           launches round such a tensor anyway, so no bit of any result changes (``check_act_storage_precision``).
  ``conv_out_storage``     ``ResnetBlock`` only so far: the outputs ``y1`` / ``y2`` of its two 3x3 convolutions, which GroupNorm reads
                           four times each, are written (``Run.conv(out_dtype=)``: a ``_to16`` launch rounds the fp32 epilogue
                           value to nearest even), read and saved as bf16; the backward is the exact gradient of that forward, the
                           rounding passed through as the identity.  Needs ``conv_precision = "bf16"`` (``check_storage_precision``).
                           Unlike ``act_storage`` it moves results, by about what the bf16 convolutions themselves do.
  ``attn_precision``       ``LinearAttention``: the four passes of its core on ``csrc/linattn16.hip`` (a placeholder on ``Attention``).
  ``full_attn_precision``  ``Attention``: the three passes of its core on ``csrc/attention16.hip``.

``amp`` (``AMP_TYPES``: ``"no"``, the default, or ``"fp16"``) is the reference's mixed-precision mode under the reference's name
and is NOT one of ``SWITCHES`` (those are fp32 / bf16 pairs): at ``"fp16"`` every launch that ``conv_precision = "bf16"`` would
put on the bf16 matrix cores -- the 3x3 and 1x1 convolutions, the im2col convolutions, ``to_qkv`` / ``to_out``, and both of
their gradients -- runs on the fp16 forms of ``csrc/conv16.hip`` instead (``ld_dn_conv_f16``, ``ld_dn_wgrad_f16``,
``ld_dn_pack_conv_f16``): operands rounded to fp16, fp32 accumulation, fp16 kernel-layout weights (``amp`` is in their cache
key), and everything in memory and everything else fp32.  fp16 has three more significand bits than bf16 and a narrow range: a
large operand becomes inf and a small one underflows, so this mode is meant to run under the loss scaler of
``DenoiserTrainer(amp=True)``.  It is validated on assignment like a switch, handed down by ``TrainableUnet`` like
``conv_precision``, no part of a ``state_dict``, and refused together with ``conv_precision = "bf16"`` (two masters for the
same launches); the storage switches need ``conv_precision = "bf16"`` and so stay out of reach.

``amp_attn`` (``AMP_ATTN_TYPES``: ``"fp32"``, the default, or ``"fp16"``) is ``amp``'s counterpart for the two attention cores and
is NOT one of ``SWITCHES`` either: at ``"fp16"`` the four passes of a ``LinearAttention``'s core and the three of an
``Attention``'s run on the fp16 instantiations of ``csrc/linattn16.hip`` / ``csrc/attention16.hip`` (``ld_dn_la_*_f16``,
``ld_dn_fa_*_f16``): the bf16 kernels' contract with the same operands rounded to fp16 and ``v_mfma_f32_32x32x16_f16``, except
that the linear core's dv product keeps ``1 / Z`` on the ``dctx`` side (``exp(k - m) / Z`` is an fp16 subnormal from 128 x 128
pixels on).  It is validated on assignment, read at every launch, no part of a ``state_dict`` or of the packed weights' cache
key (the cores have none), handed down by ``TrainableUnet`` to both kinds of module, and on a module independent of ``amp`` and
``conv_precision``.  It is refused together with the bf16 switch of the same launches (``attn_precision = "bf16"`` on
``LinearAttention``, ``full_attn_precision = "bf16"`` on ``Attention``; either on ``TrainableUnet``).  fp16's range is narrow --
a large dO or dctx becomes inf, a small p or ds underflows --, so ``DenoiserTrainer`` takes it only with the loss scaler of
``amp=True``.
"""
import ctypes as C

import torch
from torch import nn

from . import _cabi as cabi


def pad64(c):
    return (c + 63) // 64 * 64


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class PackedWeights:
    """Mixin of a trainable module: the cache of the kernel-layout copies of its weights (``_pack(dev)`` builds them)."""

    _packed = None

    def invalidate(self):
        """Drop the kernel-layout copies of the weights; they are rebuilt on next use.  ``.to()``, ``load_state_dict`` and any
        in-place change of a parameter (an optimiser step: its ``_version`` moves) do this by themselves."""
        self._packed = None

    def _apply(self, fn, *args, **kwargs):
        self.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        self.invalidate()
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    def _packed_for(self, dev):
        key = (dev, getattr(self, "conv_precision", "fp32"), getattr(self, "amp", "no")) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._packed is None or self._packed[0] != key:
            with torch.no_grad():
                self._packed = (key, self._pack(dev))
        return self._packed[1]


# ---------------------------------------------------------------------------------------------------- packing
# switch -> the class attribute that lists the values a module implements (the module docstring)
SWITCHES = {"conv_precision": "CONV_PRECISIONS", "act_storage": "ACT_STORAGES", "conv_out_storage": "CONV_OUT_STORAGES",
            "attn_precision": "ATTN_PRECISIONS", "full_attn_precision": "FULL_ATTN_PRECISIONS"}


def check_switch(owner, switch, value, allowed=("fp32", "bf16")):
    if not isinstance(value, str) or value not in allowed:
        raise ValueError(f"{owner}: {switch} {value!r} is not one of {', '.join(repr(v) for v in allowed)}")
    return value


AMP_TYPES = ("no", "fp16")      # TrainableModule.amp (the module docstring); outside SWITCHES


def check_amp_precision(name, amp, conv_precision):
    """``amp = "fp16"`` and ``conv_precision = "bf16"`` both route the convolution launches: together they are refused."""
    if amp == "fp16" and conv_precision == "bf16":
        raise ValueError(f"{name}: amp 'fp16' and conv_precision 'bf16' both choose the operand format of the convolutions; "
                         "set one of them")


AMP_ATTN_TYPES = ("fp32", "fp16")      # LinearAttention / Attention / TrainableUnet .amp_attn (the module docstring); outside SWITCHES


def check_amp_attn_precision(name, amp_attn, switch, precision):
    """``amp_attn = "fp16"`` and the bf16 switch of the same attention core both route its launches: together they are
    refused."""
    if amp_attn == "fp16" and precision == "bf16":
        raise ValueError(f"{name}: amp_attn 'fp16' and {switch} 'bf16' both choose the operand format of the attention core; "
                         "set one of them")


_OPERAND_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def check_act_storage(name, value, allowed=("fp32", "bf16")):
    """``check_switch`` under the one earlier name that ``tests/test_act_storage.py`` imports."""
    return check_switch(name, "act_storage", value, allowed)


_WHY_BF16_CONVS = {
    "act_storage": "the fp32 convolutions do not round their activations: the rounding would change results",
    "conv_out_storage": "only the bf16 convolutions have a launch that writes a bf16 output",
}


def check_storage_precision(name, switch, storage, conv_precision):
    """The two storage switches (``act_storage``, ``conv_out_storage``) are built on the bf16 convolutions only."""
    if storage == "bf16" and conv_precision != "bf16":
        raise ValueError(f"{name}: {switch} 'bf16' needs conv_precision 'bf16' ({_WHY_BF16_CONVS[switch]})")


def check_act_storage_precision(name, act_storage, conv_precision):
    """bf16 storage of the conv-only activations is exact only where the convolutions round them to bf16 anyway
    (``check_storage_precision`` under the earlier name that ``tests/test_act_storage.py`` imports)."""
    check_storage_precision(name, "act_storage", act_storage, conv_precision)


def pack_conv(lib, st, w, co, cop, ci, cip, k, precision="fp32"):
    """OIHW [co, ci, k, k] -> forward layout [cop][k*k][cip] and data-gradient layout [cip][flipped k*k][cop], zero in the
    padded channels; fp32, or with ``precision="bf16"`` / ``"fp16"`` (a module's ``operand_precision``) rounded to that
    format (what ``Run.conv`` then takes), in one launch."""
    w = w.detach().contiguous()
    kk = k * k
    if precision in _OPERAND_DTYPES:
        fwd, dgr = (torch.empty(cop * kk * cip, dtype=_OPERAND_DTYPES[precision], device=w.device) for _ in range(2))
        pack, what = (lib.ld_dn_pack_conv16, "dn_pack_conv16") if precision == "bf16" else (lib.ld_dn_pack_conv_f16, "dn_pack_conv_f16")
        cabi.check(pack(w.data_ptr(), fwd.data_ptr(), dgr.data_ptr(), co, cop, ci, cip, k, st), what)
        return fwd, dgr
    fwd, dgr = w.new_zeros(cop * kk * cip), w.new_zeros(cip * kk * cop)
    cabi.check(lib.ld_seg_permute3(w.data_ptr(), fwd.data_ptr(), co, ci, kk, 0, kk * cip, 1, cip, st), "permute3")
    cabi.check(lib.ld_seg_permute3(w.data_ptr(), dgr.data_ptr(), co, ci, kk, (kk - 1) * cop, 1, kk * cop, -cop, st), "permute3")
    return fwd, dgr


def as_conv_precision(t, precision):
    """A kernel-layout weight a module packed by itself (fp32), as ``Run.conv`` takes it at ``precision``: rounded to bf16
    or fp16 (torch's cast: round-to-nearest-even, overflow to inf, as ``ld_dn_pack_conv16`` / ``_f16`` round) or as it is."""
    return t.to(_OPERAND_DTYPES[precision]) if precision in _OPERAND_DTYPES else t


def pack_vec(v, n):
    """A bias or gain as n floats, zero behind its own."""
    out = v.new_zeros(n)
    out[:v.numel()].copy_(v.detach())
    return out


def ones_zeros(n, dev):
    """``ld_pc_conv``'s unit scale and the shift of a convolution without bias."""
    return torch.ones(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)


# ---------------------------------------------------------------------------------------------------- launches
class Run:
    """The launches of one forward / backward of a module on one device: here the ones every module uses.  A subclass adds
    its own and the two halves: ``forward(x, *extra, keep=True)`` returns the padded NHWC output and the tensors (or
    ``None``) to save, ``keep=False`` leaves out what only the backward reads; ``backward(dout, saved)`` returns dx (``None``:
    the input has no gradient), the gradients of the extra inputs and ``{parameter name: gradient}``.  The launches take the
    map size ``hw`` they work at, by default the run's own (H, W), which is x's.  ``packed`` has ``ones`` and ``zeros``."""

    def __init__(self, mod, packed, dev, B, H, W):
        self.mod, self.p, self.dev, self.B, self.H, self.W = mod, packed, dev, B, H, W
        self.lib, self.st = cabi.lib(), stream(dev)
        self.fill = mod.debug_fill
        self.bf16 = getattr(mod, "conv_precision", "fp32") == "bf16"      # (the precision ``packed`` was made at)
        self.fp16 = getattr(mod, "amp", "no") == "fp16"                   # amp: the same launches on the fp16 matrix cores
        self.wdtype = torch.bfloat16 if self.bf16 else torch.float16 if self.fp16 else torch.float32
        self.act16 = getattr(mod, "act_storage", "fp32") == "bf16"        # conv-only activations are kept as bf16
        self.y16 = getattr(mod, "conv_out_storage", "fp32") == "bf16"     # the convolution outputs GroupNorm reads, too

    def empty(self, *shape, dtype=torch.float32):
        t = torch.empty(*shape, dtype=dtype, device=self.dev)
        if self.fill is not None:
            t.fill_(self.fill)                  # (debug hook: nothing may depend on what a fresh buffer holds)
        return t

    def work(self, nbytes):
        return self.empty(max(int(nbytes), 8) // 8, dtype=torch.float64)

    def hw(self, hw):
        """The map size of a launch: the run's own unless the caller names another (``hw = (H, W)``)."""
        return (self.H, self.W) if hw is None else hw

    def nhwc(self, t, c, cp, hw=None, dtype=torch.float32):
        """[B, c, H, W] (fp32) of any strides -> NHWC with pixel stride cp; no copy when it already is that.  ``dtype`` is the
        copy's: ``torch.bfloat16`` for one that only bf16 convolutions read (a tensor read in place stays what it is)."""
        B, (H, W) = self.B, self.hw(hw)
        if c == cp and t.stride() == (H * W * c, 1, W * c, c) and t.data_ptr() % 16 == 0:
            return t
        out = self.empty(B, H, W, cp, dtype=dtype)
        sb, sc, sh, sw = t.stride()
        if dtype == torch.bfloat16:
            cabi.check(self.lib.ld_dn_pack_nhwc_to16(t.data_ptr(), out.data_ptr(), B, c, H, W, sb, sc, sh, sw, cp, self.st),
                       "pack_nhwc_to16")
        else:
            cabi.check(self.lib.ld_dn_pack_nhwc(t.data_ptr(), out.data_ptr(), B, c, H, W, sb, sc, sh, sw, cp, self.st), "pack_nhwc")
        return out

    def from16(self, act):
        """Whether ``act``, an activation a convolution launch is about to read, is bf16 in memory (the ``_from16`` entry
        points); that is refused where the convolutions are fp32."""
        if act.dtype != torch.bfloat16:
            return False
        if not self.bf16:
            raise RuntimeError(f"{type(self.mod).__name__}: a bfloat16 activation at conv_precision 'fp32' (only the bf16 "
                               "convolutions read 16-bit storage)")
        return True

    def conv(self, src, weight, shift, cin, cout, k, residual=None, hw=None, out_dtype=torch.float32):
        """``out_dtype``: ``torch.bfloat16`` for an output that is stored rounded (the ``_to16`` entry points; bf16
        convolutions only)."""
        H, W = self.hw(hw)
        to16 = out_dtype == torch.bfloat16
        if to16 and not self.bf16:
            raise RuntimeError(f"{type(self.mod).__name__}: a bfloat16 convolution output at conv_precision 'fp32' (only the "
                               "bf16 convolutions write 16-bit storage)")
        out = self.empty(self.B, H, W, cout, dtype=out_dtype)
        a = cabi.PcConvArgs()
        a.src, a.weight, a.scale, a.shift = src.data_ptr(), weight.data_ptr(), self.p.ones.data_ptr(), shift.data_ptr()
        a.residual, a.out = cabi.ptr(residual), out.data_ptr()
        a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout, a.ksize, a.stride, a.relu = self.B, H, W, cin, H, W, cout, k, 1, 0
        if weight.dtype != self.wdtype:
            raise RuntimeError(f"{type(self.mod).__name__}: a {weight.dtype} kernel-layout weight at conv_precision "
                               f"{'bf16' if self.bf16 else 'fp32'}{', amp fp16' if self.fp16 else ''} (the module's _pack does "
                               "not pass the precision on)")
        if self.fp16:
            a.weight = None
            cabi.check(self.lib.ld_dn_conv_f16(C.byref(a), weight.data_ptr(), self.st), "dn_conv_f16")
        elif self.from16(src) or self.bf16:
            what = "dn_conv16" + ("_from16" if src.dtype == torch.bfloat16 else "") + ("_to16" if to16 else "")
            a.weight = None
            cabi.check(getattr(self.lib, "ld_" + what)(C.byref(a), weight.data_ptr(), self.st), what)
        else:
            cabi.check(self.lib.ld_pc_conv(C.byref(a), self.st), "pc_conv")
        return out

    def wgrad_packed(self, dy, a, cop, cip, k, hw=None):
        """The weight gradient in the forward kernel layout [cop][k*k][cip] of a convolution from its output gradient dy
        [.., cop] and its input a [.., cip]."""
        B, (H, W) = self.B, self.hw(hw)
        kk = k * k
        splits = int(self.lib.ld_seg_wgrad_splits(B, H, W, cip, cop, k))
        work, dwp = self.empty(splits * cop * kk * cip), self.empty(cop * kk * cip)
        if self.fp16:
            wgrad, what = self.lib.ld_dn_wgrad_f16, "dn_wgrad_f16"
        elif self.from16(a):
            wgrad, what = self.lib.ld_dn_wgrad16_from16, "dn_wgrad16_from16"
        else:
            wgrad, what = (self.lib.ld_dn_wgrad16, "dn_wgrad16") if self.bf16 else (self.lib.ld_seg_wgrad, "seg_wgrad")
        cabi.check(wgrad(dy.data_ptr(), a.data_ptr(), work.data_ptr(), dwp.data_ptr(), B, H, W, cip, cop, k, splits, self.st), what)
        return dwp

    def wgrad(self, dy, a, co, cop, ci, cip, k, hw=None):
        """The weight gradient, in the parameter's OIHW [co, ci, k, k], of a convolution from its output gradient dy [.., cop]
        and its input a [.., cip]."""
        kk = k * k
        dwp = self.wgrad_packed(dy, a, cop, cip, k, hw)
        dw = self.empty(co, ci, k, k)
        cabi.check(self.lib.ld_dn_gather3(dwp.data_ptr(), dw.data_ptr(), co, ci, kk, 0, kk * cip, 1, cip, self.st), "gather3")
        return dw

    def bias_grad(self, dy, c, cp, hw=None):
        """The bias gradient [c] of a convolution from its output gradient dy [.., cp]."""
        B, (H, W) = self.B, self.hw(hw)
        db = self.empty(c)
        work = self.work(self.lib.ld_dn_gn_work_bytes(B, H, W, c))
        cabi.check(self.lib.ld_dn_colsum(dy.data_ptr(), work.data_ptr(), db.data_ptr(), B, H, W, c, cp, self.st), "dn_colsum")
        return db


class _Fn(torch.autograd.Function):
    """A module's ``Run.forward`` and ``Run.backward`` as one node: ``apply(mod, names, x, *extra, *params)`` with one
    parameter per name; ``extra`` are the further differentiable inputs (or ``None``)."""

    @staticmethod
    def forward(ctx, mod, names, x, *rest):
        with torch.cuda.device(x.device):
            run = mod._run(x)
            out, saved = run.forward(x, *rest[:len(rest) - len(names)])
        ctx.run, ctx.names = run, names
        ctx.save_for_backward(*[t for t in saved if t is not None])
        ctx.present = [t is not None for t in saved]
        return mod._view(out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        it = iter(ctx.saved_tensors)
        saved = tuple(next(it) if have else None for have in ctx.present)
        run = ctx.run
        with torch.cuda.device(run.dev):
            run.st = stream(run.dev)
            dx, d_extra, g = run.backward(dout, saved)
        return (None, None, dx, *d_extra) + tuple(g.get(n) for n in ctx.names)


class TrainableModule(PackedWeights, nn.Module):
    """A module whose forward and backward are HIP launches (fp32).  A subclass sets ``dim`` and ``dim_out`` (the channels of
    ``x`` and of the result) and ``Run`` (its ``Run`` subclass), and defines ``_pack(dev)``; ``forward(x, *extra)`` takes
    ``x`` [B, dim, H, W] on the GPU and returns [B, dim_out, H, W], a ``channels_last``-strided view of the kernels' NHWC
    output."""

    debug_fill = None       # a float: every buffer the module allocates is filled with it first (tests: NaN)
    conv_precision = "fp32"  # or "bf16": the operands of every convolution and of its two gradients are rounded to bf16 and
    #                          multiplied on the bf16 matrix cores with fp32 accumulation; everything else stays fp32
    act_storage = "fp32"     # or "bf16" where the module has it (ACT_STORAGES): the activations that only its convolutions read
    #                          are written, read and saved as bf16; at conv_precision "bf16" only, where no result changes
    conv_out_storage = "fp32"  # or "bf16" where the module has it (CONV_OUT_STORAGES): the convolution outputs that GroupNorm
    #                            reads are written rounded to bf16, read and saved as that; at conv_precision "bf16" only
    amp = "no"               # or "fp16" (AMP_TYPES; not one of SWITCHES): what conv_precision "bf16" routes to the bf16 matrix
    #                          cores runs on the fp16 ones instead; refused together with conv_precision "bf16"
    CONV_PRECISIONS = ("fp32", "bf16")
    ACT_STORAGES = ("fp32",)
    CONV_OUT_STORAGES = ("fp32",)
    AMP_ATTN_RIVAL = None    # an attention module: the bf16 switch of its core, which amp_attn = "fp16" is refused with
    Run = None

    def __setattr__(self, name, value):
        if name in SWITCHES and hasattr(type(self), name):
            check_switch(type(self).__name__, name, value, getattr(self, SWITCHES[name]))
        rival = type(self).AMP_ATTN_RIVAL
        if rival is not None and name == "amp_attn":
            check_amp_attn_precision(type(self).__name__, check_switch(type(self).__name__, name, value, AMP_ATTN_TYPES), rival,
                                     getattr(self, rival))
        elif rival is not None and name == rival:
            check_amp_attn_precision(type(self).__name__, self.amp_attn, rival, value)
        if name == "amp":
            check_amp_precision(type(self).__name__, check_switch(type(self).__name__, name, value, AMP_TYPES), self.conv_precision)
        elif name == "conv_precision":
            check_amp_precision(type(self).__name__, self.amp, value)
        super().__setattr__(name, value)

    @property
    def operand_precision(self):
        """What ``pack_conv`` / ``as_conv_precision`` make the kernel-layout weights at: ``"fp16"`` under ``amp``, else
        ``conv_precision``."""
        return "fp16" if self.amp == "fp16" else self.conv_precision

    def _run(self, x):
        return self.Run(self, self._packed_for(x.device), x.device, x.shape[0], x.shape[2], x.shape[3])

    def _view(self, out):
        """What the module returns of its ``Run.forward``'s output: by default the real channels of the padded NHWC tensor
        as [B, dim_out, H, W]; a module whose kernels write another layout (the head: NCHW) says so here."""
        return out[..., :self.dim_out].permute(0, 3, 1, 2)

    def _check_extra(self, x, *extra):
        """A subclass with further inputs checks them here, against an ``x`` of the right shape and type."""

    def _check(self, x, *extra):
        name = type(self).__name__
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.dim or x.numel() == 0:
            raise ValueError(f"{name}: x must be a non-empty [B, {self.dim}, H, W] tensor")
        if x.dtype != torch.float32:
            raise ValueError(f"{name}: x is {x.dtype}; only float32 is supported (no 16-bit storage in training)")
        self._check_extra(x, *extra)
        if not x.is_cuda:
            raise ValueError(f"{name}: x is a CPU tensor; the module runs on HIP kernels only (there is no CPU path)")
        for n, p in self.named_parameters():
            if p.device != x.device or p.dtype != torch.float32:
                raise ValueError(f"{name}: parameter {n} is {p.dtype} on {p.device}, x is float32 on {x.device}")

    def forward(self, x, *extra):
        self._check(x, *extra)
        names, params = zip(*self.named_parameters())
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, *extra, *params)):
            return _Fn.apply(self, names, x, *extra, *params)
        with torch.no_grad(), torch.cuda.device(x.device):
            out, _ = self._run(x).forward(x.detach(), *(None if t is None else t.detach() for t in extra), keep=False)
        return self._view(out)
