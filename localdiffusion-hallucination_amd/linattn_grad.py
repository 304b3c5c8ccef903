"""A trainable ``LinearAttention`` (ddpm.py:214-251) on HIP kernels: the second slice of the denoiser's backward pass.

``LinearAttention(dim, heads=4, dim_head=32)`` carries the reference's parameters under the reference's ``state_dict``
names (``norm.g``, ``to_qkv.weight``, ``to_out.0.weight``, ``to_out.0.bias``, ``to_out.1.g``) and takes part in
``torch.autograd`` the way ``ResnetBlock`` does: one ``autograd.Function`` whose two halves are launches -- the kernels of
``csrc/linattn_grad.hip`` (RMSNorm and its backward; the context and output passes of the attention core and the reduce and
apply passes of its backward) and the convolution kernels the library already had: ``ld_pc_conv`` with ``ksize = 1`` for
``to_qkv``, ``to_out.0`` and the two data gradients on the transposed weights, ``ld_seg_wgrad`` for the two weight gradients
and ``ld_dn_colsum`` for ``to_out.0.bias``.  fp32, no host synchronisation in either direction, no eager-PyTorch arithmetic
on an activation, and bit-reproducible results (every sum is added in a fixed order; no floating-point atomics).
``LinearAttention.attn_precision = "bf16"`` puts the four passes of the core on the bf16 matrix cores (``csrc/linattn16.hip``:
operands rounded, fp32 accumulation, the same tensors and the same order of every sum); the default runs the fp32 launches.
``LinearAttention.amp_attn = "fp16"`` puts them on the fp16 matrix cores (the ``<f16>`` instantiations, ``ld_dn_la_*_f16``).

The layout is ``resblock.py``'s: activations NHWC with a pixel stride of the next multiple of 64 floats, zero in the
padding; ``to_qkv``'s output is [B, H, W, pad64(3 hidden)] with q at channel 0, k at ``hidden``, v at ``2 hidden`` and a
head's 32 channels contiguous inside each.  The attention core's backward is one reduction over pixels and one
element-wise pass: nothing of size [N, N] or per pixel is kept besides ``qkv``.  The module adds no residual (the
reference's ``Unet`` writes ``attn(x) + x``).

What every trainable module shares is in ``trainable.py``; this file holds the module's own launches and what ``Attention``
shares with it alone: ``attention_init`` (the constructor checks and sizes), ``AttentionPacked`` (the kernel-layout weights)
and ``RMSNormRun`` (the RMSNorm launches).
"""
import torch
from torch import nn

from . import _cabi as cabi
from .trainable import Run, TrainableModule, ones_zeros, pack_conv, pack_vec, pad64, stream

DIM_HEAD = 32


class _RMSNorm(nn.Module):
    """Parameter holder with the reference's name (``g`` [1, dim, 1, 1], ones); the arithmetic is in ``_Run``."""

    def __init__(self, dim):
        super().__init__()
        self.g = nn.Parameter(torch.ones(1, dim, 1, 1))


def attention_init(mod, dim, heads, dim_head):
    """The constructor checks, sizes and the parameters in front of ``to_out`` that ``LinearAttention`` and ``Attention``
    share."""
    name = type(mod).__name__
    if dim <= 0 or dim % 32:
        raise ValueError(f"{name}: dim {dim} must be a positive multiple of 32")
    if dim_head != DIM_HEAD:
        raise ValueError(f"{name}: dim_head {dim_head}; the kernels are built for dim_head = 32, the reference's only value")
    if heads < 1:
        raise ValueError(f"{name}: heads {heads} must be at least 1")
    mod.dim = mod.dim_out = dim
    mod.heads, mod.dim_head, mod.hidden = heads, dim_head, heads * dim_head
    mod.cp, mod.hp, mod.ld3 = pad64(dim), pad64(mod.hidden), pad64(3 * mod.hidden)
    mod.norm = _RMSNorm(dim)
    mod.to_qkv = nn.Conv2d(dim, 3 * mod.hidden, 1, bias=False)


class AttentionPacked:
    """Kernel-layout copies of an attention module's weights on one device (zero in the padded channels); ``to_out`` is the
    module's output convolution."""

    def __init__(self, mod, to_out, dev):
        lib, st = cabi.lib(), stream(dev)
        prec = mod.operand_precision
        self.wqf, self.wqd = pack_conv(lib, st, mod.to_qkv.weight, 3 * mod.hidden, mod.ld3, mod.dim, mod.cp, 1, prec)
        self.wof, self.wod = pack_conv(lib, st, to_out.weight, mod.dim, mod.cp, mod.hidden, mod.hp, 1, prec)
        self.bo = pack_vec(to_out.bias, mod.cp)
        self.ones, self.zeros = ones_zeros(max(mod.cp, mod.hp, mod.ld3), dev)


class RMSNormRun(Run):
    """``Run`` with the RMSNorm launches, for the two attention modules."""

    def rms_forward(self, x, g, c, cp, keep):
        B, H, W = self.B, self.H, self.W
        out = self.empty(B, H, W, cp)
        rinv = self.empty(B, H, W) if keep else None
        cabi.check(self.lib.ld_dn_rms_forward(x.data_ptr(), g.data_ptr(), cabi.ptr(rinv), out.data_ptr(), B, H, W, c, cp, self.st),
                   "dn_rms_forward")
        return out, rinv

    def rms_backward(self, dout, x, g, rinv, c, cp, dx):
        B, H, W = self.B, self.H, self.W
        dg = self.empty(1, c, 1, 1)
        work = self.work(self.lib.ld_dn_rms_work_bytes(B, H, W, c))
        cabi.check(self.lib.ld_dn_rms_backward(dout.data_ptr(), x.data_ptr(), g.data_ptr(), rinv.data_ptr(), work.data_ptr(),
                                               dg.data_ptr(), dx.data_ptr(), B, H, W, c, cp, self.st), "dn_rms_backward")
        return dg


class _Run(RMSNormRun):
    """The launches of one forward / backward of the module on one device."""

    def la_work(self):
        return self.work(self.lib.ld_dn_la_work_bytes(self.B, self.mod.heads, self.H, self.W))

    def la(self, name):
        """The core's entry point ``ld_dn_la_<name>`` at the module's ``amp_attn`` / ``attn_precision`` (read at every
        launch; the two are never both set)."""
        suffix = "_f16" if self.mod.amp_attn == "fp16" else "16" if self.mod.attn_precision == "bf16" else ""
        return getattr(self.lib, f"ld_dn_la_{name}{suffix}")

    # ------------------------------------------------------------------------------------------------ the two halves
    def forward(self, x, keep=True):
        m, p = self.mod, self.p
        B, H, W = self.B, self.H, self.W
        g1, g2 = m.norm.g.detach(), m.to_out[1].g.detach()
        xp = self.nhwc(x, m.dim, m.cp)
        xn, r1 = self.rms_forward(xp, g1, m.dim, m.cp, keep)
        qkv = self.conv(xn, p.wqf, p.zeros, m.cp, m.ld3, 1)
        ctx, kstat = self.empty(B, m.heads, 32, 32), self.empty(B, m.heads, 32, 2)
        cabi.check(self.la("context")(qkv.data_ptr(), self.la_work().data_ptr(), ctx.data_ptr(), kstat.data_ptr(), B, H, W,
                                      m.heads, m.ld3, self.st), "dn_la_context")
        att = self.empty(B, H, W, m.hp)
        cabi.check(self.la("out")(qkv.data_ptr(), ctx.data_ptr(), att.data_ptr(), B, H, W, m.heads, m.ld3, m.hp, self.st),
                   "dn_la_out")
        y = self.conv(att, p.wof, p.bo, m.hp, m.cp, 1)
        out, r2 = self.rms_forward(y, g2, m.dim, m.cp, keep)
        return out, (xp, r1, xn, qkv, ctx, kstat, att, y, r2)

    def backward(self, dout, saved):
        m, p = self.mod, self.p
        B, H, W = self.B, self.H, self.W
        xp, r1, xn, qkv, ctx, kstat, att, y, r2 = saved
        g1, g2 = m.norm.g.detach(), m.to_out[1].g.detach()
        g = {}
        dop = self.nhwc(dout, m.dim, m.cp)
        dy = self.empty(B, H, W, m.cp)                       # (not in place: dop may be the caller's own tensor)
        g["to_out.1.g"] = self.rms_backward(dop, y, g2, r2, m.dim, m.cp, dy)
        g["to_out.0.weight"] = self.wgrad(dy, att, m.dim, m.cp, m.hidden, m.hp, 1)
        g["to_out.0.bias"] = self.bias_grad(dy, m.dim, m.cp)
        datt = self.conv(dy, p.wod, p.zeros, m.cp, m.hp, 1)
        dctx, rk = self.empty(B, m.heads, 32, 32), self.empty(B, m.heads, 32)
        cabi.check(self.la("backward_reduce")(qkv.data_ptr(), datt.data_ptr(), ctx.data_ptr(), self.la_work().data_ptr(),
                                              dctx.data_ptr(), rk.data_ptr(), B, H, W, m.heads, m.ld3, m.hp, self.st),
                   "dn_la_backward_reduce")
        dqkv = self.empty(B, H, W, m.ld3)
        cabi.check(self.la("backward_apply")(qkv.data_ptr(), datt.data_ptr(), ctx.data_ptr(), kstat.data_ptr(), dctx.data_ptr(),
                                             rk.data_ptr(), dqkv.data_ptr(), B, H, W, m.heads, m.ld3, m.hp, self.st),
                   "dn_la_backward_apply")
        g["to_qkv.weight"] = self.wgrad(dqkv, xn, 3 * m.hidden, m.ld3, m.dim, m.cp, 1)
        dxp = self.conv(dqkv, p.wqd, p.zeros, m.ld3, m.cp, 1)                # = d xn, then d x in place
        g["norm.g"] = self.rms_backward(dxp, xp, g1, r1, m.dim, m.cp, dxp)
        return dxp[..., :m.dim].permute(0, 3, 1, 2), (), g


class LinearAttention(TrainableModule):
    """``LinearAttention(dim, heads=4, dim_head=32)`` of ddpm.py:214-251, forward and backward in HIP (fp32).

    ``forward(x)``: ``x`` [B, dim, H, W] fp32 on the GPU (``channels_last`` with ``dim`` a multiple of 64 is read in place);
    returns ``to_out(...)`` [B, dim, H, W], a ``channels_last``-strided view of the kernels' NHWC output, without the
    residual.  ``dim`` is a positive multiple of 32, ``heads >= 1``, ``dim_head`` is 32; any H, W >= 1.

    ``attn_precision = "bf16"`` (default ``"fp32"``) runs the four passes of the attention core -- context, output and the
    backward's reduce and apply -- on the bf16 matrix cores (csrc/linattn16.hip): both operands of every 32 x 32 product of
    a head rounded to bf16, fp32 accumulation, the softmaxes, (m, Z), the merges and everything in memory fp32, every sum in
    a fixed order.  It may change between steps; it is no part of the ``state_dict`` or of the packed weights (the core
    has none), and it is independent of ``conv_precision``.

    ``amp_attn = "fp16"`` (default ``"fp32"``, ``trainable.AMP_ATTN_TYPES``) runs the same four passes on the fp16 matrix
    cores (``ld_dn_la_*_f16``): the bf16 contract with fp16 rounding of the same operands, except that the dv product of the
    apply pass rounds ``dctx[d][e] / Z[d]`` and ``exp(k - m)`` instead of ``dctx`` and ``exp(k - m) / Z``, which is an fp16
    subnormal on large maps.  An operand beyond 65504 becomes inf: the mode is meant for ``DenoiserTrainer``'s loss scaler.
    The same rules as ``attn_precision`` (read at every launch, in no ``state_dict``, independent of ``amp`` and
    ``conv_precision``), and the two together are refused with ``ValueError`` in either order of assignment."""

    Run = _Run
    attn_precision = "fp32"
    ATTN_PRECISIONS = ("fp32", "bf16")
    amp_attn = "fp32"
    AMP_ATTN_RIVAL = "attn_precision"

    def __init__(self, dim, heads=4, dim_head=32):
        super().__init__()
        attention_init(self, dim, heads, dim_head)
        self.to_out = nn.Sequential(nn.Conv2d(self.hidden, dim, 1), _RMSNorm(dim))

    def _pack(self, dev):
        return AttentionPacked(self, self.to_out[0], dev)
