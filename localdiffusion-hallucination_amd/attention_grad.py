"""A trainable full ``Attention`` (ddpm.py:253-282 with attend.py's non-flash path) on HIP kernels: the third slice of the
denoiser's backward pass.

``Attention(dim, heads=4, dim_head=32)`` carries the reference's parameters under the reference's ``state_dict`` names
(``norm.g``, ``to_qkv.weight``, ``to_out.weight``, ``to_out.bias``; there is no RMSNorm behind ``to_out``) and takes part in
``torch.autograd`` the way ``LinearAttention`` does: one ``autograd.Function`` whose two halves are launches -- RMSNorm and
its backward (``csrc/linattn_grad.hip``), ``ld_pc_conv`` with ``ksize = 1`` for ``to_qkv``, ``to_out`` and the two data
gradients on the transposed weights, ``ld_seg_wgrad`` for the two weight gradients, ``ld_dn_colsum`` for the bias, and the
softmax attention itself in ``csrc/attention_grad.hip``: ``ld_dn_fa_forward`` (an online softmax over tiles of 64 keys that
keeps one number per row, ``lse``) and ``ld_dn_fa_backward`` (a row pass for dq, a column pass for dk and dv, the
probabilities recomputed from ``qkv`` and ``lse``), or their bf16 matrix-core siblings ``ld_dn_fa_forward16`` /
``ld_dn_fa_backward16`` of ``csrc/attention16.hip`` at ``full_attn_precision = "bf16"``, or the fp16 ones (``ld_dn_fa_forward_f16``
/ ``ld_dn_fa_backward_f16``) at ``amp_attn = "fp16"``.  fp32 storage, no host synchronisation in either direction, no eager-PyTorch
arithmetic on an activation, bit-reproducible results (every sum is added in a fixed order; no floating-point atomics),
and nothing of size [n, n] is kept or written in either direction.

The layout is ``linattn_grad.py``'s: activations NHWC with a pixel stride of the next multiple of 64 floats, zero in the
padding; ``to_qkv``'s output is [B, H, W, pad64(3 hidden)] with q at channel 0, k at ``hidden``, v at ``2 hidden`` and a
head's 32 channels contiguous inside each.  q is not pre-scaled: the kernels apply ``dim_head ** -0.5`` to the logits.  The
module adds no residual (the reference's ``Unet`` writes ``attn(x) + x``).

This file holds the module's two launch sequences and its constructor; the rest is ``trainable.py``'s and, shared with
``LinearAttention`` alone, ``linattn_grad.py``'s ``attention_init``, ``AttentionPacked`` and ``RMSNormRun``.
"""
from torch import nn

from . import _cabi as cabi
from .linattn_grad import AttentionPacked, RMSNormRun, attention_init
from .trainable import TrainableModule


class _Run(RMSNormRun):
    """The launches of one forward / backward of the module on one device."""

    def fa(self, name):
        """The core's entry point ``ld_dn_fa_<name>`` at the module's ``amp_attn`` / ``full_attn_precision`` (read at every
        launch; the two are never both set)."""
        suffix = "_f16" if self.mod.amp_attn == "fp16" else "16" if self.mod.full_attn_precision == "bf16" else ""
        return getattr(self.lib, f"ld_dn_fa_{name}{suffix}")

    def forward(self, x, keep=True):
        m, p, lib = self.mod, self.p, self.lib
        B, H, W = self.B, self.H, self.W
        xp = self.nhwc(x, m.dim, m.cp)
        xn, r1 = self.rms_forward(xp, m.norm.g.detach(), m.dim, m.cp, keep)
        qkv = self.conv(xn, p.wqf, p.zeros, m.cp, m.ld3, 1)
        att = self.empty(B, H, W, m.hp)
        lse = self.empty(B, m.heads, H * W) if keep else None
        cabi.check(self.fa("forward")(qkv.data_ptr(), att.data_ptr(), cabi.ptr(lse), B, H, W, m.heads, m.ld3, m.hp, self.st),
                   "dn_fa_forward")
        y = self.conv(att, p.wof, p.bo, m.hp, m.cp, 1)
        return y, (xp, r1, xn, qkv, att, lse)

    def backward(self, dout, saved):
        m, p, lib = self.mod, self.p, self.lib
        B, H, W = self.B, self.H, self.W
        xp, r1, xn, qkv, att, lse = saved
        g = {}
        dy = self.nhwc(dout, m.dim, m.cp)                    # (read only: it may be the caller's own tensor)
        g["to_out.weight"] = self.wgrad(dy, att, m.dim, m.cp, m.hidden, m.hp, 1)
        g["to_out.bias"] = self.bias_grad(dy, m.dim, m.cp)
        datt = self.conv(dy, p.wod, p.zeros, m.cp, m.hp, 1)
        dqkv = self.empty(B, H, W, m.ld3)
        work = self.work(lib.ld_dn_fa_work_bytes(B, m.heads, H, W))
        cabi.check(self.fa("backward")(qkv.data_ptr(), att.data_ptr(), datt.data_ptr(), lse.data_ptr(), work.data_ptr(),
                                       dqkv.data_ptr(), B, H, W, m.heads, m.ld3, m.hp, self.st), "dn_fa_backward")
        g["to_qkv.weight"] = self.wgrad(dqkv, xn, 3 * m.hidden, m.ld3, m.dim, m.cp, 1)
        dxp = self.conv(dqkv, p.wqd, p.zeros, m.ld3, m.cp, 1)                # = d xn, then d x in place
        g["norm.g"] = self.rms_backward(dxp, xp, m.norm.g.detach(), r1, m.dim, m.cp, dxp)
        return dxp[..., :m.dim].permute(0, 3, 1, 2), (), g


class Attention(TrainableModule):
    """``Attention(dim, heads=4, dim_head=32)`` of ddpm.py:253-282, forward and backward in HIP (fp32).

    ``forward(x)``: ``x`` [B, dim, H, W] fp32 on the GPU (``channels_last`` with ``dim`` a multiple of 64 is read in place);
    returns ``to_out(...)`` [B, dim, H, W], a ``channels_last``-strided view of the kernels' NHWC output, without the
    residual.  ``dim`` is a positive multiple of 32, ``heads >= 1``, ``dim_head`` is 32; any H, W >= 1.

    ``attn_precision`` is ``"fp32"``, the only value so far (``ATTN_PRECISIONS``): the full-softmax core has no bf16 kernels
    yet under that name, and ``"bf16"`` is refused with ``ValueError``.

    ``full_attn_precision = "bf16"`` (default ``"fp32"``, ``FULL_ATTN_PRECISIONS``) runs the three passes of the core -- the
    forward, the backward's row pass and its column pass -- on the bf16 matrix cores (csrc/attention16.hip,
    ``ld_dn_fa_forward16`` / ``ld_dn_fa_backward16``): both operands of every product (q, k, v, dO, and the computed p and
    ds) rounded to bf16, fp32 accumulation; the logits' scale, the online softmax, its normaliser (the unrounded p), lse,
    delta and everything in memory stay fp32, every sum keeps one order.  It is read at every launch and may change between
    calls; it is no part of the ``state_dict``, of the packed weights' cache key or of a checkpoint, and it is independent
    of ``attn_precision`` (``LinearAttention``'s switch) and of ``conv_precision``.

    ``amp_attn = "fp16"`` (default ``"fp32"``, ``trainable.AMP_ATTN_TYPES``) runs the same three passes on the fp16 matrix
    cores (``ld_dn_fa_forward_f16`` / ``ld_dn_fa_backward_f16``): that contract with q, k, v, dO, p and ds rounded to fp16
    instead (three more significand bits; beyond 65504 is inf and a small p or ds underflows, so it is meant for
    ``DenoiserTrainer``'s loss scaler).  The same rules, independent of ``amp``; together with ``full_attn_precision =
    "bf16"`` it is refused with ``ValueError`` in either order of assignment."""

    Run = _Run
    attn_precision = "fp32"
    ATTN_PRECISIONS = ("fp32",)
    full_attn_precision = "fp32"
    FULL_ATTN_PRECISIONS = ("fp32", "bf16")
    amp_attn = "fp32"
    AMP_ATTN_RIVAL = "full_attn_precision"

    def __init__(self, dim, heads=4, dim_head=32):
        super().__init__()
        attention_init(self, dim, heads, dim_head)
        self.to_out = nn.Conv2d(self.hidden, dim, 1)

    def _pack(self, dev):
        return AttentionPacked(self, self.to_out, dev)
