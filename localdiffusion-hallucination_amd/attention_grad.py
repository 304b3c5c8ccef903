"""A trainable full ``Attention`` (ddpm.py:253-282 with attend.py's non-flash path) on HIP kernels: the third slice of the
denoiser's backward pass.

``Attention(dim, heads=4, dim_head=32)`` carries the reference's parameters under the reference's ``state_dict`` names
(``norm.g``, ``to_qkv.weight``, ``to_out.weight``, ``to_out.bias``; there is no RMSNorm behind ``to_out``) and takes part in
``torch.autograd`` the way ``LinearAttention`` does: one ``autograd.Function`` whose two halves are launches -- RMSNorm and
its backward (``csrc/linattn_grad.hip``), ``ld_pc_conv`` with ``ksize = 1`` for ``to_qkv``, ``to_out`` and the two data
gradients on the transposed weights, ``ld_seg_wgrad`` for the two weight gradients, ``ld_dn_colsum`` for the bias, and the
softmax attention itself in ``csrc/attention_grad.hip``: ``ld_dn_fa_forward`` (an online softmax over tiles of 64 keys that
keeps one number per row, ``lse``) and ``ld_dn_fa_backward`` (a row pass for dq, a column pass for dk and dv, the
probabilities recomputed from ``qkv`` and ``lse``).  fp32, no host synchronisation in either direction, no eager-PyTorch
arithmetic on an activation, bit-reproducible results (every sum is added in a fixed order; no floating-point atomics),
and nothing of size [n, n] is kept or written in either direction.

The layout is ``linattn_grad.py``'s: activations NHWC with a pixel stride of the next multiple of 64 floats, zero in the
padding; ``to_qkv``'s output is [B, H, W, pad64(3 hidden)] with q at channel 0, k at ``hidden``, v at ``2 hidden`` and a
head's 32 channels contiguous inside each.  q is not pre-scaled: the kernels apply ``dim_head ** -0.5`` to the logits.  The
module adds no residual (the reference's ``Unet`` writes ``attn(x) + x``).
"""
import torch
from torch import nn

from . import _cabi as cabi
from . import linattn_grad, resblock
from .linattn_grad import DIM_HEAD, _RMSNorm
from .resblock import _pad64


class _Run(linattn_grad._Run):
    """The launches of one forward / backward of the module on one device (RMSNorm, ``conv``, ``wgrad`` and ``work`` are
    ``LinearAttention``'s)."""

    def forward(self, x, keep=True):
        m, p, lib = self.blk, self.p, self.lib
        B, H, W = self.B, self.H, self.W
        xp = self.nhwc(x, m.dim, m.cp)
        xn, r1 = self.rms_forward(xp, m.norm.g.detach(), m.dim, m.cp, keep)
        qkv = self.conv(xn, p.wqf, p.zeros, m.cp, m.ld3, 1)
        att = self.empty(B, H, W, m.hp)
        lse = self.empty(B, m.heads, H * W) if keep else None
        cabi.check(lib.ld_dn_fa_forward(qkv.data_ptr(), att.data_ptr(), cabi.ptr(lse), B, H, W, m.heads, m.ld3, m.hp, self.st),
                   "dn_fa_forward")
        y = self.conv(att, p.wof, p.bo, m.hp, m.cp, 1)
        return y, (xp, r1, xn, qkv, att, lse)

    def backward(self, dout, saved):
        m, p, lib = self.blk, self.p, self.lib
        B, H, W = self.B, self.H, self.W
        xp, r1, xn, qkv, att, lse = saved
        g = {}
        dy = self.nhwc(dout, m.dim, m.cp)                    # (read only: it may be the caller's own tensor)
        g["to_out.weight"] = self.wgrad(dy, att, m.dim, m.cp, m.hidden, m.hp)
        db = self.empty(m.dim)
        cabi.check(lib.ld_dn_colsum(dy.data_ptr(), self.work(lib.ld_dn_gn_work_bytes(B, H, W, m.dim)).data_ptr(), db.data_ptr(), B,
                                    H, W, m.dim, m.cp, self.st), "dn_colsum")
        g["to_out.bias"] = db
        datt = self.conv(dy, p.wod, p.zeros, m.cp, m.hp, 1)
        dqkv = self.empty(B, H, W, m.ld3)
        work = self.work(lib.ld_dn_fa_work_bytes(B, m.heads, H, W))
        cabi.check(lib.ld_dn_fa_backward(qkv.data_ptr(), att.data_ptr(), datt.data_ptr(), lse.data_ptr(), work.data_ptr(),
                                         dqkv.data_ptr(), B, H, W, m.heads, m.ld3, m.hp, self.st), "dn_fa_backward")
        g["to_qkv.weight"] = self.wgrad(dqkv, xn, 3 * m.hidden, m.ld3, m.dim, m.cp)
        dxp = self.conv(dqkv, p.wqd, p.zeros, m.ld3, m.cp, 1)                # = d xn, then d x in place
        g["norm.g"] = self.rms_backward(dxp, xp, m.norm.g.detach(), r1, m.dim, m.cp, dxp)
        return dxp[..., :m.dim].permute(0, 3, 1, 2), g


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, names, x, *params):
        with torch.cuda.device(x.device):
            run = _Run(mod, mod._packed_for(x.device), x.device, x.shape[0], x.shape[2], x.shape[3])
            out, saved = run.forward(x)
        ctx.run, ctx.names = run, names
        ctx.save_for_backward(*saved)
        return out[..., :mod.dim].permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        run = ctx.run
        with torch.cuda.device(run.dev):
            run.st = resblock._st(run.dev)
            dx, g = run.backward(dout, ctx.saved_tensors)
        return (None, None, dx) + tuple(g.get(n) for n in ctx.names)


class Attention(resblock._PackedWeights, nn.Module):
    """``Attention(dim, heads=4, dim_head=32)`` of ddpm.py:253-282, forward and backward in HIP (fp32).

    ``forward(x)``: ``x`` [B, dim, H, W] fp32 on the GPU (``channels_last`` with ``dim`` a multiple of 64 is read in place);
    returns ``to_out(...)`` [B, dim, H, W], a ``channels_last``-strided view of the kernels' NHWC output, without the
    residual.  ``dim`` is a positive multiple of 32, ``heads >= 1``, ``dim_head`` is 32; any H, W >= 1."""

    debug_fill = None       # a float: every buffer the module allocates is filled with it first (tests: NaN)

    def __init__(self, dim, heads=4, dim_head=32):
        super().__init__()
        if dim <= 0 or dim % 32:
            raise ValueError(f"Attention: dim {dim} must be a positive multiple of 32")
        if dim_head != DIM_HEAD:
            raise ValueError(f"Attention: dim_head {dim_head}; the kernels are built for dim_head = 32, the reference's only value")
        if heads < 1:
            raise ValueError(f"Attention: heads {heads} must be at least 1")
        self.dim, self.heads, self.dim_head, self.hidden = dim, heads, dim_head, heads * dim_head
        self.cp, self.hp, self.ld3 = _pad64(dim), _pad64(self.hidden), _pad64(3 * self.hidden)
        self.norm = _RMSNorm(dim)
        self.to_qkv = nn.Conv2d(dim, 3 * self.hidden, 1, bias=False)
        self.to_out = nn.Conv2d(self.hidden, dim, 1)

    def _pack(self, dev):
        return linattn_grad._Packed(self, dev)

    def _check(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.dim or x.numel() == 0:
            raise ValueError(f"Attention: x must be a non-empty [B, {self.dim}, H, W] tensor")
        if x.dtype != torch.float32:
            raise ValueError(f"Attention: x is {x.dtype}; only float32 is supported (no 16-bit storage in training)")
        if not x.is_cuda:
            raise ValueError("Attention: x is a CPU tensor; the module runs on HIP kernels only (there is no CPU path)")
        for n, p in self.named_parameters():
            if p.device != x.device or p.dtype != torch.float32:
                raise ValueError(f"Attention: parameter {n} is {p.dtype} on {p.device}, x is float32 on {x.device}")

    def forward(self, x):
        self._check(x)
        names, params = zip(*self.named_parameters())
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return _AttentionFn.apply(self, names, x, *params)
        with torch.no_grad(), torch.cuda.device(x.device):
            run = _Run(self, self._packed_for(x.device), x.device, x.shape[0], x.shape[2], x.shape[3])
            out, _ = run.forward(x.detach(), keep=False)
        return out[..., :self.dim].permute(0, 3, 1, 2)
