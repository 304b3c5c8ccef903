"""A trainable ``LinearAttention`` (ddpm.py:214-251) on HIP kernels: the second slice of the denoiser's backward pass.

``LinearAttention(dim, heads=4, dim_head=32)`` carries the reference's parameters under the reference's ``state_dict``
names (``norm.g``, ``to_qkv.weight``, ``to_out.0.weight``, ``to_out.0.bias``, ``to_out.1.g``) and takes part in
``torch.autograd`` the way ``ResnetBlock`` does: one ``autograd.Function`` whose two halves are launches -- the kernels of
``csrc/linattn_grad.hip`` (RMSNorm and its backward; the context and output passes of the attention core and the reduce and
apply passes of its backward) and the convolution kernels the library already had: ``ld_pc_conv`` with ``ksize = 1`` for
``to_qkv``, ``to_out.0`` and the two data gradients on the transposed weights, ``ld_seg_wgrad`` for the two weight gradients
and ``ld_dn_colsum`` for ``to_out.0.bias``.  fp32, no host synchronisation in either direction, no eager-PyTorch arithmetic
on an activation, and bit-reproducible results (every sum is added in a fixed order; no floating-point atomics).

The layout is ``resblock.py``'s: activations NHWC with a pixel stride of the next multiple of 64 floats, zero in the
padding; ``to_qkv``'s output is [B, H, W, pad64(3 hidden)] with q at channel 0, k at ``hidden``, v at ``2 hidden`` and a
head's 32 channels contiguous inside each.  The attention core's backward is one reduction over pixels and one
element-wise pass: nothing of size [N, N] or per pixel is kept besides ``qkv``.  The module adds no residual (the
reference's ``Unet`` writes ``attn(x) + x``).
"""
import torch
from torch import nn

from . import _cabi as cabi
from . import resblock
from .resblock import _pad64

DIM_HEAD = 32


class _RMSNorm(nn.Module):
    """Parameter holder with the reference's name (``g`` [1, dim, 1, 1], ones); the arithmetic is in ``_Run``."""

    def __init__(self, dim):
        super().__init__()
        self.g = nn.Parameter(torch.ones(1, dim, 1, 1))


class _Packed:
    """Kernel-layout copies of the module's weights on one device (zero in the padded channels)."""

    def __init__(self, mod, dev):
        lib, st = cabi.lib(), resblock._st(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.keep = []

        def conv1(w, co, cop, ci, cip):
            """OI11 [co, ci] -> forward layout [cop][cip] and data-gradient layout [cip][cop]."""
            w = w.detach().contiguous()
            fwd, dgr = torch.zeros(cop * cip, **f32), torch.zeros(cip * cop, **f32)
            cabi.check(lib.ld_seg_permute3(w.data_ptr(), fwd.data_ptr(), co, ci, 1, 0, cip, 1, cip, st), "permute3")
            cabi.check(lib.ld_seg_permute3(w.data_ptr(), dgr.data_ptr(), co, ci, 1, 0, 1, cop, cop, st), "permute3")
            self.keep.append(w)
            return fwd, dgr

        out = mod.to_out[0] if isinstance(mod.to_out, nn.Sequential) else mod.to_out      # (full Attention: a bare Conv2d)
        self.wqf, self.wqd = conv1(mod.to_qkv.weight, 3 * mod.hidden, mod.ld3, mod.dim, mod.cp)
        self.wof, self.wod = conv1(out.weight, mod.dim, mod.cp, mod.hidden, mod.hp)
        self.bo = torch.zeros(mod.cp, **f32)
        self.bo[:mod.dim].copy_(out.bias.detach())
        n = max(mod.cp, mod.hp, mod.ld3)
        self.ones, self.zeros = torch.ones(n, **f32), torch.zeros(n, **f32)


class _Run(resblock._Run):
    """The launches of one forward / backward of the module on one device (``empty``, ``nhwc`` and ``conv`` are the
    block's)."""

    def work(self, nbytes):
        return self.empty(max(int(nbytes), 8) // 8, dtype=torch.float64)

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

    def la_work(self):
        return self.work(self.lib.ld_dn_la_work_bytes(self.B, self.blk.heads, self.H, self.W))

    def wgrad(self, dy, a, co, cop, ci, cip):
        """The weight gradient [co, ci, 1, 1] of a 1x1 convolution from its output gradient dy [.., cop] and input a [.., cip]."""
        B, H, W = self.B, self.H, self.W
        splits = int(self.lib.ld_seg_wgrad_splits(B, H, W, cip, cop, 1))
        work, dwp = self.empty(splits * cop * cip), self.empty(cop * cip)
        cabi.check(self.lib.ld_seg_wgrad(dy.data_ptr(), a.data_ptr(), work.data_ptr(), dwp.data_ptr(), B, H, W, cip, cop, 1, splits,
                                         self.st), "seg_wgrad")
        dw = self.empty(co, ci, 1, 1)
        cabi.check(self.lib.ld_dn_gather3(dwp.data_ptr(), dw.data_ptr(), co, ci, 1, 0, cip, 1, cip, self.st), "gather3")
        return dw

    # ------------------------------------------------------------------------------------------------ the two halves
    def forward(self, x, keep=True):
        m, p, lib = self.blk, self.p, self.lib
        B, H, W = self.B, self.H, self.W
        g1, g2 = m.norm.g.detach(), m.to_out[1].g.detach()
        xp = self.nhwc(x, m.dim, m.cp)
        xn, r1 = self.rms_forward(xp, g1, m.dim, m.cp, keep)
        qkv = self.conv(xn, p.wqf, p.zeros, m.cp, m.ld3, 1)
        ctx, kstat = self.empty(B, m.heads, 32, 32), self.empty(B, m.heads, 32, 2)
        cabi.check(lib.ld_dn_la_context(qkv.data_ptr(), self.la_work().data_ptr(), ctx.data_ptr(), kstat.data_ptr(), B, H, W,
                                        m.heads, m.ld3, self.st), "dn_la_context")
        att = self.empty(B, H, W, m.hp)
        cabi.check(lib.ld_dn_la_out(qkv.data_ptr(), ctx.data_ptr(), att.data_ptr(), B, H, W, m.heads, m.ld3, m.hp, self.st),
                   "dn_la_out")
        y = self.conv(att, p.wof, p.bo, m.hp, m.cp, 1)
        out, r2 = self.rms_forward(y, g2, m.dim, m.cp, keep)
        return out, (xp, r1, xn, qkv, ctx, kstat, att, y, r2)

    def backward(self, dout, saved):
        m, p, lib = self.blk, self.p, self.lib
        B, H, W = self.B, self.H, self.W
        xp, r1, xn, qkv, ctx, kstat, att, y, r2 = saved
        g1, g2 = m.norm.g.detach(), m.to_out[1].g.detach()
        g = {}
        dop = self.nhwc(dout, m.dim, m.cp)
        dy = self.empty(B, H, W, m.cp)                       # (not in place: dop may be the caller's own tensor)
        g["to_out.1.g"] = self.rms_backward(dop, y, g2, r2, m.dim, m.cp, dy)
        g["to_out.0.weight"] = self.wgrad(dy, att, m.dim, m.cp, m.hidden, m.hp)
        db = self.empty(m.dim)
        cabi.check(lib.ld_dn_colsum(dy.data_ptr(), self.work(lib.ld_dn_gn_work_bytes(B, H, W, m.dim)).data_ptr(), db.data_ptr(), B,
                                    H, W, m.dim, m.cp, self.st), "dn_colsum")
        g["to_out.0.bias"] = db
        datt = self.conv(dy, p.wod, p.zeros, m.cp, m.hp, 1)
        dctx, rk = self.empty(B, m.heads, 32, 32), self.empty(B, m.heads, 32)
        cabi.check(lib.ld_dn_la_backward_reduce(qkv.data_ptr(), datt.data_ptr(), ctx.data_ptr(), self.la_work().data_ptr(),
                                                dctx.data_ptr(), rk.data_ptr(), B, H, W, m.heads, m.ld3, m.hp, self.st),
                   "dn_la_backward_reduce")
        dqkv = self.empty(B, H, W, m.ld3)
        cabi.check(lib.ld_dn_la_backward_apply(qkv.data_ptr(), datt.data_ptr(), ctx.data_ptr(), kstat.data_ptr(), dctx.data_ptr(),
                                               rk.data_ptr(), dqkv.data_ptr(), B, H, W, m.heads, m.ld3, m.hp, self.st),
                   "dn_la_backward_apply")
        g["to_qkv.weight"] = self.wgrad(dqkv, xn, 3 * m.hidden, m.ld3, m.dim, m.cp)
        dxp = self.conv(dqkv, p.wqd, p.zeros, m.ld3, m.cp, 1)                # = d xn, then d x in place
        g["norm.g"] = self.rms_backward(dxp, xp, g1, r1, m.dim, m.cp, dxp)
        return dxp[..., :m.dim].permute(0, 3, 1, 2), g


class _LinearAttentionFn(torch.autograd.Function):
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


class LinearAttention(resblock._PackedWeights, nn.Module):
    """``LinearAttention(dim, heads=4, dim_head=32)`` of ddpm.py:214-251, forward and backward in HIP (fp32).

    ``forward(x)``: ``x`` [B, dim, H, W] fp32 on the GPU (``channels_last`` with ``dim`` a multiple of 64 is read in place);
    returns ``to_out(...)`` [B, dim, H, W], a ``channels_last``-strided view of the kernels' NHWC output, without the
    residual.  ``dim`` is a positive multiple of 32, ``heads >= 1``, ``dim_head`` is 32; any H, W >= 1."""

    debug_fill = None       # a float: every buffer the module allocates is filled with it first (tests: NaN)

    def __init__(self, dim, heads=4, dim_head=32):
        super().__init__()
        if dim <= 0 or dim % 32:
            raise ValueError(f"LinearAttention: dim {dim} must be a positive multiple of 32")
        if dim_head != DIM_HEAD:
            raise ValueError(f"LinearAttention: dim_head {dim_head}; the kernels are built for dim_head = 32, the reference's "
                             "only value")
        if heads < 1:
            raise ValueError(f"LinearAttention: heads {heads} must be at least 1")
        self.dim, self.heads, self.dim_head, self.hidden = dim, heads, dim_head, heads * dim_head
        self.cp, self.hp, self.ld3 = _pad64(dim), _pad64(self.hidden), _pad64(3 * self.hidden)
        self.norm = _RMSNorm(dim)
        self.to_qkv = nn.Conv2d(dim, 3 * self.hidden, 1, bias=False)
        self.to_out = nn.Sequential(nn.Conv2d(self.hidden, dim, 1), _RMSNorm(dim))

    def _pack(self, dev):
        return _Packed(self, dev)

    def _check(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.dim or x.numel() == 0:
            raise ValueError(f"LinearAttention: x must be a non-empty [B, {self.dim}, H, W] tensor")
        if x.dtype != torch.float32:
            raise ValueError(f"LinearAttention: x is {x.dtype}; only float32 is supported (no 16-bit storage in training)")
        if not x.is_cuda:
            raise ValueError("LinearAttention: x is a CPU tensor; the module runs on HIP kernels only (there is no CPU path)")
        for n, p in self.named_parameters():
            if p.device != x.device or p.dtype != torch.float32:
                raise ValueError(f"LinearAttention: parameter {n} is {p.dtype} on {p.device}, x is float32 on {x.device}")

    def forward(self, x):
        self._check(x)
        names, params = zip(*self.named_parameters())
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return _LinearAttentionFn.apply(self, names, x, *params)
        with torch.no_grad(), torch.cuda.device(x.device):
            run = _Run(self, self._packed_for(x.device), x.device, x.shape[0], x.shape[2], x.shape[3])
            out, _ = run.forward(x.detach(), keep=False)
        return out[..., :self.dim].permute(0, 3, 1, 2)
