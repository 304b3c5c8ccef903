"""A trainable ``ResnetBlock`` (ddpm.py:170-212) on HIP kernels: the first slice of the denoiser's backward pass.

``ResnetBlock(dim, dim_out, time_emb_dim=..., groups=8)`` carries the reference's parameters under the reference's
``state_dict`` names and takes part in ``torch.autograd``: its forward and its backward are one ``autograd.Function``
whose two halves are launches of ``csrc/denoiser_grad.hip`` (GroupNorm -> FiLM -> SiLU in training mode and its
backward, the time projection and its backward, the layout kernels) and of the convolution kernels the library already
had: ``ld_pc_conv`` (forward, and the data gradients on the flipped / transposed weight with the skip path's gradient
as its ``residual``) and ``ld_seg_wgrad`` (weight gradients); the bias gradients are ``ld_dn_colsum``, a sibling of
``ld_seg_colsum`` that knows the pixel stride and spreads over the chip at these shapes.  There is no host
synchronisation in either direction and no eager-PyTorch arithmetic on an activation.

Those convolution kernels want channel counts that are multiples of 64; the denoiser's are multiples of 32.  A count
that is not a multiple of 64 is carried the way ``MnistClassifier`` carries conv1's 32 channels: every activation has a
pixel stride of the next multiple of 64 floats, the upper part zero, and the kernel-layout weights are zero there.  The
GroupNorm kernels know the real channel count, so padding enters no statistic and no gradient.

NOT covered (follow-ups that build on this module's layout; linear attention and RMSNorm are in ``linattn_grad.py``, full
attention is in ``attention_grad.py``): Down/Upsample, the 7x7 stem, the ResUnet encoder, the time MLP in front of the
blocks, any optimiser / EMA / ``Trainer``, 16-bit storage, and ``Unet`` assembling the backward of its blocks.
"""
import ctypes as C

import torch
from torch import nn

from . import _cabi as cabi

def _pad64(c):
    return (c + 63) // 64 * 64


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _PackedWeights:
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
        key = (dev,) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._packed is None or self._packed[0] != key:
            with torch.no_grad():
                self._packed = (key, self._pack(dev))
        return self._packed[1]


class _Block(nn.Module):
    """Parameter holder with the reference Block's names (``proj``, ``norm``); the arithmetic is in ``_Run``."""

    def __init__(self, dim, dim_out, groups):
        super().__init__()
        self.proj = nn.Conv2d(dim, dim_out, 3, padding=1)
        self.norm = nn.GroupNorm(groups, dim_out)


class _Packed:
    """Kernel-layout copies of one block's weights on one device (zero in the padded channels)."""

    def __init__(self, blk, dev):
        lib, st = cabi.lib(), _st(dev)
        ci, co, cip, cop = blk.dim, blk.dim_out, blk.cip, blk.cop
        f32 = dict(dtype=torch.float32, device=dev)
        self.keep = []

        def conv(w, cin, cinp, k):
            """OIHW [co, cin, k, k] -> forward layout [cop][k*k][cinp] and data-gradient layout [cinp][flipped k*k][cop]."""
            w = w.detach().contiguous()
            kk = k * k
            fwd, dgr = torch.zeros(cop * kk * cinp, **f32), torch.zeros(cinp * kk * cop, **f32)
            cabi.check(lib.ld_seg_permute3(w.data_ptr(), fwd.data_ptr(), co, cin, kk, 0, kk * cinp, 1, cinp, st), "permute3")
            cabi.check(lib.ld_seg_permute3(w.data_ptr(), dgr.data_ptr(), co, cin, kk, (kk - 1) * cop, 1, kk * cop, -cop, st),
                       "permute3")
            self.keep.append(w)
            return fwd, dgr

        def vec(v, n, fill=0.0):
            out = torch.full((n,), fill, **f32)
            out[:v.numel()].copy_(v.detach())
            return out

        self.w1f, self.w1d = conv(blk.block1.proj.weight, ci, cip, 3)
        self.w2f, self.w2d = conv(blk.block2.proj.weight, co, cop, 3)
        self.b1, self.b2 = vec(blk.block1.proj.bias, cop), vec(blk.block2.proj.bias, cop)
        self.g1, self.be1 = vec(blk.block1.norm.weight, co), vec(blk.block1.norm.bias, co)
        self.g2, self.be2 = vec(blk.block2.norm.weight, co), vec(blk.block2.norm.bias, co)
        self.wrf = self.wrd = self.br = None
        if blk.has_res_conv:
            self.wrf, self.wrd = conv(blk.res_conv.weight, ci, cip, 1)
            self.br = vec(blk.res_conv.bias, cop)
        n = max(cip, cop)
        self.ones, self.zeros = torch.ones(n, **f32), torch.zeros(n, **f32)


class _Run:
    """The launches of one forward / backward of a block on one device."""

    def __init__(self, blk, packed, dev, B, H, W):
        self.blk, self.p, self.dev, self.B, self.H, self.W = blk, packed, dev, B, H, W
        self.lib, self.st = cabi.lib(), _st(dev)
        self.fill = blk.debug_fill

    def empty(self, *shape, dtype=torch.float32):
        t = torch.empty(*shape, dtype=dtype, device=self.dev)
        if self.fill is not None:
            t.fill_(self.fill)                  # (debug hook: nothing may depend on what a fresh buffer holds)
        return t

    def nhwc(self, t, c, cp):
        """[B, c, H, W] of any strides -> NHWC with pixel stride cp; no copy when it already is that."""
        B, H, W = self.B, self.H, self.W
        if c == cp and t.stride() == (H * W * c, 1, W * c, c) and t.data_ptr() % 16 == 0:
            return t
        out = self.empty(B, H, W, cp)
        sb, sc, sh, sw = t.stride()
        cabi.check(self.lib.ld_dn_pack_nhwc(t.data_ptr(), out.data_ptr(), B, c, H, W, sb, sc, sh, sw, cp, self.st), "pack_nhwc")
        return out

    def conv(self, src, weight, shift, cin, cout, k, residual=None):
        out = self.empty(self.B, self.H, self.W, cout)
        a = cabi.PcConvArgs()
        a.src, a.weight, a.scale, a.shift = src.data_ptr(), weight.data_ptr(), self.p.ones.data_ptr(), shift.data_ptr()
        a.residual, a.out = cabi.ptr(residual), out.data_ptr()
        a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout, a.ksize, a.stride, a.relu = self.B, self.H, self.W, cin, self.H, self.W, \
            cout, k, 1, 0
        cabi.check(self.lib.ld_pc_conv(C.byref(a), self.st), "pc_conv")
        return out

    def gn_work(self):
        return self.empty(int(self.lib.ld_dn_gn_work_bytes(self.B, self.H, self.W, self.blk.dim_out)) // 8, dtype=torch.float64)

    def gn_forward(self, y, gamma, beta, film, residual, out=None):
        blk = self.blk
        stat = self.empty(self.B, blk.groups, 2)
        out = self.empty(self.B, self.H, self.W, blk.cop) if out is None else out
        cabi.check(self.lib.ld_dn_gn_forward(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), cabi.ptr(film), cabi.ptr(residual),
                                             self.gn_work().data_ptr(), stat.data_ptr(), out.data_ptr(), self.B, self.H, self.W,
                                             blk.dim_out, blk.cop, blk.groups, self.st), "dn_gn_forward")
        return out, stat

    def gn_backward(self, dout, y, stat, gamma, beta, film, dy):
        blk = self.blk
        dg, db = self.empty(blk.dim_out), self.empty(blk.dim_out)
        dfilm = None if film is None else self.empty(self.B, 2 * blk.dim_out)
        cabi.check(self.lib.ld_dn_gn_backward(dout.data_ptr(), y.data_ptr(), stat.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                              cabi.ptr(film), self.gn_work().data_ptr(), dg.data_ptr(), db.data_ptr(),
                                              cabi.ptr(dfilm), dy.data_ptr(), self.B, self.H, self.W, blk.dim_out, blk.cop,
                                              blk.groups, self.st), "dn_gn_backward")
        return dg, db, dfilm

    def wgrad(self, dy, a, cin, cinp, k):
        """The weight gradient in the parameter's OIHW and the bias gradient of a convolution with output gradient dy."""
        blk, B, H, W = self.blk, self.B, self.H, self.W
        co, cop, kk = blk.dim_out, blk.cop, k * k
        splits = int(self.lib.ld_seg_wgrad_splits(B, H, W, cinp, cop, k))
        work, dwp = self.empty(splits * cop * kk * cinp), self.empty(cop * kk * cinp)
        cabi.check(self.lib.ld_seg_wgrad(dy.data_ptr(), a.data_ptr(), work.data_ptr(), dwp.data_ptr(), B, H, W, cinp, cop, k,
                                         splits, self.st), "seg_wgrad")
        dw = self.empty(co, cin, k, k)
        cabi.check(self.lib.ld_dn_gather3(dwp.data_ptr(), dw.data_ptr(), co, cin, kk, 0, kk * cinp, 1, cinp, self.st), "gather3")
        db = self.empty(co)
        cabi.check(self.lib.ld_dn_colsum(dy.data_ptr(), self.gn_work().data_ptr(), db.data_ptr(), B, H, W, co, cop, self.st),
                   "dn_colsum")
        return dw, db

    # ------------------------------------------------------------------------------------------------ the two halves
    def forward(self, x, temb):
        blk, p, lib = self.blk, self.p, self.lib
        ci, co, cip, cop = blk.dim, blk.dim_out, blk.cip, blk.cop
        xp = self.nhwc(x, ci, cip)
        film = None
        if temb is not None:
            temb = temb.contiguous()
            w, b = blk.mlp[1].weight.detach().contiguous(), blk.mlp[1].bias.detach().contiguous()
            film = self.empty(self.B, 2 * co)
            cabi.check(lib.ld_dn_time_proj(temb.data_ptr(), w.data_ptr(), b.data_ptr(), film.data_ptr(), self.B, temb.shape[1],
                                           2 * co, self.st), "dn_time_proj")
        y1 = self.conv(xp, p.w1f, p.b1, cip, cop, 3)
        h1, stat1 = self.gn_forward(y1, p.g1, p.be1, film, None)
        y2 = self.conv(h1, p.w2f, p.b2, cop, cop, 3)
        res = self.conv(xp, p.wrf, p.br, cip, cop, 1) if blk.has_res_conv else xp
        out, stat2 = self.gn_forward(y2, p.g2, p.be2, None, res, out=res if blk.has_res_conv else None)
        return out, (xp, y1, y2, stat1, stat2, h1, film, temb)

    def backward(self, dout, saved):
        blk, p, lib = self.blk, self.p, self.lib
        ci, co, cip, cop = blk.dim, blk.dim_out, blk.cip, blk.cop
        xp, y1, y2, stat1, stat2, h1, film, temb = saved
        g = {}
        dop = self.nhwc(dout, co, cop)
        dy2 = self.empty(self.B, self.H, self.W, cop)
        g["block2.norm.weight"], g["block2.norm.bias"], _ = self.gn_backward(dop, y2, stat2, p.g2, p.be2, None, dy2)
        g["block2.proj.weight"], g["block2.proj.bias"] = self.wgrad(dy2, h1, co, cop, 3)
        dy1 = self.conv(dy2, p.w2d, p.zeros, cop, cop, 3)                 # = d h1, then d y1 in place
        g["block1.norm.weight"], g["block1.norm.bias"], dfilm = self.gn_backward(dy1, y1, stat1, p.g1, p.be1, film, dy1)
        g["block1.proj.weight"], g["block1.proj.bias"] = self.wgrad(dy1, xp, ci, cip, 3)
        if blk.has_res_conv:
            g["res_conv.weight"], g["res_conv.bias"] = self.wgrad(dop, xp, ci, cip, 1)
            dskip = self.conv(dop, p.wrd, p.zeros, cop, cip, 1)
        else:
            dskip = dop
        dxp = self.conv(dy1, p.w1d, p.zeros, cop, cip, 3, residual=dskip)
        dtemb = None
        if film is not None:
            w = blk.mlp[1].weight.detach().contiguous()
            T = temb.shape[1]
            dw, db, dtemb = self.empty(2 * co, T), self.empty(2 * co), self.empty(self.B, T)
            cabi.check(lib.ld_dn_time_proj_backward(dfilm.data_ptr(), temb.data_ptr(), w.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                                    dtemb.data_ptr(), self.B, T, 2 * co, self.st), "dn_time_proj_backward")
            g["mlp.1.weight"], g["mlp.1.bias"] = dw, db
        return dxp[..., :ci].permute(0, 3, 1, 2), dtemb, g


class _ResnetBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, blk, names, x, temb, *params):
        with torch.cuda.device(x.device):
            run = _Run(blk, blk._packed_for(x.device), x.device, x.shape[0], x.shape[2], x.shape[3])
            out, saved = run.forward(x, temb)
        ctx.run, ctx.names, ctx.has_temb = run, names, temb is not None
        ctx.save_for_backward(*[t for t in saved if t is not None])
        ctx.present = [t is not None for t in saved]
        return out[..., :blk.dim_out].permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        it = iter(ctx.saved_tensors)
        saved = tuple(next(it) if have else None for have in ctx.present)
        run = ctx.run
        with torch.cuda.device(run.dev):
            run.st = _st(run.dev)
            dx, dtemb, g = run.backward(dout, saved)
        return (None, None, dx, dtemb) + tuple(g.get(n) for n in ctx.names)


class ResnetBlock(_PackedWeights, nn.Module):
    """``ResnetBlock(dim, dim_out, time_emb_dim=None, groups=8)`` of ddpm.py:188-212, forward and backward in HIP (fp32).

    ``forward(x, time_emb=None)``: ``x`` [B, dim, H, W] fp32 on the GPU (``channels_last`` with ``dim`` a multiple of 64 is
    read in place), ``time_emb`` [B, time_emb_dim]; returns [B, dim_out, H, W] (a ``channels_last``-strided view of the
    kernels' NHWC output).  ``dim`` and ``dim_out`` are multiples of 32, ``groups`` divides ``dim_out`` with ``dim_out /
    groups`` a multiple of 4; any H, W >= 1."""

    debug_fill = None       # a float: every buffer the module allocates is filled with it first (tests: NaN)

    def __init__(self, dim, dim_out, *, time_emb_dim=None, groups=8):
        super().__init__()
        if dim <= 0 or dim_out <= 0 or dim % 32 or dim_out % 32:
            raise ValueError(f"ResnetBlock: dim {dim} and dim_out {dim_out} must be positive multiples of 32")
        if groups <= 0 or dim_out % groups or (dim_out // groups) % 4:
            raise ValueError(f"ResnetBlock: groups {groups} must divide dim_out {dim_out} with dim_out / groups a multiple of 4")
        self.dim, self.dim_out, self.groups, self.time_emb_dim = dim, dim_out, groups, time_emb_dim
        self.cip, self.cop = _pad64(dim), _pad64(dim_out)
        self.mlp = nn.Sequential(nn.SiLU(), nn.Linear(time_emb_dim, dim_out * 2)) if time_emb_dim is not None else None
        self.block1 = _Block(dim, dim_out, groups)
        self.block2 = _Block(dim_out, dim_out, groups)
        self.has_res_conv = dim != dim_out
        self.res_conv = nn.Conv2d(dim, dim_out, 1) if self.has_res_conv else nn.Identity()

    def _pack(self, dev):
        return _Packed(self, dev)

    # ------------------------------------------------------------------------------------------------ forward
    def _check(self, x, time_emb):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.dim or x.numel() == 0:
            raise ValueError(f"ResnetBlock: x must be a non-empty [B, {self.dim}, H, W] tensor")
        if x.dtype != torch.float32:
            raise ValueError(f"ResnetBlock: x is {x.dtype}; only float32 is supported (no 16-bit storage in training)")
        if not x.is_cuda:
            raise ValueError("ResnetBlock: x is a CPU tensor; the block runs on HIP kernels only (there is no CPU path)")
        if time_emb is not None:
            if self.mlp is None:
                raise ValueError("ResnetBlock: time_emb given to a block built without time_emb_dim")
            if time_emb.dtype != torch.float32 or time_emb.device != x.device or \
                    tuple(time_emb.shape) != (x.shape[0], self.time_emb_dim):
                raise ValueError(f"ResnetBlock: time_emb must be float32 [{x.shape[0]}, {self.time_emb_dim}] on {x.device}")
        for n, p in self.named_parameters():
            if p.device != x.device or p.dtype != torch.float32:
                raise ValueError(f"ResnetBlock: parameter {n} is {p.dtype} on {p.device}, x is float32 on {x.device}")

    def forward(self, x, time_emb=None):
        self._check(x, time_emb)
        names, params = zip(*self.named_parameters())
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params) or
                                                  (time_emb is not None and time_emb.requires_grad))
        if needs_grad:
            return _ResnetBlockFn.apply(self, names, x, time_emb, *params)
        with torch.no_grad(), torch.cuda.device(x.device):
            run = _Run(self, self._packed_for(x.device), x.device, x.shape[0], x.shape[2], x.shape[3])
            out, _ = run.forward(x.detach(), None if time_emb is None else time_emb.detach())
        return out[..., :self.dim_out].permute(0, 3, 1, 2)
