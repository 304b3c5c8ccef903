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

This file holds what is the block's own: which weights it packs, the GroupNorm and time-projection launches, and the two
launch sequences.  The layout helpers, the packed-weight cache, the launches every module uses, the ``autograd.Function`` and
the input checks are ``trainable.py``'s, shared with the two attention modules.

NOT covered (follow-ups that build on this module's layout; linear attention and RMSNorm are in ``linattn_grad.py``, full
attention is in ``attention_grad.py``, Down/Upsample, the 7x7 stem, the head and the plain 3x3 are in ``resample.py``, the
ResUnet condition encoder is in ``condenc.py``, the time MLP in front of the blocks and ``TrainableUnet`` assembling the
backward of its blocks are in ``unet_grad.py``): 16-bit storage beyond ``act_storage``'s conv-only activations and
``conv_out_storage``'s convolution outputs ``y1`` / ``y2`` (gradients, the result).
"""
import torch
from torch import nn

from . import _cabi as cabi
from .trainable import Run, TrainableModule, check_storage_precision, ones_zeros, pack_conv, pack_vec, pad64, stream


class _Block(nn.Module):
    """Parameter holder with the reference Block's names (``proj``, ``norm``); the arithmetic is in ``_Run``."""

    def __init__(self, dim, dim_out, groups):
        super().__init__()
        self.proj = nn.Conv2d(dim, dim_out, 3, padding=1)
        self.norm = nn.GroupNorm(groups, dim_out)


class _Packed:
    """Kernel-layout copies of one block's weights on one device (zero in the padded channels)."""

    def __init__(self, blk, dev):
        lib, st = cabi.lib(), stream(dev)
        ci, co, cip, cop = blk.dim, blk.dim_out, blk.cip, blk.cop
        self.w1f, self.w1d = pack_conv(lib, st, blk.block1.proj.weight, co, cop, ci, cip, 3, blk.operand_precision)
        self.w2f, self.w2d = pack_conv(lib, st, blk.block2.proj.weight, co, cop, co, cop, 3, blk.operand_precision)
        self.b1, self.b2 = pack_vec(blk.block1.proj.bias, cop), pack_vec(blk.block2.proj.bias, cop)
        self.g1, self.be1 = pack_vec(blk.block1.norm.weight, co), pack_vec(blk.block1.norm.bias, co)
        self.g2, self.be2 = pack_vec(blk.block2.norm.weight, co), pack_vec(blk.block2.norm.bias, co)
        self.wrf = self.wrd = self.br = None
        if blk.has_res_conv:
            self.wrf, self.wrd = pack_conv(lib, st, blk.res_conv.weight, co, cop, ci, cip, 1, blk.operand_precision)
            self.br = pack_vec(blk.res_conv.bias, cop)
        self.ones, self.zeros = ones_zeros(max(cip, cop), dev)


class _Run(Run):
    """The launches of one forward / backward of a block on one device."""

    def gn_work(self):
        return self.work(self.lib.ld_dn_gn_work_bytes(self.B, self.H, self.W, self.mod.dim_out))

    def gn_forward(self, y, gamma, beta, film, residual, out=None, dtype=torch.float32):
        """``dtype``: of a fresh ``out``; ``torch.bfloat16`` for one that only bf16 convolutions read."""
        blk = self.mod
        stat = self.empty(self.B, blk.groups, 2)
        out = self.empty(self.B, self.H, self.W, blk.cop, dtype=dtype) if out is None else out
        what = "dn_gn_forward" + ("_from16" if y.dtype == torch.bfloat16 else "") + ("_to16" if out.dtype == torch.bfloat16 else "")
        fn = getattr(self.lib, "ld_" + what)
        cabi.check(fn(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), cabi.ptr(film), cabi.ptr(residual), self.gn_work().data_ptr(),
                      stat.data_ptr(), out.data_ptr(), self.B, self.H, self.W, blk.dim_out, blk.cop, blk.groups, self.st), what)
        return out, stat

    def gn_backward(self, dout, y, stat, gamma, beta, film, dy):
        blk = self.mod
        dg, db = self.empty(blk.dim_out), self.empty(blk.dim_out)
        dfilm = None if film is None else self.empty(self.B, 2 * blk.dim_out)
        what = "dn_gn_backward" + ("_from16" if y.dtype == torch.bfloat16 else "")
        cabi.check(getattr(self.lib, "ld_" + what)(dout.data_ptr(), y.data_ptr(), stat.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                   cabi.ptr(film), self.gn_work().data_ptr(), dg.data_ptr(), db.data_ptr(),
                                                   cabi.ptr(dfilm), dy.data_ptr(), self.B, self.H, self.W, blk.dim_out, blk.cop,
                                                   blk.groups, self.st), what)
        return dg, db, dfilm

    # ------------------------------------------------------------------------------------------------ the two halves
    def forward(self, x, temb, keep=True):              # (keep: the GroupNorm kernels always write their statistics)
        blk, p, lib = self.mod, self.p, self.lib
        ci, co, cip, cop = blk.dim, blk.dim_out, blk.cip, blk.cop
        # act_storage "bf16": what only the convolutions read is bf16 -- h1 always; the block's own copy of x where a res_conv
        # reads it (without one it is also the fp32 residual of the second GroupNorm; an x read in place is no copy)
        a16 = torch.bfloat16 if self.act16 else torch.float32
        # conv_out_storage "bf16": y1 and y2, which the GroupNorm launches (forward and backward) read, are bf16 -- written
        # rounded by their convolutions; res_conv's output, the second GroupNorm's residual and output buffer, stays fp32
        y16 = torch.bfloat16 if self.y16 else torch.float32
        xp = self.nhwc(x, ci, cip, dtype=a16 if blk.has_res_conv else torch.float32)
        film = None
        if temb is not None:
            temb = temb.contiguous()
            w, b = blk.mlp[1].weight.detach().contiguous(), blk.mlp[1].bias.detach().contiguous()
            film = self.empty(self.B, 2 * co)
            cabi.check(lib.ld_dn_time_proj(temb.data_ptr(), w.data_ptr(), b.data_ptr(), film.data_ptr(), self.B, temb.shape[1],
                                           2 * co, self.st), "dn_time_proj")
        y1 = self.conv(xp, p.w1f, p.b1, cip, cop, 3, out_dtype=y16)
        h1, stat1 = self.gn_forward(y1, p.g1, p.be1, film, None, dtype=a16)
        y2 = self.conv(h1, p.w2f, p.b2, cop, cop, 3, out_dtype=y16)
        res = self.conv(xp, p.wrf, p.br, cip, cop, 1) if blk.has_res_conv else xp
        out, stat2 = self.gn_forward(y2, p.g2, p.be2, None, res, out=res if blk.has_res_conv else None)
        return out, (xp, y1, y2, stat1, stat2, h1, film, temb)

    def backward(self, dout, saved):
        blk, p, lib = self.mod, self.p, self.lib
        ci, co, cip, cop = blk.dim, blk.dim_out, blk.cip, blk.cop
        xp, y1, y2, stat1, stat2, h1, film, temb = saved
        g = {}
        dop = self.nhwc(dout, co, cop)
        dy2 = self.empty(self.B, self.H, self.W, cop)
        g["block2.norm.weight"], g["block2.norm.bias"], _ = self.gn_backward(dop, y2, stat2, p.g2, p.be2, None, dy2)
        g["block2.proj.weight"], g["block2.proj.bias"] = self.wgrad(dy2, h1, co, cop, co, cop, 3), self.bias_grad(dy2, co, cop)
        dy1 = self.conv(dy2, p.w2d, p.zeros, cop, cop, 3)                 # = d h1, then d y1 in place
        g["block1.norm.weight"], g["block1.norm.bias"], dfilm = self.gn_backward(dy1, y1, stat1, p.g1, p.be1, film, dy1)
        g["block1.proj.weight"], g["block1.proj.bias"] = self.wgrad(dy1, xp, co, cop, ci, cip, 3), self.bias_grad(dy1, co, cop)
        if blk.has_res_conv:
            g["res_conv.weight"], g["res_conv.bias"] = self.wgrad(dop, xp, co, cop, ci, cip, 1), self.bias_grad(dop, co, cop)
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
        return dxp[..., :ci].permute(0, 3, 1, 2), (dtemb,), g


class ResnetBlock(TrainableModule):
    """``ResnetBlock(dim, dim_out, time_emb_dim=None, groups=8)`` of ddpm.py:188-212, forward and backward in HIP (fp32).

    ``forward(x, time_emb=None)``: ``x`` [B, dim, H, W] fp32 on the GPU (``channels_last`` with ``dim`` a multiple of 64 is
    read in place), ``time_emb`` [B, time_emb_dim]; returns [B, dim_out, H, W] (a ``channels_last``-strided view of the
    kernels' NHWC output).  ``dim`` and ``dim_out`` are multiples of 32, ``groups`` divides ``dim_out`` with ``dim_out /
    groups`` a multiple of 4; any H, W >= 1.

    ``act_storage = "bf16"`` (with ``conv_precision = "bf16"``; refused with ``ValueError`` otherwise): block1's GroupNorm ->
    FiLM -> SiLU output, and the block's padded NHWC copy of ``x`` when it has a ``res_conv`` and makes one, are written, read
    and saved for the backward as bf16 -- what every convolution that reads them rounds them to anyway, so the output and
    every gradient keep their bits.

    ``conv_out_storage = "bf16"`` (with ``conv_precision = "bf16"`` as well, independent of ``act_storage``): the outputs
    ``y1`` / ``y2`` of the two 3x3 convolutions are written as bf16 -- the fp32 epilogue value rounded to nearest even --, and
    GroupNorm's statistics, its apply pass and both passes of its backward read that tensor, which is also what autograd keeps.
    The backward is the exact gradient of the forward that was computed (it uses the stored ``y``; the rounding is passed
    through as the identity), so the output and the gradients move by about what the bf16 convolutions move them, and a
    step stays reproducible bit for bit.  ``res_conv``'s output, the statistics, all gradients and the result stay fp32."""

    Run = _Run
    ACT_STORAGES = ("fp32", "bf16")
    CONV_OUT_STORAGES = ("fp32", "bf16")

    def __init__(self, dim, dim_out, *, time_emb_dim=None, groups=8):
        super().__init__()
        if dim <= 0 or dim_out <= 0 or dim % 32 or dim_out % 32:
            raise ValueError(f"ResnetBlock: dim {dim} and dim_out {dim_out} must be positive multiples of 32")
        if groups <= 0 or dim_out % groups or (dim_out // groups) % 4:
            raise ValueError(f"ResnetBlock: groups {groups} must divide dim_out {dim_out} with dim_out / groups a multiple of 4")
        self.dim, self.dim_out, self.groups, self.time_emb_dim = dim, dim_out, groups, time_emb_dim
        self.cip, self.cop = pad64(dim), pad64(dim_out)
        self.mlp = nn.Sequential(nn.SiLU(), nn.Linear(time_emb_dim, dim_out * 2)) if time_emb_dim is not None else None
        self.block1 = _Block(dim, dim_out, groups)
        self.block2 = _Block(dim_out, dim_out, groups)
        self.has_res_conv = dim != dim_out
        self.res_conv = nn.Conv2d(dim, dim_out, 1) if self.has_res_conv else nn.Identity()

    def _pack(self, dev):
        return _Packed(self, dev)

    def _check_extra(self, x, time_emb):
        if time_emb is not None:
            if self.mlp is None:
                raise ValueError("ResnetBlock: time_emb given to a block built without time_emb_dim")
            if time_emb.dtype != torch.float32 or time_emb.device != x.device or \
                    tuple(time_emb.shape) != (x.shape[0], self.time_emb_dim):
                raise ValueError(f"ResnetBlock: time_emb must be float32 [{x.shape[0]}, {self.time_emb_dim}] on {x.device}")

    def forward(self, x, time_emb=None):
        for switch in ("act_storage", "conv_out_storage"):
            check_storage_precision("ResnetBlock", switch, getattr(self, switch), self.conv_precision)
        return super().forward(x, time_emb)
