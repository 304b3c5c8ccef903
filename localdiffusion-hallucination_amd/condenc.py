"""The ResUnet condition encoder (``Unet.cond_model``, unet_model.py:8-51 and :91-137), trainable on HIP kernels: the fifth
slice of the denoiser's backward pass.

``BasicBlock(input_dim, mid_dim, output_dim, pool=False)`` is a ``TrainableModule`` (``trainable.py``) with the reference's
``state_dict`` names (``convblock.0/.1/.3/.4`` and ``identity.0/.1``): ``relu(GN(conv3(relu(GN(conv3(x))))) + GN(conv3_id(x)))``
with GroupNorm at 16 groups on the statistics of the batch, then ``MaxPool2d(2)`` when ``pool`` is set -- the pool is the end
of the block's launch sequence (as in ``unet.py``'s ``_Plan._basic_block``), so the module tree keeps the reference's
parameter names.  ``ResUnet(data)`` is the four (or three) blocks in ``nn.Sequential``s of the reference's names.  fp32,
activations NHWC with a pixel stride of ``pad64(channels)``, no host synchronisation, no atomics, the same bits on every call.

Every convolution and its gradients are the launches the other modules use (``ld_pc_conv``, ``ld_seg_wgrad``,
``ld_dn_colsum``), the pool and its backward are ``ld_seg_pool`` / ``ld_seg_pool_backward`` on the padded pixel (the padding
is zero and stays zero); what is new is in ``csrc/condenc_grad.hip``:

* ``ld_dn_gnr_forward`` / ``ld_dn_gnr_backward``: GroupNorm -> ReLU at any even number of channels per group (2 at 32
  channels), in the one-operand form (``convblock.1``) and the two-operand form of the block's tail, ``relu(GN_a(y) +
  GN_b(y2))``.  The backward takes the ReLU mask from the saved result (``out > 0``) and gives both GroupNorms' gradients
  from one pass.
* ``ld_dn_im2col3``: the first block reads a 1..4-channel image; its two 3x3 convolutions (``convblock.0``, ``identity.0``)
  are 1x1 convolutions over the 9 in_channels columns of one shared im2col tensor, their weights the OIHW parameters as they
  lie in memory.  The im2col tensor is recomputed in the backward.  **The image block has no input gradient**: its input is
  data.  An ``x`` that requires grad is refused; the backward returns ``None`` for x.

The two data gradients of a non-image block (through ``convblock.0`` and through ``identity.0``) are summed by passing one as
the other convolution's ``residual``.

``TrainableUnet`` (``unet_grad.py``) puts ``ResUnet`` in ``Unet.cond_model``'s place.  Not covered yet: a fused optimiser /
EMA step, a ``Trainer``, and 16-bit storage.
"""
import torch
from torch import nn

from . import _cabi as cabi
from .trainable import Run, TrainableModule, ones_zeros, pack_conv, pack_vec, pad64, stream

GROUPS = 16                     # unet_model.py:6 (group_num)
FILTERS = (32, 32, 64, 128, 256)
DATA = ("mri", "mnist", "mvtec", "mvtecGray", "mvtecSR")
EARLY_EXIT = ("mnist", "mvtecSR")


class _Packed:
    pass


class _Run(Run):
    """The launches of one forward / backward of a block on one device.  H, W are x's; the pooled result is H/2 x W/2."""

    def gn_work(self, c):
        return self.work(self.lib.ld_dn_gnr_work_bytes(self.B, self.H, self.W, c, GROUPS))

    def gn_forward(self, y, gamma, beta, c, cp, y2=None, gamma2=None, beta2=None):
        """relu(GN(y) (+ GN(y2))) and the statistics of each operand."""
        stat = self.empty(self.B, GROUPS, 2)
        stat2 = None if y2 is None else self.empty(self.B, GROUPS, 2)
        out = self.empty(self.B, self.H, self.W, cp)
        cabi.check(self.lib.ld_dn_gnr_forward(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), cabi.ptr(y2), cabi.ptr(gamma2),
                                              cabi.ptr(beta2), self.gn_work(c).data_ptr(), stat.data_ptr(), cabi.ptr(stat2),
                                              out.data_ptr(), self.B, self.H, self.W, c, cp, GROUPS, 1, self.st), "dn_gnr_forward")
        return out, stat, stat2

    def gn_backward(self, dout, act, y, stat, gamma, dy, c, cp, y2=None, stat2=None, gamma2=None, dy2=None):
        """(dgamma, dbeta) of each operand; dy (and dy2) are written, dy may be dout."""
        g = [self.empty(c) for _ in range(2 if y2 is None else 4)]
        g2 = g[2:] if y2 is not None else (None, None)
        cabi.check(self.lib.ld_dn_gnr_backward(dout.data_ptr(), act.data_ptr(), y.data_ptr(), stat.data_ptr(), gamma.data_ptr(),
                                               cabi.ptr(y2), cabi.ptr(stat2), cabi.ptr(gamma2), self.gn_work(c).data_ptr(),
                                               g[0].data_ptr(), g[1].data_ptr(), dy.data_ptr(), cabi.ptr(g2[0]), cabi.ptr(g2[1]),
                                               cabi.ptr(dy2), self.B, self.H, self.W, c, cp, GROUPS, 1, self.st),
                   "dn_gnr_backward")
        return g

    def im2col(self, x):
        m = self.mod
        out = self.empty(self.B, self.H, self.W, m.cik)
        sb, sc, sh, sw = x.stride()
        cabi.check(self.lib.ld_dn_im2col3(x.data_ptr(), out.data_ptr(), self.B, m.dim, self.H, self.W, sb, sc, sh, sw, m.cik,
                                          self.st), "dn_im2col3")
        return out

    # ------------------------------------------------------------------------------------------------ the two halves
    def forward(self, x, keep=True):
        m, p = self.mod, self.p
        # the input of the block's first two convolutions: the image's im2col columns under a 1x1, or x under a 3x3
        xin, src = (x, self.im2col(x)) if m.image else 2 * (self.nhwc(x, m.dim, m.cik),)
        y1 = self.conv(src, p.w1f, p.b1, m.cik, m.cmp, m.k_in)
        h1, stat1, _ = self.gn_forward(y1, p.g1, p.be1, m.mid_dim, m.cmp)
        y2 = self.conv(h1, p.w2f, p.b2, m.cmp, m.cop, 3)
        y3 = self.conv(src, p.w3f, p.b3, m.cik, m.cop, m.k_in)
        act, stat2, stat3 = self.gn_forward(y2, p.g2, p.be2, m.dim_out, m.cop, y3, p.g3, p.be3)
        out = act
        if m.pool:
            out = self.empty(self.B, self.H // 2, self.W // 2, m.cop)
            cabi.check(self.lib.ld_seg_pool(act.data_ptr(), out.data_ptr(), self.B, self.H // 2, self.W // 2, m.cop, self.st),
                       "seg_pool")
        return out, (xin, y1, stat1, h1, y2, stat2, y3, stat3, act)

    def backward(self, dout, saved):
        m, p = self.mod, self.p
        xin, y1, stat1, h1, y2, stat2, y3, stat3, act = saved
        ci, mid, co, cik, cmp_, cop = m.dim, m.mid_dim, m.dim_out, m.cik, m.cmp, m.cop
        g = {}
        if m.pool:
            hw = (self.H // 2, self.W // 2)
            dop = self.nhwc(dout, co, cop, hw)
            dact = self.empty(self.B, self.H, self.W, cop)
            cabi.check(self.lib.ld_seg_pool_backward(act.data_ptr(), dop.data_ptr(), None, dact.data_ptr(), self.B, hw[0], hw[1],
                                                     cop, self.st), "seg_pool_backward")
            dy2 = dact                                                # (our own buffer: the GroupNorm backward works in place)
        else:
            dact = self.nhwc(dout, co, cop)
            dy2 = self.empty(self.B, self.H, self.W, cop)             # (dact may be the caller's tensor)
        dy3 = self.empty(self.B, self.H, self.W, cop)
        (g["convblock.4.weight"], g["convblock.4.bias"], g["identity.1.weight"],
         g["identity.1.bias"]) = self.gn_backward(dact, act, y2, stat2, p.g2, dy2, co, cop, y3, stat3, p.g3, dy3)
        g["convblock.3.weight"], g["convblock.3.bias"] = self.wgrad(dy2, h1, co, cop, mid, cmp_, 3), self.bias_grad(dy2, co, cop)
        dy1 = self.conv(dy2, p.w2d, p.zeros, cop, cmp_, 3)                # = d h1, then d y1 in place
        g["convblock.1.weight"], g["convblock.1.bias"] = self.gn_backward(dy1, h1, y1, stat1, p.g1, dy1, mid, cmp_)
        g["convblock.0.bias"], g["identity.0.bias"] = self.bias_grad(dy1, mid, cmp_), self.bias_grad(dy3, co, cop)
        if m.image:
            col = self.im2col(xin)
            g["convblock.0.weight"] = self.wgrad(dy1, col, mid, cmp_, 9 * ci, cik, 1).view(mid, ci, 3, 3)
            g["identity.0.weight"] = self.wgrad(dy3, col, co, cop, 9 * ci, cik, 1).view(co, ci, 3, 3)
            return None, (), g
        g["convblock.0.weight"] = self.wgrad(dy1, xin, mid, cmp_, ci, cik, 3)
        g["identity.0.weight"] = self.wgrad(dy3, xin, co, cop, ci, cik, 3)
        dskip = self.conv(dy3, p.w3d, p.zeros, cop, cik, 3)
        dxp = self.conv(dy1, p.w1d, p.zeros, cmp_, cik, 3, residual=dskip)
        return dxp[..., :ci].permute(0, 3, 1, 2), (), g


class BasicBlock(TrainableModule):
    """``BasicBlock(input_dim, mid_dim, output_dim)`` of unet_model.py:8-51 as ``ResUnet`` builds it (stride 1, residual, no
    squeeze-excite, ``input_dim != output_dim``), forward and backward in HIP (fp32); ``pool=True`` appends ``MaxPool2d(2)``.
    Parameters: ``convblock.0/.3`` and ``identity.0`` (3x3 convolutions), ``convblock.1/.4`` and ``identity.1`` (GroupNorm,
    16 groups, eps 1e-5, always the statistics of the batch).

    ``forward(x)``: ``x`` [B, input_dim, H, W] fp32 on the GPU, any H, W >= 1 (even with ``pool``); returns [B, output_dim, H,
    W] or [B, output_dim, H/2, W/2] (a ``channels_last``-strided view of the kernels' NHWC output).  ``mid_dim`` and
    ``output_dim`` are multiples of 32; ``input_dim`` is a multiple of 32 (``channels_last`` with a multiple of 64 is read in
    place) or 1..4, the image block: its input is data, **it has no input gradient**, an ``x`` that requires grad raises
    ``ValueError``, and x may have any strides."""

    Run = _Run

    def __init__(self, input_dim, mid_dim, output_dim, pool=False):
        super().__init__()
        dims = (input_dim, mid_dim, output_dim)
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in dims):
            raise ValueError(f"BasicBlock: input_dim, mid_dim and output_dim must be ints, got {dims}")
        if mid_dim <= 0 or output_dim <= 0 or mid_dim % 32 or output_dim % 32:
            raise ValueError(f"BasicBlock: mid_dim {mid_dim} and output_dim {output_dim} must be positive multiples of 32")
        if not (1 <= input_dim <= 4 or (input_dim > 0 and input_dim % 32 == 0)):
            raise ValueError(f"BasicBlock: input_dim {input_dim} must be 1..4 (an image) or a positive multiple of 32")
        if input_dim == output_dim:
            raise ValueError(f"BasicBlock: input_dim == output_dim == {input_dim} (the Identity shortcut) is not built: ResUnet "
                             "never makes it")
        self.dim, self.mid_dim, self.dim_out, self.pool = input_dim, mid_dim, output_dim, bool(pool)
        self.image = input_dim <= 4
        # the first two convolutions' input channels and kernel size as launched: im2col columns under a 1x1, or x under a 3x3
        self.cik, self.k_in = (pad64(9 * input_dim), 1) if self.image else (pad64(input_dim), 3)
        self.cmp, self.cop = pad64(mid_dim), pad64(output_dim)
        self.convblock = nn.Sequential(nn.Conv2d(input_dim, mid_dim, 3, padding=1), nn.GroupNorm(GROUPS, mid_dim), nn.ReLU(),
                                       nn.Conv2d(mid_dim, output_dim, 3, padding=1), nn.GroupNorm(GROUPS, output_dim))
        self.identity = nn.Sequential(nn.Conv2d(input_dim, output_dim, 3, padding=1), nn.GroupNorm(GROUPS, output_dim))

    def _pack(self, dev):
        lib, st, p = cabi.lib(), stream(dev), _Packed()
        cb, idn = self.convblock, self.identity
        mid, co = self.mid_dim, self.dim_out
        if self.image:                                          # OIHW is [out][9 input_dim] in memory: a 1x1 over the columns
            p.w1f, p.w1d = pack_conv(lib, st, cb[0].weight, mid, self.cmp, 9 * self.dim, self.cik, 1, self.operand_precision)
            p.w3f, p.w3d = pack_conv(lib, st, idn[0].weight, co, self.cop, 9 * self.dim, self.cik, 1, self.operand_precision)
        else:
            p.w1f, p.w1d = pack_conv(lib, st, cb[0].weight, mid, self.cmp, self.dim, self.cik, 3, self.operand_precision)
            p.w3f, p.w3d = pack_conv(lib, st, idn[0].weight, co, self.cop, self.dim, self.cik, 3, self.operand_precision)
        p.w2f, p.w2d = pack_conv(lib, st, cb[3].weight, co, self.cop, mid, self.cmp, 3, self.operand_precision)
        p.b1, p.b2, p.b3 = pack_vec(cb[0].bias, self.cmp), pack_vec(cb[3].bias, self.cop), pack_vec(idn[0].bias, self.cop)
        p.g1, p.be1 = pack_vec(cb[1].weight, mid), pack_vec(cb[1].bias, mid)
        p.g2, p.be2 = pack_vec(cb[4].weight, co), pack_vec(cb[4].bias, co)
        p.g3, p.be3 = pack_vec(idn[1].weight, co), pack_vec(idn[1].bias, co)
        p.ones, p.zeros = ones_zeros(max(self.cik, self.cmp, self.cop), dev)
        return p

    def _check_extra(self, x):
        if self.pool and (x.shape[2] % 2 or x.shape[3] % 2):
            raise ValueError(f"BasicBlock: H {x.shape[2]} and W {x.shape[3]} must be even (pool=True)")
        if self.image and x.requires_grad:
            raise ValueError("BasicBlock: the image block (input_dim 1..4) has no input gradient, its input is data; x must not "
                             "require grad")


class ResUnet(nn.Module):
    """``ResUnet(data='mri')`` of unet_model.py:91-137, the denoiser's condition encoder, forward and backward in HIP (fp32):
    ``residual_conv1``, ``residual_conv2``, ``residual_conv3`` and, unless ``data`` is 'mnist' or 'mvtecSR', ``mid_conv``,
    each an ``nn.Sequential`` of one ``BasicBlock``, so that the ``state_dict`` is the reference ``Unet``'s under
    ``cond_model.``.  The reference's three ``MaxPool2d(2)`` belong to blocks 1, 2 and (when there is a fourth) 3.

    ``forward(x)``: ``x`` [B, in_channels, H, W] fp32 on the GPU (data: it must not require grad), in_channels 3 for 'mvtec'
    and 'mvtecSR' and 1 otherwise; returns [B, 256, H/8, W/8] (H, W divisible by 8), or for 'mnist' and 'mvtecSR' [B, 128,
    H/4, W/4] (H, W divisible by 4)."""

    def __init__(self, data="mri"):
        super().__init__()
        if data not in DATA:
            raise ValueError(f"ResUnet: data {data!r} is not one of {', '.join(repr(d) for d in DATA)}")
        self.data = data
        self.in_channels = 1 if "mvtecGray" in data else 3 if "mvtec" in data else 1       # unet_model.py:94-99
        self.filters = list(FILTERS)
        self.early_exit = data in EARLY_EXIT
        f = self.filters
        self.residual_conv1 = nn.Sequential(BasicBlock(self.in_channels, f[0], f[1], pool=True))
        self.residual_conv2 = nn.Sequential(BasicBlock(f[1], f[1], f[2], pool=True))
        self.residual_conv3 = nn.Sequential(BasicBlock(f[2], f[2], f[3], pool=not self.early_exit))
        if not self.early_exit:
            self.mid_conv = nn.Sequential(BasicBlock(f[3], f[3], f[4]))

    def forward(self, x):
        div = 4 if self.early_exit else 8
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.in_channels or x.numel() == 0:
            raise ValueError(f"ResUnet: x must be a non-empty [B, {self.in_channels}, H, W] tensor")
        if x.shape[2] % div or x.shape[3] % div:
            raise ValueError(f"ResUnet: H {x.shape[2]} and W {x.shape[3]} must be divisible by {div} (data {self.data!r})")
        x = self.residual_conv3(self.residual_conv2(self.residual_conv1(x)))
        return x if self.early_exit else self.mid_conv(x)
