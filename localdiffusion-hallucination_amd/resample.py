"""The layers between the blocks of the denoiser, trainable on HIP kernels: the fourth slice of its backward pass.

``Downsample(dim, dim_out)`` (ddpm.py:120-124), ``Upsample(dim, dim_out)`` (ddpm.py:114-118) and ``Conv2d`` in exactly the
three uses ``Unet`` makes of it -- the 3x3 in place of the last stage's Down/Upsample, the 7x7 stem ``init_conv`` and the
1x1 head ``final_conv``.  Each is a ``TrainableModule`` (``trainable.py``) with the reference's ``state_dict`` names
(``1.weight`` / ``1.bias`` for the two ``nn.Sequential``s, ``weight`` / ``bias`` for ``Conv2d``): fp32, activations NHWC with
a pixel stride of ``pad64(channels)``, no host synchronisation, no atomics, the same bits on every call.

Every convolution and its gradients are the launches the other modules use (``ld_pc_conv``, ``ld_seg_wgrad``,
``ld_dn_colsum``) at the map size of the layer; what is new is in ``csrc/resample_grad.hip``:

* Downsample is ``ld_dn_space_to_depth`` and a 1x1 convolution over 4 dim channels.  The kernel's channel order is (p1 p2 c),
  which makes 16-byte copies; the reference's (c p1 p2) is met in the weight packing (``ld_seg_permute3`` with (d0, d1, d2) =
  (dim_out, dim, 4)) and the weight gradient gathered back the same way.  The backward recomputes the rearranged x instead of
  keeping it; dx is ``ld_pc_conv`` on the transposed weight, then ``ld_dn_depth_to_space``.
* Upsample is ``ld_dn_upsample2x`` and a 3x3 convolution at 2H x 2W.  Only x is saved (a quarter of the upsampled map, which
  the backward recomputes for the weight gradient); dx is ``ld_pc_conv`` on the flipped, transposed weight at 2H x 2W, then
  ``ld_dn_upsample2x_backward``: ((g[2h][2w] + g[2h][2w+1]) + g[2h+1][2w]) + g[2h+1][2w+1].
* The stem is ``ld_dn_im2col`` (49 in_channels columns per pixel, padded to a multiple of 64) and a 1x1 convolution whose
  weight is the OIHW parameter as it lies in memory; the im2col tensor is recomputed in the backward.  **The stem has no
  input gradient**: its input is data.  An ``x`` that requires grad is refused; the backward returns ``None`` for x.
* The head is ``ld_dn_head_forward`` / ``ld_dn_head_backward``: the result is the kernels' NCHW tensor itself, contiguous
  (padding 1..6 output channels to 64 would write 64 times the bytes).
"""
import torch
from torch import nn

from . import _cabi as cabi
from .trainable import Run, TrainableModule, as_conv_precision, ones_zeros, pack_conv, pack_vec, pad64, stream


class _Packed:
    pass


def _dims(name, dim, dim_out):
    dim_out = dim if dim_out is None else dim_out
    if dim <= 0 or dim_out <= 0 or dim % 32 or dim_out % 32:
        raise ValueError(f"{name}: dim {dim} and dim_out {dim_out} must be positive multiples of 32")
    return dim, dim_out


# ------------------------------------------------------------------------------------------------------ Downsample
class _DownRun(Run):
    """H, W are x's; the convolution works at H/2 x W/2 on 4 dim channels."""

    def s2d(self, xp):
        m = self.mod
        out = self.empty(self.B, self.H // 2, self.W // 2, 4 * m.dim)
        cabi.check(self.lib.ld_dn_space_to_depth(xp.data_ptr(), out.data_ptr(), self.B, self.H // 2, self.W // 2, m.dim, m.cip,
                                                 self.st), "dn_space_to_depth")
        return out

    def forward(self, x, keep=True):
        m, p = self.mod, self.p
        xp = self.nhwc(x, m.dim, m.cip)
        out = self.conv(self.s2d(xp), p.wf, p.b, 4 * m.dim, m.cop, 1, hw=(self.H // 2, self.W // 2))
        return out, (xp,)

    def backward(self, dout, saved):
        m, p = self.mod, self.p
        (xp,) = saved
        hw = (self.H // 2, self.W // 2)
        dop = self.nhwc(dout, m.dim_out, m.cop, hw)
        g = {"1.bias": self.bias_grad(dop, m.dim_out, m.cop, hw)}
        dwp = self.wgrad_packed(dop, self.s2d(xp), m.cop, 4 * m.dim, 1, hw)
        dw = self.empty(m.dim_out, 4 * m.dim, 1, 1)                  # [dim_out][c][p] <- dwp[o][p dim + c]
        cabi.check(self.lib.ld_dn_gather3(dwp.data_ptr(), dw.data_ptr(), m.dim_out, m.dim, 4, 0, 4 * m.dim, 1, m.dim, self.st),
                   "gather3")
        g["1.weight"] = dw
        gs = self.conv(dop, p.wd, p.zeros, m.cop, 4 * m.dim, 1, hw=hw)
        dxp = self.empty(self.B, self.H, self.W, m.cip)
        cabi.check(self.lib.ld_dn_depth_to_space(gs.data_ptr(), dxp.data_ptr(), self.B, hw[0], hw[1], m.dim, m.cip, self.st),
                   "dn_depth_to_space")
        return dxp[..., :m.dim].permute(0, 3, 1, 2), (), g


class Downsample(TrainableModule):
    """``Downsample(dim, dim_out=None)`` of ddpm.py:120-124, forward and backward in HIP (fp32): 'b c (h p1) (w p2) -> b (c p1
    p2) h w' and ``Conv2d(4 dim, dim_out, 1)``, the parameters ``1.weight`` [dim_out, 4 dim, 1, 1] and ``1.bias``.

    ``forward(x)``: ``x`` [B, dim, H, W] fp32 on the GPU with H and W even (``channels_last`` with ``dim`` a multiple of 64 is
    read in place); returns [B, dim_out, H/2, W/2] (a ``channels_last``-strided view of the kernels' NHWC output).  ``dim`` and
    ``dim_out`` are multiples of 32."""

    Run = _DownRun

    def __init__(self, dim, dim_out=None):
        super().__init__()
        self.dim, self.dim_out = _dims("Downsample", dim, dim_out)
        self.cip, self.cop = pad64(self.dim), pad64(self.dim_out)
        self.add_module("1", nn.Conv2d(4 * self.dim, self.dim_out, 1))

    def _pack(self, dev):
        lib, st, p = cabi.lib(), stream(dev), _Packed()
        conv = self._modules["1"]
        C4, co, cop = 4 * self.dim, self.dim_out, self.cop
        w = conv.weight.detach().contiguous()                        # [co][c][p], p = p1 2 + p2
        p.wf, p.wd = w.new_zeros(cop * C4), w.new_zeros(C4 * cop)    # [cop][p dim + c] and its transpose [p dim + c][cop]
        cabi.check(lib.ld_seg_permute3(w.data_ptr(), p.wf.data_ptr(), co, self.dim, 4, 0, C4, 1, self.dim, st), "permute3")
        cabi.check(lib.ld_seg_permute3(w.data_ptr(), p.wd.data_ptr(), co, self.dim, 4, 0, 1, cop, self.dim * cop, st), "permute3")
        p.wf, p.wd = (as_conv_precision(t, self.operand_precision) for t in (p.wf, p.wd))     # (its own layout: not pack_conv's)
        p.b = pack_vec(conv.bias, cop)
        p.ones, p.zeros = ones_zeros(max(C4, cop), dev)
        return p

    def _check_extra(self, x):
        if x.shape[2] % 2 or x.shape[3] % 2:
            raise ValueError(f"Downsample: H {x.shape[2]} and W {x.shape[3]} must be even")


# ------------------------------------------------------------------------------------------------------ Upsample
class _UpRun(Run):
    """H, W are x's; the convolution works at 2H x 2W."""

    def up(self, xp):
        m = self.mod
        out = self.empty(self.B, 2 * self.H, 2 * self.W, m.cip)
        cabi.check(self.lib.ld_dn_upsample2x(xp.data_ptr(), out.data_ptr(), self.B, self.H, self.W, m.dim, m.cip, self.st),
                   "dn_upsample2x")
        return out

    def forward(self, x, keep=True):
        m, p = self.mod, self.p
        xp = self.nhwc(x, m.dim, m.cip)
        out = self.conv(self.up(xp), p.wf, p.b, m.cip, m.cop, 3, hw=(2 * self.H, 2 * self.W))
        return out, (xp,)

    def backward(self, dout, saved):
        m, p = self.mod, self.p
        (xp,) = saved
        hw = (2 * self.H, 2 * self.W)
        dop = self.nhwc(dout, m.dim_out, m.cop, hw)
        g = {"1.bias": self.bias_grad(dop, m.dim_out, m.cop, hw),
             "1.weight": self.wgrad(dop, self.up(xp), m.dim_out, m.cop, m.dim, m.cip, 3, hw)}
        gu = self.conv(dop, p.wd, p.zeros, m.cop, m.cip, 3, hw=hw)
        dxp = self.empty(self.B, self.H, self.W, m.cip)
        cabi.check(self.lib.ld_dn_upsample2x_backward(gu.data_ptr(), dxp.data_ptr(), self.B, self.H, self.W, m.dim, m.cip,
                                                      self.st), "dn_upsample2x_backward")
        return dxp[..., :m.dim].permute(0, 3, 1, 2), (), g


class Upsample(TrainableModule):
    """``Upsample(dim, dim_out=None)`` of ddpm.py:114-118, forward and backward in HIP (fp32): nearest x 2 and ``Conv2d(dim,
    dim_out, 3, padding=1)``, the parameters ``1.weight`` and ``1.bias``.

    ``forward(x)``: ``x`` [B, dim, H, W] fp32 on the GPU, any H, W >= 1 (``channels_last`` with ``dim`` a multiple of 64 is read
    in place); returns [B, dim_out, 2H, 2W] (a ``channels_last``-strided view of the kernels' NHWC output).  ``dim`` and
    ``dim_out`` are multiples of 32."""

    Run = _UpRun

    def __init__(self, dim, dim_out=None):
        super().__init__()
        self.dim, self.dim_out = _dims("Upsample", dim, dim_out)
        self.cip, self.cop = pad64(self.dim), pad64(self.dim_out)
        self.add_module("1", nn.Conv2d(self.dim, self.dim_out, 3, padding=1))

    def _pack(self, dev):
        lib, st, p = cabi.lib(), stream(dev), _Packed()
        conv = self._modules["1"]
        p.wf, p.wd = pack_conv(lib, st, conv.weight, self.dim_out, self.cop, self.dim, self.cip, 3, self.operand_precision)
        p.b = pack_vec(conv.bias, self.cop)
        p.ones, p.zeros = ones_zeros(max(self.cip, self.cop), dev)
        return p


# ------------------------------------------------------------------------------------------------------ Conv2d
class _Conv3Run(Run):
    def forward(self, x, keep=True):
        m, p = self.mod, self.p
        xp = self.nhwc(x, m.dim, m.cip)
        return self.conv(xp, p.wf, p.b, m.cip, m.cop, 3), (xp,)

    def backward(self, dout, saved):
        m, p = self.mod, self.p
        (xp,) = saved
        dop = self.nhwc(dout, m.dim_out, m.cop)
        g = {"bias": self.bias_grad(dop, m.dim_out, m.cop), "weight": self.wgrad(dop, xp, m.dim_out, m.cop, m.dim, m.cip, 3)}
        dxp = self.conv(dop, p.wd, p.zeros, m.cop, m.cip, 3)
        return dxp[..., :m.dim].permute(0, 3, 1, 2), (), g


class _StemRun(Run):
    def im2col(self, x):
        m = self.mod
        out = self.empty(self.B, self.H, self.W, m.cip)
        sb, sc, sh, sw = x.stride()
        cabi.check(self.lib.ld_dn_im2col(x.data_ptr(), out.data_ptr(), self.B, m.dim, self.H, self.W, sb, sc, sh, sw, m.cip,
                                         self.st), "dn_im2col")
        return out

    def forward(self, x, keep=True):
        m, p = self.mod, self.p
        return self.conv(self.im2col(x), p.wf, p.b, m.cip, m.cop, 1), (x,)

    def backward(self, dout, saved):
        m = self.mod
        (x,) = saved
        dop = self.nhwc(dout, m.dim_out, m.cop)
        dw = self.wgrad(dop, self.im2col(x), m.dim_out, m.cop, 49 * m.dim, m.cip, 1)
        return None, (), {"bias": self.bias_grad(dop, m.dim_out, m.cop), "weight": dw.view(m.dim_out, m.dim, 7, 7)}


class _HeadRun(Run):
    def forward(self, x, keep=True):
        m, p = self.mod, self.p
        xp = self.nhwc(x, m.dim, m.cip)
        out = self.empty(self.B, m.dim_out, self.H, self.W)
        cabi.check(self.lib.ld_dn_head_forward(xp.data_ptr(), p.w.data_ptr(), p.b.data_ptr(), out.data_ptr(), self.B, self.H,
                                               self.W, m.dim, m.cip, m.dim_out, self.st), "dn_head_forward")
        return out, (xp,)

    def backward(self, dout, saved):
        m, p = self.mod, self.p
        (xp,) = saved
        dout = dout.contiguous()                                     # (NCHW, as the forward gave it: a copy only otherwise)
        dw, db = self.empty(m.dim_out, m.dim, 1, 1), self.empty(m.dim_out)
        dxp = self.empty(self.B, self.H, self.W, m.cip)
        work = self.work(self.lib.ld_dn_head_work_bytes(self.B, self.H, self.W, m.dim, m.dim_out))
        cabi.check(self.lib.ld_dn_head_backward(dout.data_ptr(), xp.data_ptr(), p.w.data_ptr(), work.data_ptr(), dw.data_ptr(),
                                                db.data_ptr(), dxp.data_ptr(), self.B, self.H, self.W, m.dim, m.cip, m.dim_out,
                                                self.st), "dn_head_backward")
        return dxp[..., :m.dim].permute(0, 3, 1, 2), (), {"weight": dw, "bias": db}


_USES = ("Conv2d: only the denoiser's three uses are built: kernel_size 3 with padding 1 and both channel counts multiples of "
         "32 (downs.-1.3, ups.-1.3); kernel_size 7 with padding 3, in_channels 1..4 and out_channels a multiple of 32 "
         "(init_conv); kernel_size 1 with padding 0, in_channels a multiple of 32 and out_channels 1..8 (final_conv)")


class Conv2d(TrainableModule):
    """``nn.Conv2d(in_channels, out_channels, kernel_size, padding=padding)`` in the three uses the denoiser makes of it,
    forward and backward in HIP (fp32), the parameters ``weight`` and ``bias``:

    * ``Conv2d(c, c', 3, padding=1)``, c and c' multiples of 32 (``downs.-1.3``, ``ups.-1.3``);
    * ``Conv2d(channels, init_dim, 7, padding=3)``, channels 1..4, init_dim a multiple of 32 (``init_conv``).  Its input is
      data: **the stem has no input gradient**.  An ``x`` that requires grad raises ``ValueError``; x may have any strides;
    * ``Conv2d(dim, out_dim, 1)``, dim a multiple of 32, out_dim 1..8 (``final_conv``): the result is NCHW and contiguous.

    Anything else raises ``ValueError``.  ``forward(x)``: ``x`` [B, in_channels, H, W] fp32 on the GPU, any H, W >= 1; for the
    first and the last use a ``channels_last`` x with ``in_channels`` a multiple of 64 is read in place, and the first two
    return a ``channels_last``-strided view of the kernels' NHWC output."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0):
        super().__init__()
        ci, co, k = in_channels, out_channels, kernel_size
        ints = all(isinstance(v, int) and not isinstance(v, bool) for v in (ci, co, k, padding))
        if ints and (k, padding) == (3, 1) and ci > 0 and co > 0 and ci % 32 == 0 and co % 32 == 0:
            self.use, self.Run, self.cip = "conv3x3", _Conv3Run, pad64(ci)
        elif ints and (k, padding) == (7, 3) and 1 <= ci <= 4 and co > 0 and co % 32 == 0:
            self.use, self.Run, self.cip = "stem", _StemRun, pad64(49 * ci)
        elif ints and (k, padding) == (1, 0) and ci > 0 and ci % 32 == 0 and 1 <= co <= 8:
            self.use, self.Run, self.cip = "head", _HeadRun, pad64(ci)
        else:
            raise ValueError(f"{_USES}; got in_channels {ci}, out_channels {co}, kernel_size {k}, padding {padding}")
        self.dim, self.dim_out, self.kernel_size, self.padding, self.cop = ci, co, k, padding, pad64(co)
        ref = nn.Conv2d(ci, co, k, padding=padding)                  # (nn.Conv2d's initialisation)
        self.weight, self.bias = ref.weight, ref.bias

    def _pack(self, dev):
        lib, st, p = cabi.lib(), stream(dev), _Packed()
        ci, co = self.dim, self.dim_out
        if self.use == "head":
            # The head kernels read the parameters' own [O][C] and [O]: these are views of them (contiguous already, so no
            # copy), always current whatever the cache key says, and there is no ``ones`` / ``zeros`` because ``_HeadRun``
            # never calls ``Run.conv``.
            p.w, p.b = self.weight.detach().contiguous(), self.bias.detach().contiguous()
            return p
        if self.use == "stem":                                       # OIHW is [co][49 ci] in memory: a 1x1 over the columns
            p.wf, p.wd = pack_conv(lib, st, self.weight, co, self.cop, 49 * ci, self.cip, 1, self.operand_precision)
        else:
            p.wf, p.wd = pack_conv(lib, st, self.weight, co, self.cop, ci, self.cip, 3, self.operand_precision)
        p.b = pack_vec(self.bias, self.cop)
        p.ones, p.zeros = ones_zeros(max(self.cip, self.cop), dev)
        return p

    def _view(self, out):
        return out if self.use == "head" else super()._view(out)

    def _check_extra(self, x):
        if self.use == "stem" and x.requires_grad:
            raise ValueError("Conv2d: the stem (kernel_size 7) has no input gradient, its input is data; x must not require grad")
