"""Segmentation U-Net of the reference (``unet_model.UNet``, /root/reference/unet_model.py:140-243) on the HIP kernels of
``csrc/segnet.hip``: the OOD-mask producer that the reference's MRI evaluation runs on the conditioning image before
``sample(..., mask=...)`` (test.py:214-221, 284-289, ``ood_detector.seg: True``).

``SegUNet`` keeps the reference's module tree, so ``state_dict()`` has its 118 names, shapes and dtypes (BatchNorm running
statistics and ``num_batches_tracked`` included) and ``test.py``'s ``seg_model.load_state_dict(torch.load(path))`` works
unchanged.  The forward is 23 launches: per DoubleConv two 3x3 convolutions with BatchNorm (eval) + ReLU as an fp32
epilogue, Down's max-pool read by the next convolution, each Up's ConvTranspose2d(2, 2) as a 1x1 GEMM whose output the
next convolution reads through depth-to-space beside the skip tensor, and the 1x1 head.  In ``eval()`` mode, as
test.py:221 puts it, BatchNorm uses the running statistics.  In ``train()`` mode ``forward`` uses batch statistics and
updates the running ones, as the reference module does (fp32 only, the kernels of ``csrc/segtrain.hip``); the optimisation
step of train_seg.py is ``segtrain.SegTrainer``.  No CPU fallback.

Not covered: ``bilinear=True``, sizes that are not multiples of 16 (the reference's F.pad path, :193-199), more than
one class, 16-bit storage while training.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _cabi as cabi
from .weights import SEG_WIDTHS

_TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
BN_EPS = 1e-5


class _DoubleConv(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.double_conv = nn.Sequential(
            nn.Conv2d(cin, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True),
            nn.Conv2d(cout, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))


class _Down(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.maxpool_conv = nn.Sequential(nn.MaxPool2d(2), _DoubleConv(cin, cout))


class _Up(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.up = nn.ConvTranspose2d(cin, cin // 2, kernel_size=2, stride=2)
        self.conv = _DoubleConv(cin, cout)


class _OutConv(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size=1)


def _bn_affine(bn):
    """BatchNorm2d (eval) as out = x * s + t, in fp32 from the running statistics."""
    s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    t = bn.bias.detach().float() - bn.running_mean.detach().float() * s
    return s.contiguous(), t.contiguous()


class SegUNet(nn.Module):
    def __init__(self, n_channels=1, n_classes=1, bilinear=False, compute_dtype="fp32"):
        super().__init__()
        if bilinear:
            raise ValueError("SegUNet: bilinear=True (nn.Upsample + DoubleConv(in, out, in // 2)) has no HIP kernels; "
                             "only the ConvTranspose2d form (bilinear=False) that test.py / train_seg.py build is supported")
        if n_channels not in (1, 3):
            raise ValueError(f"SegUNet: n_channels={n_channels}; the first convolution takes 1 or 3 input channels")
        if n_classes != 1:
            raise ValueError(f"SegUNet: n_classes={n_classes}; the head kernel writes one class (the OOD mask)")
        self.n_channels, self.n_classes, self.bilinear = n_channels, n_classes, bilinear
        w = SEG_WIDTHS
        self.inc = _DoubleConv(n_channels, w[0])
        self.down1, self.down2, self.down3, self.down4 = (_Down(w[i], w[i + 1]) for i in range(4))
        self.up1, self.up2, self.up3, self.up4 = (_Up(w[4 - i], w[3 - i]) for i in range(4))
        self.outc = _OutConv(w[0], n_classes)
        self.compute_dtype = compute_dtype if compute_dtype in _TDT else None
        if self.compute_dtype is None:
            raise ValueError(f"SegUNet: compute_dtype {compute_dtype!r} (fp32, bf16 or fp16)")
        self._prep = None            # device-side packed weights + BN affines (per device / weights)
        self._plans = {}             # (B, H, W, dtype) -> launch list with its activation buffers
        self._train = None           # segtrain._TrainState: training-layout weights, gradients, saved activations

    # ------------------------------------------------------------------ cache control
    def invalidate(self):
        self._prep = None
        self._plans = {}
        self._train = None

    def set_compute_dtype(self, dtype):
        if dtype not in _TDT:
            raise ValueError(f"SegUNet: compute_dtype {dtype!r} (fp32, bf16 or fp16)")
        if dtype != self.compute_dtype:
            self.compute_dtype = dtype
            self._plans = {}

    def _apply(self, fn, *args, **kwargs):
        self.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        self.invalidate()
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    # ------------------------------------------------------------------ weights in kernel layout
    def _double_convs(self):
        """The nine DoubleConvs in launch order: inc, down1..4, up1..4."""
        return [self.inc] + [d.maxpool_conv[1] for d in (self.down1, self.down2, self.down3, self.down4)] + \
               [u.conv for u in (self.up1, self.up2, self.up3, self.up4)]

    def _prepare(self, dev):
        if self._prep is not None:
            return self._prep
        lib = cabi.lib()
        st = torch.cuda.current_stream(dev).cuda_stream
        prep = {"dc": [], "up": []}
        with torch.no_grad():
            for i, dc in enumerate(self._double_convs()):
                c1, bn1, _, c2, bn2, _ = dc.double_conv
                layers = []
                for conv, bn in ((c1, bn1), (c2, bn2)):
                    w = conv.weight.detach().to(dev, torch.float32).contiguous()
                    s, t = _bn_affine(bn)
                    if i == 0 and conv is c1:         # inc's first convolution reads the OIHW weight directly
                        packed = w
                    else:
                        packed = torch.empty(w.numel(), dtype=torch.float32, device=dev)
                        cabi.check(lib.ld_seg_pack_weight(w.data_ptr(), packed.data_ptr(), w.shape[0], w.shape[1], 3, st),
                                   "seg_pack_weight")
                    layers.append((packed, s.to(dev), t.to(dev), w.shape[0], w.shape[1]))
                prep["dc"].append(layers)
            for u in (self.up1, self.up2, self.up3, self.up4):
                w = u.up.weight.detach().to(dev, torch.float32).contiguous()
                b = u.up.bias.detach().to(dev, torch.float32).contiguous()
                cin, cout = w.shape[0], w.shape[1]
                wp = torch.empty(cin * 4 * cout, dtype=torch.float32, device=dev)
                bp = torch.empty(4 * cout, dtype=torch.float32, device=dev)
                cabi.check(lib.ld_seg_pack_convt(w.data_ptr(), b.data_ptr(), wp.data_ptr(), bp.data_ptr(), cin, cout, st),
                           "seg_pack_convt")
                prep["up"].append((wp, bp, cin, cout))
            prep["head"] = (self.outc.conv.weight.detach().to(dev, torch.float32).reshape(-1).contiguous(),
                            self.outc.conv.bias.detach().to(dev, torch.float32).contiguous())
        self._prep = prep
        return prep

    # ------------------------------------------------------------------ launch list
    def _plan(self, B, H, W, dev):
        key = (B, H, W, self.compute_dtype, str(dev))
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        prep = self._prepare(dev)
        tdt, code = _TDT[self.compute_dtype], cabi.dtype_code(self.compute_dtype)
        lib = cabi.lib()
        w = SEG_WIDTHS
        bufs = []

        def act(h, wd, c):
            t = torch.empty((B, h, wd, c), dtype=tdt, device=dev)
            bufs.append(t)
            return t

        launches = []          # (function, args struct or tuple) -- the input image / outputs are bound per call

        def conv(src0, c0, mode, layer, out, h, wd, src1=None, c1=0, ksize=3, scale=True, relu=1):
            packed, s, t, cout, _ = layer
            a = cabi.SegConvArgs()
            a.src0, a.src1, a.C0, a.C1, a.mode, a.ksize = src0.data_ptr(), cabi.ptr(src1), c0, c1, mode, ksize
            a.weight, a.scale, a.shift, a.relu = packed.data_ptr(), s.data_ptr() if scale else None, t.data_ptr(), relu
            a.out, a.B, a.H, a.W, a.Cout, a.dtype = out.data_ptr(), B, h, wd, out.shape[-1], code
            launches.append((lib.ld_seg_conv, a, "seg_conv"))

        skips = []
        h, wd = H, W
        x1a = act(h, wd, w[0])                             # inc.conv1 comes from the image (bound per call)
        x = act(h, wd, w[0])
        conv(x1a, w[0], cabi.SEG_SRC_PLAIN, prep["dc"][0][1], x, h, wd)
        skips.append(x)
        for lvl in range(1, 5):                            # down1..down4: pool on load, DoubleConv
            h, wd = h // 2, wd // 2
            mid = act(h, wd, w[lvl])
            conv(x, w[lvl - 1], cabi.SEG_SRC_POOL, prep["dc"][lvl][0], mid, h, wd)
            x = act(h, wd, w[lvl])
            conv(mid, w[lvl], cabi.SEG_SRC_PLAIN, prep["dc"][lvl][1], x, h, wd)
            skips.append(x)
        for i in range(4):                                 # up1..up4: convT as a GEMM, cat + depth-to-space, DoubleConv
            wp, bp, cin, cout = prep["up"][i]
            low = act(h, wd, 4 * cout)
            conv(x, cin, cabi.SEG_SRC_PLAIN, (wp, None, bp, 4 * cout, cin), low, h, wd, ksize=1, scale=False, relu=0)
            h, wd = h * 2, wd * 2
            skip = skips[3 - i]
            mid = act(h, wd, cout)
            conv(skip, skip.shape[-1], cabi.SEG_SRC_CAT_D2S, prep["dc"][5 + i][0], mid, h, wd, src1=low, c1=cout)
            x = act(h, wd, cout)
            conv(mid, cout, cabi.SEG_SRC_PLAIN, prep["dc"][5 + i][1], x, h, wd)
        plan = {"launches": launches, "bufs": bufs, "x1a": x1a, "last": x}
        self._plans[key] = plan
        return plan

    def _check_input(self, x):
        if self.training:
            raise RuntimeError("SegUNet.predict_mask runs BatchNorm with its running statistics: call .eval() first "
                               "(test.py:221 does); in train() mode use forward() or segtrain.SegTrainer")
        if x.dim() != 4 or x.shape[1] != self.n_channels:
            raise ValueError(f"SegUNet: input {tuple(x.shape)}, expected [B, {self.n_channels}, H, W]")
        B, _, H, W = x.shape
        if B < 1 or H < 16 or W < 16 or H % 16 or W % 16:
            raise ValueError(f"SegUNet: H, W = {H}, {W} must be positive multiples of 16 (four 2x2 pools without the "
                             "reference's F.pad path, unet_model.py:193-199, which is not covered)")
        if not torch.cuda.is_available():
            raise RuntimeError("SegUNet needs a GPU (HIP kernels only; there is no CPU fallback)")
        if not x.is_cuda:
            raise ValueError("SegUNet: the input must be a CUDA tensor on the module's device")
        return x.detach().to(torch.float32).contiguous()

    def _run(self, x, logits=None, prob=None, mask=None):
        B, _, H, W = x.shape
        dev = x.device
        plan = self._plan(B, H, W, dev)
        prep = self._prep
        lib = cabi.lib()
        st = torch.cuda.current_stream(dev).cuda_stream
        code = cabi.dtype_code(self.compute_dtype)
        w0, s0, t0, _, _ = prep["dc"][0][0]
        cabi.check(lib.ld_seg_conv_image(x.data_ptr(), w0.data_ptr(), s0.data_ptr(), t0.data_ptr(), plan["x1a"].data_ptr(),
                                         B, self.n_channels, H, W, code, st), "seg_conv_image")
        for fn, a, what in plan["launches"]:
            cabi.check(fn(C.byref(a), st), what)
        hw, hb = prep["head"]
        cabi.check(lib.ld_seg_head(plan["last"].data_ptr(), hw.data_ptr(), hb.data_ptr(), cabi.ptr(logits), cabi.ptr(prob),
                                   cabi.ptr(mask), B, H, W, SEG_WIDTHS[0], code, st), "seg_head")

    def forward(self, x):
        """x: NCHW fp32 [B, n_channels, H, W] on the GPU -> logits NCHW fp32 [B, 1, H, W] (unet_model.py:232-243).  In
        ``train()`` mode: batch statistics, and the running ones are updated (fp32 only)."""
        if self.training:
            from . import segtrain
            return segtrain.train_forward(self, x)
        x = self._check_input(x)
        logits = torch.empty((x.shape[0], 1, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
        self._run(x, logits=logits)
        return logits

    def predict_mask(self, x, return_logits=False):
        """-> (prob, binary): sigmoid(logits) and (prob > 0.5) as 0 / 1, NCHW fp32 (test.py:286-288), from the fused head;
        with ``return_logits`` also the logits."""
        x = self._check_input(x)
        shape = (x.shape[0], 1, x.shape[2], x.shape[3])
        prob = torch.empty(shape, dtype=torch.float32, device=x.device)
        binary = torch.empty(shape, dtype=torch.float32, device=x.device)
        logits = torch.empty(shape, dtype=torch.float32, device=x.device) if return_logits else None
        self._run(x, logits=logits, prob=prob, mask=binary)
        return (prob, binary, logits) if return_logits else (prob, binary)
