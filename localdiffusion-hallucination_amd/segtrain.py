"""Training the segmentation U-Net on the GPU: one optimisation step of the reference's ``train_seg.py:78-95`` over
``SegUNet`` (fp32, NHWC, the kernels of ``csrc/segtrain.hip``), and the evaluation half of its epoch (``:101-121``).

    model.train(); prediction = model(input)
    loss = BCEWithLogitsLoss(pos_weight=10)(prediction, target) + DiceLoss(eps=1e-5)(sigmoid(prediction), target)
    loss.backward(); Adam(lr=1e-3).step()

The training-mode forward and every data gradient are ``ld_pc_conv`` launches (exact-f32 MFMA implicit GEMM), the weight
gradients ``ld_seg_wgrad``; BatchNorm uses batch statistics and updates the running ones; the pooled tensors and the
concatenations are materialised because they are saved activations.  Nothing inside a step synchronises with the host:
the loss comes back as a device scalar.  The kernels work on the module's own ``nn.Parameter`` / buffer storage, so
``state_dict()`` holds the trained values after every step.

inc's first convolution (Cin 1 or 3) runs through the same kernels on an image padded to 64 channels with zeros (its
weight gradient is read from the first Cin input channels of the padded one).

Not covered: 16-bit storage while training, ``bilinear=True``, more than one class, multi-GPU training.
"""
import csv
import ctypes as C
import os

import torch

from . import _cabi as cabi
from .dataset import epoch_batches
from .segnet import BN_EPS, SegUNet
from .strided_adam import StridedAdam
from .weights import SEG_WIDTHS

BN_MOMENTUM = 0.1
PAD_CIN = 64                      # inc's first convolution: the image padded to the kernels' channel granule
RED_WORK_BYTES = 2048 * 2 * 64 * 8    # LD_SEG_RED_WORK_BYTES


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _Conv:
    """One 3x3 convolution + BatchNorm of a DoubleConv: the parameters, their kernel layouts and gradient buffers."""

    def __init__(self, conv, bn, dev, first):
        self.conv, self.bn = conv, bn
        self.cout, self.cin = conv.weight.shape[0], conv.weight.shape[1]
        self.cin_k = PAD_CIN if first else self.cin          # channels the kernels see
        f32 = dict(dtype=torch.float32, device=dev)
        self.wf = torch.zeros(self.cout * 9 * self.cin_k, **f32)              # [co][ky][kx][ci] (OHWI)
        self.wb = None if first else torch.empty(self.cin * 9 * self.cout, **f32)   # [ci][2-ky][2-kx][co]
        self.gw = torch.empty(self.cout * 9 * self.cin_k, **f32)              # like wf
        self.ggamma, self.gbeta = torch.empty(self.cout, **f32), torch.empty(self.cout, **f32)
        # the weight seen as [cout][cin][9] in each kernel layout: (buffer, offset, s0, s1, s2); gw has wf's strides.  inc's
        # first convolution has no wb, and nothing writes lanes cin..63 of its wf: they stay zero
        self.mirrors = ((self.wf, 0, 9 * self.cin_k, 1, self.cin_k),)
        if self.wb is not None:
            self.mirrors += ((self.wb, 8 * self.cout, 1, 9 * self.cout, -self.cout),)


class _TrainState:
    """Per-module training state: kernel-layout weights (packed here, then kept current by the optimiser's mirrors),
    gradient buffers and the per-(B, H, W) plans with the saved activations."""

    def __init__(self, net, dev):
        for p in list(net.parameters()) + list(net.buffers()):
            if p.device != dev or (p.dtype != torch.float32 and p.is_floating_point()) or not p.is_contiguous():
                raise ValueError("SegUNet training: parameters and buffers must be contiguous fp32 tensors on the input's "
                                 "device (call .to(device) first)")
        self.net, self.dev = net, dev
        f32 = dict(dtype=torch.float32, device=dev)
        self.convs = []                     # 18 _Conv in launch order
        for i, dc in enumerate(net._double_convs()):
            c1, bn1, _, c2, bn2, _ = dc.double_conv
            self.convs.append((_Conv(c1, bn1, dev, first=(i == 0)), _Conv(c2, bn2, dev, first=False)))
        self.ups = []
        for u in (net.up1, net.up2, net.up3, net.up4):
            cin, cout = u.up.weight.shape[0], u.up.weight.shape[1]
            wf = torch.empty(4 * cout * cin, **f32)                           # [(p1, p2, c)][ci]: the GEMM's OHWI weight
            wb = torch.empty(cin * 4 * cout, **f32)                           # [ci][(p1, p2, c)]: the data gradient's
            self.ups.append({"m": u.up, "cin": cin, "cout": cout, "wf": wf, "wb": wb,
                             # the weight seen as [cin][cout][4] in each layout, as _Conv.mirrors; gw has wf's strides
                             "mirrors": ((wf, 0, 1, cin, cout * cin), (wb, 0, 4 * cout, 1, cout)),
                             "bias4": torch.empty(4 * cout, **f32),
                             "gw": torch.empty(4 * cout * cin, **f32), "gb": torch.empty(cout, **f32)})
        self.ghw, self.ghb = torch.empty(SEG_WIDTHS[0], **f32), torch.empty(1, **f32)
        self.ones, self.zeros = torch.ones(4 * SEG_WIDTHS[4], **f32), torch.zeros(4 * SEG_WIDTHS[4], **f32)
        self.red_work = torch.empty(RED_WORK_BYTES // 8, dtype=torch.float64, device=dev)
        self.loss_out = torch.empty(3, **f32)
        self.wg_work = None
        self.plans = {}
        self.pack()

    # ------------------------------------------------------------------ weights in kernel layout
    def pack(self):
        """Every kernel-layout copy from the parameters' own layout (construction; the optimiser step keeps them current)."""
        lib, st = cabi.lib(), _st(self.dev)
        for _, prm, _, dims, _, mirrors in self.named_grads():
            for buf, off, s0, s1, s2 in mirrors:
                cabi.check(lib.ld_seg_permute3(prm.data_ptr(), buf.data_ptr(), *dims, off, s0, s1, s2, st), "seg_permute3")
        self.pack_bias4()

    def pack_bias4(self):
        """The transposed convolutions' bias repeated for the four (p1, p2): one source element in four places, so no mirror."""
        for u in self.ups:
            u["bias4"].view(4, u["cout"]).copy_(u["m"].bias.detach().view(1, u["cout"]).expand(4, u["cout"]))

    # ------------------------------------------------------------------ buffers per input shape
    def plan(self, B, H, W):
        key = (B, H, W)
        p = self.plans.get(key)
        if p is not None:
            return p
        dev, w = self.dev, SEG_WIDTHS
        lib = cabi.lib()

        def buf(h, wd, c):
            return torch.empty((B, h, wd, c), dtype=torch.float32, device=dev)

        blocks = []
        need = 0
        for i in range(9):
            lvl = i if i < 5 else 8 - i
            h, wd = H >> lvl, W >> lvl
            c1, c2 = self.convs[i]
            cin = c1.cin_k
            blk = {"h": h, "w": wd, "cin": cin, "cout": c1.cout,
                   "xin": torch.zeros((B, h, wd, cin), dtype=torch.float32, device=dev) if i == 0 else buf(h, wd, cin),
                   "y1": buf(h, wd, c1.cout), "a1": buf(h, wd, c1.cout), "y2": buf(h, wd, c1.cout), "a2": buf(h, wd, c1.cout),
                   "stat1": torch.empty(3 * c1.cout, dtype=torch.float32, device=dev),
                   "stat2": torch.empty(3 * c1.cout, dtype=torch.float32, device=dev),
                   "gout": buf(h, wd, c1.cout), "ga1": buf(h, wd, c1.cout), "gxin": buf(h, wd, cin) if i > 0 else None}
            if i < 4:
                blk["gskip"] = buf(h, wd, c1.cout)
            if i >= 5:
                u = self.ups[i - 5]
                blk["low"], blk["glow"] = buf(h // 2, wd // 2, 4 * u["cout"]), buf(h // 2, wd // 2, 4 * u["cout"])
                s = lib.ld_seg_wgrad_splits(B, h // 2, wd // 2, u["cin"], 4 * u["cout"], 1)
                blk["splits_up"] = s
                need = max(need, s * 4 * u["cout"] * u["cin"])
            blk["splits1"] = lib.ld_seg_wgrad_splits(B, h, wd, cin, c1.cout, 3)
            blk["splits2"] = lib.ld_seg_wgrad_splits(B, h, wd, c1.cout, c1.cout, 3)
            if min(blk["splits1"], blk["splits2"]) < 1:
                raise RuntimeError("ld_seg_wgrad_splits refused a level's shape")
            need = max(need, blk["splits1"] * c1.cout * 9 * cin, blk["splits2"] * c1.cout * 9 * c1.cout)
            blocks.append(blk)
        if self.wg_work is None or self.wg_work.numel() < need:
            self.wg_work = torch.empty(need, dtype=torch.float32, device=dev)
        p = {"blocks": blocks, "logits": torch.empty((B, 1, H, W), dtype=torch.float32, device=dev),
             "dz": torch.empty(B * H * W, dtype=torch.float32, device=dev)}
        self.plans[key] = p
        return p

    # ------------------------------------------------------------------ launches
    def _conv(self, src, weight, shift, out, B, h, wd, cin, cout, ksize):
        a = cabi.PcConvArgs()
        a.src, a.weight, a.scale, a.shift, a.residual, a.out = src.data_ptr(), weight.data_ptr(), self.ones.data_ptr(), \
            shift.data_ptr(), None, out.data_ptr()
        a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout, a.ksize, a.stride, a.relu = B, h, wd, cin, h, wd, cout, ksize, 1, 0
        cabi.check(cabi.lib().ld_pc_conv(C.byref(a), _st(self.dev)), "pc_conv")

    def forward(self, x, update_running):
        """x: NCHW fp32 on the device -> the plan, with every saved activation and ``logits`` [B, 1, H, W] filled."""
        B, nc, H, W = x.shape
        if B * (H // 16) * (W // 16) < 2:
            raise ValueError(f"SegUNet training: B*H*W/256 = {B * (H // 16) * (W // 16)}; BatchNorm in training mode needs "
                             "at least two values per channel at the deepest level")
        p = self.plan(B, H, W)
        lib, st, net = cabi.lib(), _st(self.dev), self.net
        blocks = p["blocks"]
        blocks[0]["xin"][..., :nc].copy_(x.permute(0, 2, 3, 1))
        for i, blk in enumerate(blocks):
            h, wd, M = blk["h"], blk["w"], B * blk["h"] * blk["w"]
            if 1 <= i <= 4:
                prev = blocks[i - 1]
                cabi.check(lib.ld_seg_pool(prev["a2"].data_ptr(), blk["xin"].data_ptr(), B, h, wd, blk["cin"], st), "seg_pool")
            elif i >= 5:
                u, prev, skip = self.ups[i - 5], blocks[i - 1], blocks[8 - i]
                self._conv(prev["a2"], u["wf"], u["bias4"], blk["low"], B, h // 2, wd // 2, u["cin"], 4 * u["cout"], 1)
                cabi.check(lib.ld_seg_cat_d2s(skip["a2"].data_ptr(), blk["low"].data_ptr(), blk["xin"].data_ptr(), B, h, wd,
                                              skip["cout"], u["cout"], st), "seg_cat_d2s")
            src, cin = blk["xin"], blk["cin"]
            for cv, yk, ak, sk in zip(self.convs[i], ("y1", "y2"), ("a1", "a2"), ("stat1", "stat2")):
                self._conv(src, cv.wf, self.zeros, blk[yk], B, h, wd, cin, cv.cout, 3)
                bn = cv.bn
                rm = bn.running_mean.data_ptr() if update_running else None
                rv = bn.running_var.data_ptr() if update_running else None
                cabi.check(lib.ld_seg_bn_train(blk[yk].data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(),
                                               self.red_work.data_ptr(), blk[sk].data_ptr(), rm, rv, BN_MOMENTUM, BN_EPS,
                                               blk[ak].data_ptr(), M, cv.cout, st), "seg_bn_train")
                if update_running:
                    bn.num_batches_tracked.add_(1)
                src, cin = blk[ak], cv.cout
        hw, hb = net.outc.conv.weight, net.outc.conv.bias
        cabi.check(lib.ld_seg_head(blocks[8]["a2"].data_ptr(), hw.data_ptr(), hb.data_ptr(), p["logits"].data_ptr(), None, None,
                                   B, H, W, SEG_WIDTHS[0], cabi.LD_F32, st), "seg_head")
        return p

    def loss(self, logits, target, dz, pos_weight, dice_eps):
        cabi.check(cabi.lib().ld_seg_loss(logits.data_ptr(), target.data_ptr(), self.red_work.data_ptr(),
                                          self.loss_out.data_ptr(), cabi.ptr(dz), logits.numel(), pos_weight, dice_eps,
                                          _st(self.dev)), "seg_loss")

    def backward(self, p, B):
        """From p['dz'] to every gradient buffer (the kernels' layouts)."""
        lib, st, net = cabi.lib(), _st(self.dev), self.net
        blocks = p["blocks"]
        work, red = self.wg_work.data_ptr(), self.red_work.data_ptr()
        last = blocks[8]
        cabi.check(lib.ld_seg_head_backward(p["dz"].data_ptr(), last["a2"].data_ptr(), net.outc.conv.weight.data_ptr(), red,
                                            self.ghw.data_ptr(), self.ghb.data_ptr(), last["gout"].data_ptr(),
                                            B * last["h"] * last["w"], SEG_WIDTHS[0], st), "seg_head_backward")
        for i in range(8, -1, -1):
            blk = blocks[i]
            h, wd, M = blk["h"], blk["w"], B * blk["h"] * blk["w"]
            c1, c2 = self.convs[i]
            for cv, g, yk, ak, sk, src, cin, spl in ((c2, blk["gout"], "y2", "a2", "stat2", blk["a1"], c2.cin_k, blk["splits2"]),
                                                     (c1, blk["ga1"], "y1", "a1", "stat1", blk["xin"], c1.cin_k, blk["splits1"])):
                cabi.check(lib.ld_seg_bn_backward(g.data_ptr(), blk[ak].data_ptr(), blk[yk].data_ptr(), cv.bn.weight.data_ptr(),
                                                  blk[sk].data_ptr(), red, cv.ggamma.data_ptr(), cv.gbeta.data_ptr(),
                                                  g.data_ptr(), M, cv.cout, st), "seg_bn_backward")
                cabi.check(lib.ld_seg_wgrad(g.data_ptr(), src.data_ptr(), work, cv.gw.data_ptr(), B, h, wd, cin, cv.cout, 3, spl,
                                            st), "seg_wgrad")
                if cv.wb is not None:                                      # data gradient: the flipped, transposed weight
                    self._conv(g, cv.wb, self.zeros, blk["ga1"] if cv is c2 else blk["gxin"], B, h, wd, cv.cout, cv.cin, 3)
            if i >= 5:
                u, prev, skip = self.ups[i - 5], blocks[i - 1], blocks[8 - i]
                cabi.check(lib.ld_seg_cat_d2s_backward(blk["gxin"].data_ptr(), skip["gskip"].data_ptr(), blk["glow"].data_ptr(),
                                                       B, h, wd, skip["cout"], u["cout"], st), "seg_cat_d2s_backward")
                Ml = B * (h // 2) * (wd // 2)
                cabi.check(lib.ld_seg_colsum(blk["glow"].data_ptr(), red, u["gb"].data_ptr(), Ml, 4 * u["cout"], 4, st),
                           "seg_colsum")
                cabi.check(lib.ld_seg_wgrad(blk["glow"].data_ptr(), prev["a2"].data_ptr(), work, u["gw"].data_ptr(), B, h // 2,
                                            wd // 2, u["cin"], 4 * u["cout"], 1, blk["splits_up"], st), "seg_wgrad")
                self._conv(blk["glow"], u["wb"], self.zeros, prev["gout"], B, h // 2, wd // 2, 4 * u["cout"], u["cin"], 1)
            elif i >= 1:
                prev = blocks[i - 1]
                cabi.check(lib.ld_seg_pool_backward(prev["a2"].data_ptr(), blk["gxin"].data_ptr(), prev["gskip"].data_ptr(),
                                                    prev["gout"].data_ptr(), B, h, wd, blk["cin"], st), "seg_pool_backward")

    def named_grads(self):
        """(parameter name, parameter, gradient buffer, (d0, d1, d2), gradient strides, mirrors) in ``named_parameters()``
        order: what ``StridedAdam.step`` takes."""
        by_param = {}

        def flat(prm, g):
            by_param[id(prm)] = (g, (1, 1, prm.numel()), (0, 0, 1), ())
        for pair in self.convs:
            for cv in pair:
                by_param[id(cv.conv.weight)] = (cv.gw, (cv.cout, cv.cin, 9), cv.mirrors[0][2:], cv.mirrors)
                flat(cv.bn.weight, cv.ggamma)
                flat(cv.bn.bias, cv.gbeta)
        for u in self.ups:
            by_param[id(u["m"].weight)] = (u["gw"], (u["cin"], u["cout"], 4), u["mirrors"][0][2:], u["mirrors"])
            flat(u["m"].bias, u["gb"])
        flat(self.net.outc.conv.weight, self.ghw)
        flat(self.net.outc.conv.bias, self.ghb)
        return [(n, prm) + by_param[id(prm)] for n, prm in self.net.named_parameters()]

    def grads_own_layout(self):
        out = {}
        for name, prm, g, dims, strides, _ in self.named_grads():
            out[name] = torch.as_strided(g, dims, strides).reshape(prm.shape).clone()
        return out


def train_state(net, dev):
    st = getattr(net, "_train", None)
    if st is None or st.dev != dev:
        st = _TrainState(net, dev)
        net._train = st
    return st


def check_train_input(net, x):
    if net.compute_dtype != "fp32":
        raise ValueError(f"SegUNet training runs in fp32 only (compute_dtype {net.compute_dtype!r}); 16-bit storage while "
                         "training is not covered")
    if x.dim() != 4 or x.shape[1] != net.n_channels:
        raise ValueError(f"SegUNet: input {tuple(x.shape)}, expected [B, {net.n_channels}, H, W]")
    B, _, H, W = x.shape
    if B < 1 or H < 16 or W < 16 or H % 16 or W % 16:
        raise ValueError(f"SegUNet: H, W = {H}, {W} must be positive multiples of 16")
    if not torch.cuda.is_available() or not x.is_cuda:
        raise RuntimeError("SegUNet in train() mode runs on the GPU only (HIP kernels; there is no CPU fallback): move the "
                           "module and the input to the device.  For inference call .eval() first (test.py:221 does)")
    return x.detach().to(torch.float32).contiguous()


def train_forward(net, x):
    """``SegUNet.forward`` in ``train()`` mode: batch statistics, running statistics updated, logits NCHW fp32."""
    x = check_train_input(net, x)
    st = train_state(net, x.device)
    p = st.forward(x, update_running=True)
    net._prep, net._plans = None, {}             # the eval-mode cache holds the old running statistics
    return p["logits"].clone()


class SegTrainer:
    """``train_seg.py``'s optimisation loop over a ``SegUNet`` on the GPU (fp32)."""

    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, pos_weight=10.0, dice_eps=1e-5):
        if not isinstance(net, SegUNet):
            raise TypeError("SegTrainer trains a SegUNet")
        if net.compute_dtype != "fp32":
            raise ValueError(f"SegTrainer runs in fp32 only (compute_dtype {net.compute_dtype!r}); 16-bit storage while "
                             "training is not covered")
        self.net, self.adam = net, StridedAdam(lr, betas, eps)
        self.pos_weight, self.dice_eps = float(pos_weight), float(dice_eps)

    @property
    def t(self):                  # optimisation steps taken
        return self.adam.t

    def _target(self, x, target):
        if tuple(target.shape) != (x.shape[0], 1, x.shape[2], x.shape[3]):
            raise ValueError(f"SegTrainer: target {tuple(target.shape)} for input {tuple(x.shape)}")
        return target.detach().to(x.device, torch.float32).contiguous()

    def _forward_backward(self, x, target, update_running):
        x = check_train_input(self.net, x)
        target = self._target(x, target)
        st = train_state(self.net, x.device)
        p = st.forward(x, update_running)
        st.loss(p["logits"], target, p["dz"], self.pos_weight, self.dice_eps)
        st.backward(p, x.shape[0])
        return st

    def loss_and_grads(self, x, target):
        """-> (loss, {name: gradient in the parameter's own shape}) at the current weights; changes neither the
        parameters nor the running statistics."""
        st = self._forward_backward(x, target, update_running=False)
        return st.loss_out[0].clone(), st.grads_own_layout()

    def step(self, x, target):
        """One optimisation step -> the loss (before the step) as a device scalar; no host synchronisation."""
        st = self._forward_backward(x, target, update_running=True)
        loss = st.loss_out[0].clone()
        self.adam.step(st.named_grads(), st.dev)             # its mirrors keep wf / wb current: no repack
        st.pack_bias4()
        self.net._prep, self.net._plans = None, {}          # eval-mode cache: repack on next use
        return loss

    def evaluate(self, x, target):
        """train_seg.py:104-115 on one batch: eval-mode forward -> (dice, bce) = (1 - DiceLoss, BCEWithLogitsLoss)."""
        net = self.net
        was = net.training
        net.eval()
        try:
            logits = net(x)
        finally:
            net.train(was)
        target = self._target(logits, target)
        st = train_state(net, logits.device)
        st.loss(logits, target, None, self.pos_weight, self.dice_eps)
        out = st.loss_out.cpu()
        return 1.0 - float(out[2]), float(out[1])

    def fit(self, train_batches, val_batches, epochs, out_path, log=None):
        """The epochs of train_seg.py:78-121: ``train_batches`` / ``val_batches`` are sequences of (input, target), or
        ``train_batches`` is a callable epoch -> such a sequence (a new batch composition per epoch, as the reference's
        ``DataLoader(shuffle=True)`` gives); ``out_path`` receives ``torch.save(model.state_dict())`` whenever the mean validation dice improves (the file
        ``checkpoint.load_seg_checkpoint`` and test.py:219 read).  With ``log`` (a directory) train.csv / val.csv are
        rewritten every epoch.  -> {'best_dice', 'best_epoch', 'train', 'val'}.

        Either may be a ``dataset.BatchSource`` over a ``DeviceDataset.seg``.  As ``train_batches`` it is asked for
        ``batches(epoch)`` -- the epoch's shuffle and augmentation -- and walked lazily: batch k + 1 is made after batch k's step
        was enqueued, and nothing new synchronises inside an epoch.  As ``val_batches`` it is walked as ``batches(0)`` at every
        epoch, so every epoch validates on the same batches.  ``fit`` over sources is bit-identical to
        ``fit(lambda e: list(source.batches(e)), list(val.batches(0)), ...)``."""
        best, best_epoch, train_rows, val_rows = 0.0, None, [], []
        for e in range(int(epochs)):
            self.net.train()
            losses = [self.step(x, t) for x, t in epoch_batches(train_batches, e)]
            train_rows.append((e, float(torch.stack(losses).mean()) if losses else float("nan")))
            scores = [self.evaluate(x, t) for x, t in epoch_batches(val_batches)]
            dice = sum(s[0] for s in scores) / max(1, len(scores))
            bce = sum(s[1] for s in scores) / max(1, len(scores))
            val_rows.append((e, dice, bce))
            if log is not None:
                for name, head, rows in (("train.csv", ("epoch", "loss"), train_rows), ("val.csv", ("epoch", "dice", "bce"), val_rows)):
                    with open(os.path.join(log, name), "w", newline="") as f:
                        csv.writer(f).writerows([head] + rows)
            if dice > best:
                best, best_epoch = dice, e
                torch.save({k: v.detach().cpu() for k, v in self.net.state_dict().items()}, out_path)
        return {"best_dice": best, "best_epoch": best_epoch, "train": train_rows, "val": val_rows}
