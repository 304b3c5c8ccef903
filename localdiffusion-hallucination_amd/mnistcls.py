"""The MNIST digit classifier of the reference's MNIST experiment and its training, on the GPU.

``MnistClassifier`` is ``SimpleCNN`` (train_mnist_cls.py:31-47, also models.py:24-40) with the reference's parameter names
and shapes, so a ``state_dict`` saved by train_mnist_cls.py:116 loads with ``strict=True`` and ours loads into the
reference's class:

    conv1 (1 -> 32, 3x3, pad 1) + ReLU + MaxPool2d(2); conv2 (32 -> 64) + ReLU + MaxPool2d(2);
    x.view(-1, 64 * 7 * 7); fc1 (3136 -> 128) + ReLU; fc2 (128 -> 10)

``MnistClassifierTrainer`` is the optimisation loop of train_mnist_cls.py:79-119: ``nn.CrossEntropyLoss()`` (the mean of
log-softmax + NLL), the whole backward pass and ``torch.optim.Adam(lr=1e-3)`` with its defaults.

Everything runs in fp32 through the kernels of ``csrc/mnistcls.hip`` (plus ``ld_pc_conv`` / ``ld_seg_wgrad`` for conv2 and
its gradients).  Activations are NHWC, so fc1 reads the features in (y, x, c) order: its weight is repacked once on the
device from the reference's ``c * 49 + y * 7 + x`` order, its gradient is read back through the same strides, and the
optimiser's launch keeps the packed copies current.  There is no autograd graph and no CPU fallback; nothing inside
``forward`` / ``predict`` / ``step`` synchronises with the host.

Not covered: the commented-out VGG16 variant, augmentations, 16-bit storage, more than one GPU.
"""
import csv
import ctypes as C

import torch
from torch import nn

from . import _cabi as cabi
from .dataset import epoch_batches
from .segtrain import RED_WORK_BYTES
from .strided_adam import StridedAdam

N_CLASSES, HIDDEN, FEATURES = 10, 128, 64 * 7 * 7
CS = 64                               # channel stride of pool1's output: conv1's 32 channels, the upper 32 zero
_GPU_ONLY = ("MnistClassifier runs on the GPU only (HIP kernels; there is no CPU fallback): move the module and the input "
             "to the device")


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _Packed:
    """Device-side state of one module on one device: the kernel-layout weights and the per-batch-size buffers."""

    def __init__(self, net, dev):
        for p in net.parameters():
            if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("MnistClassifier: parameters must be contiguous fp32 tensors on the input's device (call "
                                 ".to(device) first)")
        self.net, self.dev = net, dev
        f32 = dict(dtype=torch.float32, device=dev)
        self.w2f = torch.zeros(64 * 9 * CS, **f32)            # conv2 [co][ky][kx][ci of 64]: ld_pc_conv's OHWI
        self.w2b = torch.zeros(CS * 9 * 64, **f32)            # conv2's data gradient [ci of 64][2-ky][2-kx][co]
        self.wfc1 = torch.empty(HIDDEN * FEATURES, **f32)     # fc1 [n][(y, x, c)]
        self.ones, self.zeros = torch.ones(64, **f32), torch.zeros(64, **f32)
        self.bad_label = torch.zeros(1, dtype=torch.int32, device=dev)
        self.plans = {}
        self.pack()

    # mirrors of a parameter seen as [d0][d1][d2]: (buffer, offset, s0, s1, s2)
    def conv2_mirrors(self):
        return (self.w2f, 0, 9 * CS, 1, CS), (self.w2b, 8 * 64, 1, 9 * 64, -64)

    def fc1_mirror(self):
        return (self.wfc1, 0, FEATURES, 1, 64)                # [n][c][yx] -> n * 3136 + yx * 64 + c

    def pack(self):
        lib, st, net = cabi.lib(), _st(self.dev), self.net
        for buf, off, s0, s1, s2 in self.conv2_mirrors():
            cabi.check(lib.ld_seg_permute3(net.conv2.weight.data_ptr(), buf.data_ptr(), 64, 32, 9, off, s0, s1, s2, st),
                       "seg_permute3")
        buf, off, s0, s1, s2 = self.fc1_mirror()
        cabi.check(lib.ld_seg_permute3(net.fc1.weight.data_ptr(), buf.data_ptr(), HIDDEN, 64, 49, off, s0, s1, s2, st),
                   "seg_permute3")

    def plan(self, B, train):
        p = self.plans.get(B)
        if p is None:
            dev = self.dev
            f32 = dict(dtype=torch.float32, device=dev)
            p = {"p1": torch.zeros((B, 14, 14, CS), **f32), "a2": torch.empty((B, 14, 14, 64), **f32),
                 "p2": torch.empty((B, FEATURES), **f32), "work": torch.empty(49 * B * HIDDEN, **f32),
                 "h": torch.empty((B, HIDDEN), **f32)}
            self.plans[B] = p
        if train and "dz" not in p:
            dev = self.dev
            f32 = dict(dtype=torch.float32, device=dev)
            u8 = dict(dtype=torch.uint8, device=dev)
            lib = cabi.lib()
            splits = lib.ld_seg_wgrad_splits(B, 14, 14, CS, 64, 3)
            if splits < 1:
                raise RuntimeError("ld_seg_wgrad_splits refused conv2's shape")
            p.update({"idx1": torch.empty((B, 14, 14, 32), **u8), "idx2": torch.empty((B, FEATURES), **u8),
                      "logits": torch.empty((B, N_CLASSES), **f32), "loss_b": torch.empty(B, **f32),
                      "dz": torch.empty((B, N_CLASSES), **f32), "dh": torch.empty((B, HIDDEN), **f32),
                      "dp2": torch.empty((B, FEATURES), **f32), "da2": torch.empty((B, 14, 14, 64), **f32),
                      "dp1": torch.empty((B, 14, 14, CS), **f32), "splits2": splits,
                      "wg_work": torch.empty(splits * 64 * 9 * CS, **f32),
                      "red_work": torch.empty(RED_WORK_BYTES // 8, dtype=torch.float64, device=dev),
                      "c1_work": torch.empty(int(lib.ld_mc_conv1_wgrad_work_floats(B)), **f32)})
        return p

    def _pc_conv(self, src, weight, shift, out, B, relu):
        a = cabi.PcConvArgs()
        a.src, a.weight, a.scale, a.shift, a.residual, a.out = src.data_ptr(), weight.data_ptr(), self.ones.data_ptr(), \
            shift.data_ptr(), None, out.data_ptr()
        a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout, a.ksize, a.stride, a.relu = B, 14, 14, CS, 14, 14, 64, 3, 1, relu
        cabi.check(cabi.lib().ld_pc_conv(C.byref(a), _st(self.dev)), "pc_conv")

    def features(self, x, train):
        """x [B, 1, 28, 28] -> the plan with ``h`` [B, 128] = relu(fc1(...)) filled (and the pooling positions when
        training)."""
        B = x.shape[0]
        p = self.plan(B, train)
        lib, st, net = cabi.lib(), _st(self.dev), self.net
        idx1 = p["idx1"].data_ptr() if train else None
        idx2 = p["idx2"].data_ptr() if train else None
        cabi.check(lib.ld_mc_conv1(x.data_ptr(), net.conv1.weight.data_ptr(), net.conv1.bias.data_ptr(), p["p1"].data_ptr(), idx1,
                                   B, st), "mc_conv1")
        self._pc_conv(p["p1"], self.w2f, net.conv2.bias, p["a2"], B, 1)
        cabi.check(lib.ld_mc_pool(p["a2"].data_ptr(), p["p2"].data_ptr(), idx2, B, 7, 7, 64, st), "mc_pool")
        cabi.check(lib.ld_mc_gemm(p["p2"].data_ptr(), self.wfc1.data_ptr(), p["work"].data_ptr(), B, HIDDEN, FEATURES, FEATURES, 1,
                                  FEATURES, 1, HIDDEN, 49, st), "mc_gemm")
        cabi.check(lib.ld_mc_fc1_finish(p["work"].data_ptr(), net.fc1.bias.data_ptr(), p["h"].data_ptr(), B, HIDDEN, 49, st),
                   "mc_fc1_finish")
        return p

    def head(self, p, B, label, logits, pred):
        lib, st, net = cabi.lib(), _st(self.dev), self.net
        if label is None:
            cabi.check(lib.ld_mc_head(p["h"].data_ptr(), net.fc2.weight.data_ptr(), net.fc2.bias.data_ptr(), None,
                                      logits.data_ptr(), cabi.ptr(pred), None, None, None, None, B, st), "mc_head")
        else:
            cabi.check(lib.ld_mc_head(p["h"].data_ptr(), net.fc2.weight.data_ptr(), net.fc2.bias.data_ptr(), label.data_ptr(),
                                      logits.data_ptr(), cabi.ptr(pred), p["loss_b"].data_ptr(), p["dz"].data_ptr(),
                                      p["dh"].data_ptr(), self.bad_label.data_ptr(), B, st), "mc_head")


def _check_input(x):
    if x.dim() != 4 or tuple(x.shape[1:]) != (1, 28, 28) or x.shape[0] < 1:
        raise ValueError(f"MnistClassifier: input {tuple(x.shape)}, expected [B, 1, 28, 28]")
    if not torch.cuda.is_available() or not x.is_cuda:
        raise RuntimeError(_GPU_ONLY)
    return x.detach().to(torch.float32).contiguous()


class MnistClassifier(nn.Module):
    """``SimpleCNN``: logits [B, 10] (fp32) of NCHW images [B, 1, 28, 28] in the dataset's range 2 * u8 / 255."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 32, kernel_size=3, stride=1, padding=1)
        self.conv2 = nn.Conv2d(32, 64, kernel_size=3, stride=1, padding=1)
        self.fc1 = nn.Linear(FEATURES, HIDDEN)
        self.fc2 = nn.Linear(HIDDEN, N_CLASSES)
        for p in self.parameters():
            p.requires_grad_(False)
        self._packed = None

    # ------------------------------------------------------------------ cache control
    def invalidate(self):
        """Drop the device-side packed weights and buffers; they are rebuilt on next use.  Call it after changing a
        parameter in place (``.to()`` and ``load_state_dict`` do)."""
        self._packed = None

    def _apply(self, fn, *args, **kwargs):
        self.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        self.invalidate()
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    def packed(self, dev):
        pk = self._packed
        if pk is None or pk.dev != dev:
            pk = _Packed(self, dev)
            self._packed = pk
        return pk

    # ------------------------------------------------------------------ inference
    def _run(self, x, want_pred):
        x = _check_input(x)
        pk = self.packed(x.device)
        B = x.shape[0]
        p = pk.features(x, train=False)
        logits = torch.empty((B, N_CLASSES), dtype=torch.float32, device=x.device)
        pred = torch.empty(B, dtype=torch.int64, device=x.device) if want_pred else None
        pk.head(p, B, None, logits, pred)
        return pred, logits

    def forward(self, x):
        return self._run(x, False)[1]

    def predict(self, x):
        """-> (labels int64 [B], logits [B, 10]) on the device; the lowest index wins on equal logits, as
        ``torch.max(output, 1)`` (train_mnist_cls.py:110) does."""
        return self._run(x, True)


class MnistClassifierTrainer:
    """train_mnist_cls.py's optimisation loop over a ``MnistClassifier`` on the GPU (fp32).

    A label outside 0..9 never indexes anything on the device: its sample gets a NaN loss and no gradient, and a sticky
    device flag is raised, which ``check_labels()`` (called by ``fit`` once per epoch) turns into a ``ValueError``.  Labels
    that arrive on the host are validated there."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if not isinstance(model, MnistClassifier):
            raise TypeError("MnistClassifierTrainer trains a MnistClassifier")
        self.model, self.adam = model, StridedAdam(lr, betas, eps)
        self._grads = None

    @property
    def t(self):                  # optimisation steps taken
        return self.adam.t

    # ------------------------------------------------------------------ inputs
    def _label(self, x, label):
        if not torch.is_tensor(label) or label.dim() != 1 or label.shape[0] != x.shape[0]:
            raise ValueError(f"MnistClassifierTrainer: labels must be a tensor [B] for input {tuple(x.shape)}")
        if label.dtype != torch.int64:
            raise ValueError(f"MnistClassifierTrainer: labels must be int64, got {label.dtype}")
        if not label.is_cuda:                                  # host labels: validate before they leave the host
            if label.numel() and (int(label.min()) < 0 or int(label.max()) >= N_CLASSES):
                raise ValueError("MnistClassifierTrainer: label outside 0..9")
        return label.to(x.device).contiguous()

    def check_labels(self):
        """Raise ValueError if any step so far saw a label outside 0..9 (one host synchronisation)."""
        pk = self.model._packed
        if pk is not None and int(pk.bad_label.item()):
            pk.bad_label.zero_()
            raise ValueError("MnistClassifierTrainer: a label outside 0..9 was seen (its sample was left out of the gradient "
                             "and its loss is NaN)")

    # ------------------------------------------------------------------ one step
    def _grad_buffers(self, dev):
        if self._grads is None or self._grads["conv1.weight"].device != dev:
            f32 = dict(dtype=torch.float32, device=dev)
            self._grads = {"conv1.weight": torch.empty(32 * 9, **f32), "conv1.bias": torch.empty(32, **f32),
                           "conv2.weight": torch.empty(64 * 9 * CS, **f32), "conv2.bias": torch.empty(64, **f32),
                           "fc1.weight": torch.empty(HIDDEN * FEATURES, **f32), "fc1.bias": torch.empty(HIDDEN, **f32),
                           "fc2.weight": torch.empty(N_CLASSES * HIDDEN, **f32), "fc2.bias": torch.empty(N_CLASSES, **f32),
                           "loss": torch.empty(1, **f32)}
        return self._grads

    # parameter seen as [d0][d1][d2] and the strides of its gradient buffer
    _VIEWS = {"conv1.weight": ((1, 1, 288), (0, 0, 1)), "conv1.bias": ((1, 1, 32), (0, 0, 1)),
              "conv2.weight": ((64, 32, 9), (9 * CS, 1, CS)), "conv2.bias": ((1, 1, 64), (0, 0, 1)),
              "fc1.weight": ((HIDDEN, 64, 49), (FEATURES, 1, 64)), "fc1.bias": ((1, 1, HIDDEN), (0, 0, 1)),
              "fc2.weight": ((1, 1, N_CLASSES * HIDDEN), (0, 0, 1)), "fc2.bias": ((1, 1, N_CLASSES), (0, 0, 1))}

    def _forward_backward(self, x, label):
        x = _check_input(x)
        label = self._label(x, label)
        pk = self.model.packed(x.device)
        B = x.shape[0]
        g = self._grad_buffers(x.device)
        lib, st = cabi.lib(), _st(x.device)
        p = pk.features(x, train=True)
        pk.head(p, B, label, p["logits"], None)
        cabi.check(lib.ld_mc_small_grads(p["dz"].data_ptr(), p["h"].data_ptr(), p["dh"].data_ptr(), p["loss_b"].data_ptr(),
                                         g["fc2.weight"].data_ptr(), g["fc2.bias"].data_ptr(), g["fc1.bias"].data_ptr(),
                                         g["loss"].data_ptr(), B, st), "mc_small_grads")
        # fc1: dW [n][f] = sum_b dh[b][n] p2[b][f] (NHWC feature order); dp2 [b][f] = sum_n dh[b][n] W[n][f]
        cabi.check(lib.ld_mc_gemm(p["dh"].data_ptr(), p["p2"].data_ptr(), g["fc1.weight"].data_ptr(), HIDDEN, FEATURES, B, 1, HIDDEN,
                                  1, FEATURES, FEATURES, 1, st), "mc_gemm")
        cabi.check(lib.ld_mc_gemm(p["dh"].data_ptr(), pk.wfc1.data_ptr(), p["dp2"].data_ptr(), B, FEATURES, HIDDEN, HIDDEN, 1, 1,
                                  FEATURES, FEATURES, 1, st), "mc_gemm")
        cabi.check(lib.ld_mc_pool_backward(p["dp2"].data_ptr(), p["p2"].data_ptr(), p["idx2"].data_ptr(), p["da2"].data_ptr(), B,
                                           7, 7, 64, st), "mc_pool_backward")
        cabi.check(lib.ld_seg_colsum(p["da2"].data_ptr(), p["red_work"].data_ptr(), g["conv2.bias"].data_ptr(), B * 196, 64, 1, st),
                   "seg_colsum")
        cabi.check(lib.ld_seg_wgrad(p["da2"].data_ptr(), p["p1"].data_ptr(), p["wg_work"].data_ptr(), g["conv2.weight"].data_ptr(),
                                    B, 14, 14, CS, 64, 3, p["splits2"], st), "seg_wgrad")
        pk._pc_conv(p["da2"], pk.w2b, pk.zeros, p["dp1"], B, 0)
        cabi.check(lib.ld_mc_conv1_wgrad(x.data_ptr(), p["p1"].data_ptr(), p["dp1"].data_ptr(), p["idx1"].data_ptr(),
                                         p["c1_work"].data_ptr(), g["conv1.weight"].data_ptr(), g["conv1.bias"].data_ptr(), B, st),
                   "mc_conv1_wgrad")
        return pk, p, g

    def loss_and_grads(self, x, label):
        """-> (loss, {name: gradient in the parameter's own shape}) at the current weights; changes nothing."""
        _, _, g = self._forward_backward(x, label)
        out = {}
        for name, prm in self.model.named_parameters():
            dims, strides = self._VIEWS[name]
            out[name] = torch.as_strided(g[name], dims, strides).reshape(prm.shape).clone()
        return g["loss"][0].clone(), out

    def _adam(self, pk, g):
        mirrors = {"conv2.weight": pk.conv2_mirrors(), "fc1.weight": (pk.fc1_mirror(),)}
        self.adam.step([(n, prm, g[n]) + self._VIEWS[n] + (mirrors.get(n, ()),) for n, prm in self.model.named_parameters()],
                       pk.dev)

    def step(self, x, label):
        """One optimisation step (train_mnist_cls.py:91-96) -> the loss before the step as a device scalar; no host
        synchronisation."""
        pk, _, g = self._forward_backward(x, label)
        loss = g["loss"][0].clone()
        self._adam(pk, g)
        return loss

    # ------------------------------------------------------------------ evaluation, epochs
    def evaluate(self, x, label):
        """train_mnist_cls.py:106-112 on one batch -> (number correct as a device scalar, number seen)."""
        pred, _ = self.model.predict(x)
        label = self._label(pred, label)
        return (pred == label).sum(), int(pred.shape[0])

    def fit(self, train_batches, test_batches, epochs, out_path, csv_path=None):
        """The epochs of train_mnist_cls.py:86-119.  ``train_batches`` / ``test_batches`` are sequences of (x, label), or
        ``train_batches`` is a callable epoch -> such a sequence.  After every epoch: the test accuracy (in percent);
        ``torch.save(model.state_dict(), out_path)`` when it is strictly better than the best so far (:114-116); the CSV
        row ``epoch, train_loss, accuracy`` -- where, as in the reference, whose ``loss_lst`` is never cleared (:85, 95,
        100), ``train_loss`` is the mean over ALL steps since the start, not over the epoch.  Losses come to the host once
        per epoch.  -> {'best_acc', 'best_epoch', 'rows'}.

        Either may be a ``dataset.BatchSource`` over a ``DeviceDataset.mnist_cls``.  As ``train_batches`` it is asked for
        ``batches(epoch)`` -- the epoch's shuffle and augmentation -- and walked lazily: batch k + 1 is made after batch k's step
        was enqueued, and nothing new synchronises inside an epoch.  As ``test_batches`` it is walked as ``batches(0)`` at every
        epoch, so every epoch tests on the same batches.  ``fit`` over sources is bit-identical to
        ``fit(lambda e: list(source.batches(e)), list(test.batches(0)), ...)``."""
        best, best_epoch, rows, losses = 0.0, None, [], []
        for e in range(int(epochs)):
            self.model.train()
            dev_losses = [self.step(x, y) for x, y in epoch_batches(train_batches, e)]
            if dev_losses:
                losses += [float(v) for v in torch.stack(dev_losses).cpu().tolist()]
            self.check_labels()
            loss_mean = sum(losses) / len(losses) if losses else float("nan")
            self.model.eval()
            counts = [self.evaluate(x, y) for x, y in epoch_batches(test_batches)]
            total = sum(n for _, n in counts)
            correct = int(torch.stack([c for c, _ in counts]).sum().item()) if counts else 0
            acc = 100 * correct / total if total else 0.0
            if best < acc:
                best, best_epoch = acc, e
                torch.save({k: v.detach().cpu() for k, v in self.model.state_dict().items()}, out_path)
            rows.append((e, loss_mean, acc))
            if csv_path is not None:
                with open(csv_path, "w", newline="") as f:
                    csv.writer(f).writerows([("epoch", "train_loss", "accuracy")] + rows)
        return {"best_acc": best, "best_epoch": best_epoch, "rows": rows}
