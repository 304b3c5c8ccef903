"""``torch.optim.Adam`` (no weight decay, no amsgrad) for ``SegTrainer`` and ``MnistClassifierTrainer``: one ``ld_seg_adam``
call over all parameters, which reads every gradient through the strides of its kernel layout and writes every updated
value into the weight's kernel-layout copies (mirrors) as well, so nothing is repacked after a step."""
import math

import torch

from . import _cabi as cabi


class StridedAdam:
    def __init__(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.t = 0
        self._moments, self._dev = None, None

    def step(self, entries, dev):
        """``entries``: per parameter ``(name, parameter, gradient buffer, (d0, d1, d2), gradient strides, mirrors)`` -- the
        parameter seen as [d0][d1][d2], its gradient element at i0 s0 + i1 s1 + i2 s2 of the buffer, up to two mirrors
        ``(buffer, off, s0, s1, s2)`` as ``ld_seg_permute3`` takes them.  Moments: made on first use or a new device."""
        if self._moments is None or self._dev != dev:
            self._dev, self._moments = dev, {n: (torch.zeros_like(prm), torch.zeros_like(prm)) for n, prm, *_ in entries}
        self.t += 1
        b1, b2 = self.betas
        step_size = self.lr / (1.0 - b1 ** self.t)           # bias corrections in double on the host
        bc2_sqrt = math.sqrt(1.0 - b2 ** self.t)
        arr = (cabi.SegAdamTensor * len(entries))()
        for a, (n, prm, g, dims, strides, mirrors) in zip(arr, entries):
            m, v = self._moments[n]
            a.param, a.grad, a.m, a.v = prm.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            (a.d0, a.d1, a.d2), (a.gs0, a.gs1, a.gs2) = dims, strides
            assert len(mirrors) <= 2, n                       # the struct has mirror0 and mirror1
            for k, (buf, *where) in enumerate(mirrors):
                for field, value in zip(("mirror%d", "m%d_off", "m%d_s0", "m%d_s1", "m%d_s2"), (buf.data_ptr(), *where)):
                    setattr(a, field % k, value)
        cabi.check(cabi.lib().ld_seg_adam(arr, len(entries), b1, b2, self.eps, step_size, bc2_sqrt,
                                          torch.cuda.current_stream(dev).cuda_stream), "seg_adam")
