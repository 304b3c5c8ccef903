"""The MNIST digit classifier (train_mnist_cls.py:31-47) and its training step (:91-96) restated in plain PyTorch over
``MnistClassifier``'s parameter names: F.conv2d, F.max_pool2d, F.linear, F.cross_entropy, autograd and an explicit Adam.
dtype-generic (the tests run it in fp64 as the yardstick), CPU only, like segtrain_ref.py."""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm()) / max(1e-300, float(ref.double().norm()))


def images_of(u8, dtype=torch.float32):
    """uint8 [N, 28, 28] -> [N, 1, 28, 28] in the dataset's range: 2 * (u8 / 255) (data.py:809)."""
    x = torch.from_numpy(np.ascontiguousarray(u8)).to(dtype)[:, None]
    return 2.0 * (x / 255.0)


def params_of(sd, dtype):
    """state_dict (tensors or numpy arrays) -> leaf tensors in state_dict order."""
    return OrderedDict((k, torch.as_tensor(v).detach().cpu().to(dtype).clone().requires_grad_(True)) for k, v in sd.items())


def forward(params, x):
    h = F.max_pool2d(F.relu(F.conv2d(x, params["conv1.weight"], params["conv1.bias"], padding=1)), 2)
    h = F.max_pool2d(F.relu(F.conv2d(h, params["conv2.weight"], params["conv2.bias"], padding=1)), 2)
    h = h.view(-1, 64 * 7 * 7)
    h = F.relu(F.linear(h, params["fc1.weight"], params["fc1.bias"]))
    return F.linear(h, params["fc2.weight"], params["fc2.bias"])


def loss_and_grads(params, x, label):
    dtype = next(iter(params.values())).dtype
    loss = F.cross_entropy(forward(params, x.to(dtype)), label)
    grads = torch.autograd.grad(loss, list(params.values()))
    return loss.detach(), OrderedDict(zip(params.keys(), grads))


class Adam:
    """torch.optim.Adam(lr, betas, eps) without weight decay / amsgrad, written out."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.params, self.lr, self.betas, self.eps, self.t = params, lr, betas, eps, 0
        self.m = {k: torch.zeros_like(v) for k, v in params.items()}
        self.v = {k: torch.zeros_like(v) for k, v in params.items()}

    def step(self, grads):
        self.t += 1
        b1, b2 = self.betas
        step_size, bc2_sqrt = self.lr / (1.0 - b1 ** self.t), math.sqrt(1.0 - b2 ** self.t)
        with torch.no_grad():
            for k, p in self.params.items():
                g = grads[k]
                self.m[k].lerp_(g, 1.0 - b1)
                self.v[k].mul_(b2).addcmul_(g, g, value=1.0 - b2)
                p.addcdiv_(self.m[k], self.v[k].sqrt() / bc2_sqrt + self.eps, value=-step_size)


def train_steps(sd, batches, dtype=torch.float64, lr=1e-3, keep=()):
    """One Adam step per (x, label) batch in order -> (losses, {step number: parameters after it} for ``keep``, params)."""
    params = params_of(sd, dtype)
    opt = Adam(params, lr=lr)
    losses, kept = [], {}
    for i, (x, y) in enumerate(batches):
        loss, grads = loss_and_grads(params, x, y)
        opt.step(grads)
        losses.append(float(loss))
        if i + 1 in keep:
            kept[i + 1] = OrderedDict((k, v.detach().clone()) for k, v in params.items())
    return losses, kept, params


def epoch_batches(x, y, epochs, batch=64):
    """The batches of ``epochs`` passes over (x, y) in file order."""
    return [(x[i:i + batch], y[i:i + batch]) for _ in range(epochs) for i in range(0, x.shape[0], batch)]
