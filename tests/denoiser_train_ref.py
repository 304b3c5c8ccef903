"""Helpers of the ``DenoiserTrainer`` tests: the reference's training step (ddpm.py:1532-1571) on the CPU, in any dtype --
``unet_grad_ref.unet_forward`` + ``loss`` under ``torch.autograd``, ``clip_grad_norm_``, ``torch.optim.Adam(foreach=False)`` and
``ema_pytorch``'s update rule written out literally (skip / copy / copy-on-first-use then lerp), not through
``denoiser_train.ema_action`` --, the batches of the trainer tests, and the comparisons they share.  CPU only."""
from collections import OrderedDict

import torch

from localdiffusion_hallucination_amd import rng

import unet_grad_ref as R

F32, F64 = torch.float32, torch.float64
NO_GRAD = ("conv_fusion.mlp.1.weight", "conv_fusion.mlp.1.bias")
EMA_KW = dict(beta=0.995, update_every=2, update_after_step=2, inv_gamma=1.0, power=2 / 3, min_value=0.0)   # the trainer tests'
ADAM = dict(betas=(0.9, 0.99), eps=1e-8)
ADAM_RTOL = 2.4e-7            # test_hip_mnistcls.py / test_hip_segtrain.py: two ulps, and 1e-5 lr of absolute slack


def ema_decay(s, beta, update_after_step, inv_gamma, power, min_value, **_):
    e = max(s + 1 - update_after_step - 1, 0)
    if e <= 0:
        return 0.0
    return min(max(1.0 - (1.0 + e / inv_gamma) ** -power, min_value), beta)


def ema_update(s, ema, online, initted, **kw):
    """``EMA.update()`` number ``s`` on dictionaries of CPU tensors, in place; returns (what happened, initted)."""
    if s % kw["update_every"] != 0:
        return "skip", initted
    if s <= kw["update_after_step"]:
        for k in ema:
            ema[k].copy_(online[k].detach())
        return "copy", initted
    if not initted:
        for k in ema:
            ema[k].copy_(online[k].detach())
    w = 1.0 - ema_decay(s, **kw)
    for k in ema:
        ema[k].lerp_(online[k].detach(), w)
    return "lerp", True


class Replica:
    """clip_grad_norm_ + Adam + the EMA rule on CPU copies of the parameters, fed with gradients from outside."""

    def __init__(self, params, lr, max_norm=1.0, dtype=F32, ema_kw=None, no_grad=NO_GRAD):
        self.p = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in params.items())
        self.trained = [k for k in self.p if k not in no_grad]
        self.opt = torch.optim.Adam([self.p[k] for k in self.trained], lr=lr, foreach=False, **ADAM)
        self.ema = OrderedDict((k, v.detach().clone()) for k, v in self.p.items())
        self.max_norm, self.dtype, self.ema_kw, self.s, self.initted = max_norm, dtype, ema_kw, 0, False
        self.norm = None

    def step(self, grads):
        for k in self.trained:
            self.p[k].grad = grads[k].detach().to(self.dtype).clone()
        self.norm = float(torch.nn.utils.clip_grad_norm_([self.p[k] for k in self.trained], self.max_norm))
        self.opt.step()
        self.opt.zero_grad()
        what = None
        if self.ema_kw is not None:
            what, self.initted = ema_update(self.s, self.ema, self.p, self.initted, **self.ema_kw)
            self.s += 1
        return what

    def moments(self, k):
        st = self.opt.state[self.p[k]]
        return st["exp_avg"], st["exp_avg_sq"]

    def reset_params(self, params, ema=None):
        with torch.no_grad():
            for k, v in params.items():
                self.p[k].copy_(v.to(self.dtype))
            for k, v in (ema or {}).items():
                self.ema[k].copy_(v.to(self.dtype))


def adam_close(got, want, lr, what):
    """The rule of test_hip_mnistcls.py and test_hip_segtrain.py: allclose(rtol 2.4e-7, atol 1e-5 lr); returns the largest
    excess-free distance in units of the bound."""
    bound = 1e-5 * lr + ADAM_RTOL * want.abs()
    worst = float(((got - want).abs() / bound).max())
    assert torch.allclose(got, want, rtol=ADAM_RTOL, atol=1e-5 * lr), f"{what}: {worst:.2f} of the allclose bound"
    return worst


# ------------------------------------------------------------------------------------------------ the trainer's batches
def batch(case, step, j, timesteps):
    """Batch ``j`` of step ``step``: hr, lr (the case's condition image: no ReLU or pool tie within the margin), t, noise."""
    data, B, H, W = case
    cfg = R.CONFIGS[data]
    key = 1000 + 10 * step + j
    _, _, cond, _, _ = R.inputs(case)
    hr = R.uniform((B, cfg.channels, H, W), key)
    noise = torch.from_numpy(rng.randn((B, cfg.channels, H, W), 7, key + 5000))
    t = torch.tensor([(37 * (key + b) + 11 * b) % timesteps for b in range(B)], dtype=torch.long)
    return hr, cond, t, noise


def q_sample(hr, t, noise, schedule, dtype):
    sab, s1m = (v.to(dtype)[t][:, None, None, None] for v in schedule[:2])
    return sab * hr.to(dtype) + s1m * noise.to(dtype)


def yardstick_steps(case, sd, schedule, objective, lr, steps, n_batches, timesteps, dtype, ema_kw=None, max_norm=1.0):
    """``steps`` steps of the reference's ``Trainer.train`` on the CPU in ``dtype``: per step ``n_batches`` batches of
    ``batch()``, each loss divided by their number, the gradients accumulated; clip, Adam, EMA.  Returns the summed loss of
    every step and the ``Replica`` (parameters, moments, EMA)."""
    cfg = R.CONFIGS[case[0]]
    rep = Replica(sd, lr, max_norm, dtype, ema_kw)
    losses = []
    for s in range(steps):
        total = 0.0
        grads = None
        for j in range(n_batches):
            hr, cond, t, noise = batch(case, s, j, timesteps)
            x = q_sample(hr, t, noise, schedule, dtype)
            out = R.unet_forward(rep.p, cfg, x, cond.to(dtype), t, dtype)
            value = R.loss(out, hr, noise, t, *schedule, objective, dtype) / n_batches
            total += float(value.detach())
            g = torch.autograd.grad(value, [rep.p[k] for k in rep.trained])
            grads = list(g) if grads is None else [a + b for a, b in zip(grads, g)]
        rep.step(dict(zip(rep.trained, grads)))
        losses.append(total)
    return losses, rep
