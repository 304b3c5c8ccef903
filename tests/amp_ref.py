"""The CPU yardsticks of mixed-precision training (``amp = "fp16"``: the fp16 forms of csrc/conv16.hip and the loss scaler of
csrc/denoiser_opt.hip).  Pure torch, no GPU import.

* The convolutions: ``conv16_ref``'s functions with ``h`` (round to fp16, nearest even, overflow to inf) as the rounding, and
  exact probes in its style whose operands tell the three candidate kernels apart: integers that fp16 holds and bf16 does not
  (257 .. 2047: a bf16 kernel rounds them, an fp16 kernel must not) and exact fp16 ties (odd integers in [2049, 4095]: the
  even neighbour wins; truncation and bf16 rounding give something else).  Every builder asserts its own preconditions --
  every product and partial sum an integer below 2^24, and the expected result different from the unrounded, the truncated
  and the bf16-rounded one -- so tests/test_amp_ref.py proves the probes without a GPU.
* The scaler: ``scaler_rule`` restates ``ld_dn_opt_scaler_update`` literally; ``ScaledReplica`` is ``denoiser_train_ref.Replica``
  with the real ``torch.amp.GradScaler('cpu')`` around its Adam (``unscale_``, ``clip_grad_norm_``, ``step``, ``update``).
* ``fp16_convs``: the CPU denoiser (``unet_grad_ref.unet_forward``) with every convolution but the head on fp16-rounded
  operands, forward and both gradients: what shows at which loss scale the fp16 operands overflow.
"""
import contextlib
import math
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

import conv16_ref as P
import denoiser_train_ref as T
from exact_probes import check_exact, ints, is_integer, trits

LIMIT = P.LIMIT
F16_MAX = 65504.0


def h(t):
    """Round to fp16 (nearest even, beyond 65504 + half a step: inf) and back."""
    return t.to(torch.float16).to(t.dtype)


def trunc16(t):
    """Chop an fp32 tensor of fp16-normal magnitude to fp16's 11 significand bits (a kernel that drops bits instead of
    rounding)."""
    return (t.contiguous().view(torch.int32) & -8192).view(torch.float32)


def _same(t):
    return t


# --------------------------------------------------------------------------------------------- the probes' operands
def fp16_only_ints(shape, key):
    """+- integers in [257, 2047]: fp16 holds every one, bf16 (8 significand bits) holds only a few of them."""
    v = ints(shape, key, 257, 2047)
    return v * (2 * ints(shape, key + 3, 0, 1) - 1)


def fp16_ties(shape, key):
    """+- odd integers in [2049, 4095] (fp16's spacing there is 2: each is an exact tie, the even neighbour wins), mixed with
    integers in [257, 2047] that must come through untouched."""
    odd = 2 * ints(shape, key, 1024, 2047) + 1
    v = torch.where(ints(shape, key + 2, 0, 2) == 0, ints(shape, key + 1, 257, 2047), odd)
    return v * (2 * ints(shape, key + 3, 0, 1) - 1)


def _check_probe(fn, operand, rounds):
    """``fn(rnd, dt)``: the probe's result with ``rnd`` as the rounding.  The result with fp16 rounding is exact, and it is
    not what a bf16 kernel, a truncating kernel or (where the operand needs rounding) a kernel that does not round gives."""
    ref32 = fn(h, torch.float32)
    check_exact(ref32, fn(h, torch.float64), limit=LIMIT)
    assert torch.equal(h(operand), operand) != rounds
    assert not torch.equal(P.q(operand), operand)                     # bf16 does not hold the operand ...
    assert not torch.equal(ref32, fn(P.q, torch.float32))             # ... and a launch routed to the bf16 kernel shows
    if rounds:
        assert not torch.equal(ref32, fn(_same, torch.float32))
        assert not torch.equal(ref32, fn(trunc16, torch.float32))
        assert not torch.equal(ref32, fn(P.trunc, torch.float32))
    return ref32


def _operand(kind, shape, key):
    return fp16_only_ints(shape, key) if kind.startswith("identity") else fp16_ties(shape, key)


def conv_probe(shape, kind, epilogue=False, key=9000):
    """``kind`` "identity": x = fp16_only_ints (no rounding may happen), "rounding": x = fp16_ties; w in {-1, 0, 1}.  With
    K <= 9 * 128 every sum stays below 1152 * 4095 < 2^24."""
    B, cin, cout, H, W, k = shape
    assert k * k * cin * 4095 < LIMIT
    key += 100 * cin + 10 * H + k
    shift, res = P._epilogue(shape, key, epilogue)
    x, w = _operand(kind, (B, cin, H, W), key), trits((cout, cin, k, k), key + 7)
    ref = _check_probe(lambda rnd, dt: P.conv_ref(x, w, shift, res, dt, rnd), x, kind == "rounding")
    return NS(x=x, w=w, shift=shift, res=res, ref=ref)


def dgrad_probe(shape, kind, key=9300):
    """The data gradient; ``kind`` "identity_w" / "rounding_w" (the packed weight holds the integers: ld_dn_pack_conv_f16
    rounds it) or "identity_dy" / "rounding_dy"."""
    B, cin, cout, H, W, k = shape
    assert k * k * cout * 4095 < LIMIT
    key += 100 * cin + 10 * H + k
    if kind.endswith("_w"):
        dy, w = trits((B, cout, H, W), key), _operand(kind, (cout, cin, k, k), key + 7)
        ref = _check_probe(lambda rnd, dt: P.dgrad_ref(dy, w, dt, rnd), w, kind.startswith("rounding"))
    else:
        dy, w = _operand(kind, (B, cout, H, W), key), trits((cout, cin, k, k), key + 7)
        ref = _check_probe(lambda rnd, dt: P.dgrad_ref(dy, w, dt, rnd), dy, kind.startswith("rounding"))
    return NS(dy=dy, w=w, ref=ref)


def wgrad_probe(shape, kind, key=9600):
    """``kind`` "identity_dy", "rounding_dy", "identity_a" or "rounding_a" (which operand holds the integers)."""
    B, cin, cout, H, W, k = shape
    assert B * H * W * 4095 < LIMIT
    key += 100 * cin + 10 * H + k
    ds, as_ = (B, cout, H, W), (B, cin, H, W)
    if kind.endswith("_dy"):
        dy, a = _operand(kind, ds, key), trits(as_, key + 7)
        ref = _check_probe(lambda rnd, dt: P.wgrad_ref(dy, a, k, dt, rnd), dy, kind.startswith("rounding"))
    else:
        dy, a = trits(ds, key), _operand(kind, as_, key + 7)
        ref = _check_probe(lambda rnd, dt: P.wgrad_ref(dy, a, k, dt, rnd), a, kind.startswith("rounding"))
    return NS(dy=dy, a=a, ref=ref)


def pack_probe(shape, key=9900):
    """An OIHW weight of fp16 ties and fp16-only integers and its two padded kernel layouts, rounded to fp16."""
    co, ci, k = shape
    cop, cip = (co + 63) // 64 * 64, (ci + 63) // 64 * 64
    w = fp16_ties((co, ci, k, k), key + 10 * co + ci)
    assert not torch.equal(h(w), w) and not torch.equal(h(w), trunc16(w)) and not torch.equal(h(w), P.q(w)) and is_integer(h(w))
    fwd, dgr = P.pack_ref(h(w), cop, cip)
    return NS(w=w, cop=cop, cip=cip, fwd=fwd, dgr=dgr)


# --------------------------------------------------------------------------------------------- the scaler's rule
def scaler_rule(state, finite, lr, betas, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """``ld_dn_opt_scaler_update`` restated literally on a dict with the fields of ``ld_dn_scaler_state`` (in place; floats
    are Python doubles except where the kernel rounds to fp32).  ``finite``: whether the squared norm of the scaled gradients
    is finite.  Returns ``state``."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).to(torch.float32))          # noqa: E731
    found_inf = not finite
    state["found_inf"] = int(found_inf)
    state["inv_scale"] = f32(1.0 / state["scale"])
    if not found_inf:
        state["adam_steps"] += 1
        t = state["adam_steps"]
        state["step_size"] = f32(lr / (1.0 - betas[0] ** t))
        state["bc2_sqrt"] = f32(math.sqrt(1.0 - betas[1] ** t))
        state["growth_tracker"] += 1
        if state["growth_tracker"] == growth_interval:
            grown = f32(state["scale"] * growth_factor)
            if math.isfinite(grown):
                state["scale"] = grown
            state["growth_tracker"] = 0
    else:
        state["skipped_steps"] += 1
        state["scale"] = f32(state["scale"] * backoff_factor)
        state["growth_tracker"] = 0
    return state


def scaler_state(init_scale=65536.0, adam_steps=0, growth_tracker=0):
    """What ``ld_dn_scaler_init`` fills."""
    return dict(scale=float(init_scale), growth_tracker=growth_tracker, adam_steps=adam_steps, skipped_steps=0, found_inf=0,
                inv_scale=1.0 / init_scale, step_size=0.0, bc2_sqrt=1.0)


class ScaledReplica(T.Replica):
    """``denoiser_train_ref.Replica`` fed with SCALED gradients, its Adam driven by the real ``torch.amp.GradScaler('cpu')``:
    ``unscale_``, ``clip_grad_norm_``, ``scaler.step``, ``scaler.update``, ``zero_grad``, then the EMA rule whatever the
    scaler decided (ddpm.py:1558-1571)."""

    def __init__(self, params, lr, max_norm=1.0, dtype=torch.float32, ema_kw=None, no_grad=T.NO_GRAD, **scaler_kw):
        super().__init__(params, lr, max_norm, dtype, ema_kw, no_grad)
        self.scaler = torch.amp.GradScaler("cpu", **scaler_kw)
        self.skipped = []

    def step(self, grads):
        self.scaler.scale(torch.zeros(1))                                # (the call that creates the scale tensor lazily)
        for k in self.trained:
            self.p[k].grad = grads[k].detach().to(self.dtype).clone()
        self.scaler.unscale_(self.opt)
        self.norm = float(torch.nn.utils.clip_grad_norm_([self.p[k] for k in self.trained], self.max_norm))
        before = self.adam_steps()
        self.scaler.step(self.opt)
        self.scaler.update()
        self.skipped.append(self.adam_steps() == before)
        self.opt.zero_grad()
        what = None
        if self.ema_kw is not None:
            what, self.initted = T.ema_update(self.s, self.ema, self.p, self.initted, **self.ema_kw)
            self.s += 1
        return what

    def adam_steps(self):
        steps = {int(st["step"]) for st in self.opt.state.values()}
        assert len(steps) <= 1
        return steps.pop() if steps else 0


# --------------------------------------------------------------------------------------------- the CPU denoiser on fp16 operands
_conv2d = F.conv2d


class H16Conv(torch.autograd.Function):
    """A stride-1 "same" convolution on fp16-rounded operands, forward and both gradients (``conv16_ref.Bf16Conv`` with ``h``),
    written on the saved ``F.conv2d`` so that it can stand in for it."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return _conv2d(h(x), h(w), b, padding=w.shape[-1] // 2)

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        pad = w.shape[-1] // 2
        dx = F.conv_transpose2d(h(dout), h(w), padding=pad)
        dw = _conv2d(h(x).transpose(0, 1), h(dout).transpose(0, 1), padding=pad).transpose(0, 1)
        return dx, dw, (dout.sum(dim=(0, 2, 3)) if ctx.has_bias else None)


@contextlib.contextmanager
def fp16_convs():
    """Inside, ``torch.nn.functional.conv2d`` rounds its operands to fp16 in the forward and in both gradients, except for
    the head (at most 8 output channels: ``final_conv`` stays fp32, as under ``conv_precision = "bf16"``)."""
    def conv2d(x, w, b=None, stride=1, padding=0):
        assert stride == 1 and padding == w.shape[-1] // 2
        if w.shape[0] <= 8:
            return _conv2d(x, w, b, padding=padding)
        return H16Conv.apply(x, w, b)
    F.conv2d = conv2d
    try:
        yield
    finally:
        F.conv2d = _conv2d


def first_step_grads(case, sd, schedule, objective, timesteps, loss_scale, n_batches=2, dtype=torch.float32):
    """The accumulated gradients of step 0 of ``denoiser_train_ref.yardstick_steps`` with the loss multiplied by
    ``loss_scale`` and the convolutions on fp16 operands: {name: gradient}."""
    import unet_grad_ref as R
    cfg = R.CONFIGS[case[0]]
    leaves = R.leaves_of(sd, dtype)
    trained = [k for k in leaves if k not in T.NO_GRAD]
    grads = None
    with fp16_convs():
        for j in range(n_batches):
            hr, cond, t, noise = T.batch(case, 0, j, timesteps)
            x = T.q_sample(hr, t, noise, schedule, dtype)
            out = R.unet_forward(leaves, cfg, x, cond.to(dtype), t, dtype)
            value = R.loss(out, hr, noise, t, *schedule, objective, dtype) / n_batches * loss_scale
            g = torch.autograd.grad(value, [leaves[k] for k in trained])
            grads = list(g) if grads is None else [a + b for a, b in zip(grads, g)]
    return dict(zip(trained, grads))
