"""``DenoiserTrainer``: the reference's training step for the denoiser (``Trainer.train``, ddpm.py:1532-1606) on HIP kernels --
the seventh slice of the denoiser's backward pass.

A step is: for every batch of the loader the loss divided by the number of batches, its gradients accumulated
(``accumulate``: ``normalize`` -> ``q_sample`` -> ``TrainableUnet`` -> ``ld_p_losses`` -> ``p_losses_grad`` -> ``out.backward``);
then ``apply``: ``clip_grad_norm_(max_grad_norm)``, ``Adam(lr, betas)``, ``zero_grad`` and ``ema.update()`` as two launches of
``csrc/denoiser_opt.hip`` over every parameter tensor at once.  ``ld_dn_opt_sqnorm`` leaves the squared norm of all gradients
in device memory, ``ld_dn_opt_step`` reads it there, so nothing in a step waits for the GPU: the host decides what the EMA
does from integer counters alone (``ema_action``).

Where things live.  ``diffusion`` (an ``ldh.GaussianDiffusion`` on the GPU) gives the schedule, the objective, ``normalize``,
the noise stream and the offset noise; its ``.model``, the inference ``Unet``, plays the reference's ``ema.ema_model`` (``sample``
runs on it; ``sync_ema`` loads the EMA weights into it).  The online model is a ``TrainableUnet`` built from
``diffusion.model``'s configuration and weights.  Gradients, both Adam moments and the EMA weights are four flat fp32 buffers in
which every parameter owns a 16-byte aligned segment (``ld_dn_opt_layout``); each ``.grad`` is a view of its segment, which
autograd accumulates into in place and the step's launch zeroes, so the ``.grad`` tensors keep their addresses.
``conv_fusion.mlp.1.weight`` / ``.bias`` get no gradient (the reference calls ``conv_fusion`` without a time embedding): they
have no moments, are not in the norm, and are in the EMA.

The EMA rule is ``ema_pytorch.EMA.update`` restated from its source (``ema_action``); the package is not available where
this was built, so the rule could not be checked against it.

More than one GPU (``group=`` a torch process group, or ``comm=`` an ``LdComm``): the reference's
``Accelerator(split_batches=True)``.  Every rank is handed the same global batches and takes its rows of each
(``dist.shard_bounds``); a micro-batch is scaled by ``1 / (world * len(batches))``.  ``apply`` then all-gathers the ranks' flat
gradients -- one collective of ``flat + 4`` floats per rank, whose extra slot carries the rank's summed loss -- and
``ld_dn_opt_reduce`` adds the ``world`` copies IN RANK ORDER (plain fp32, left to right) while it gathers the squared norm in
``ld_dn_opt_sqnorm``'s order; ``ld_dn_opt_step`` follows unchanged on identical inputs.  So the replicas hold the same bits
after every step (``replica_digest`` checks it), and a W-rank step equals a one-rank step that accumulated the same W
micro-batches in order.  Drawn ``t`` and noise are the rank's rows of what one rank would draw for the global batch (seed all
ranks alike).  The gather is not overlapped with the backward pass.

Mixed precision as the reference has it (``amp=True, mixed_precision_type="fp16"``, ddpm.py:1269-1284): the online model's
convolutions run on the fp16 matrix cores (``TrainableUnet.amp``: operands rounded to fp16, everything in memory fp32 -- not
autocast's fp16 activations) under ``torch.amp.GradScaler``'s loss scaling, whose state (``ld_dn_scaler_state``) and whose
decisions live on the device.  ``accumulate`` multiplies the loss gradient by the scale it reads there
(``ld_p_losses_grad_scaled``); ``apply`` puts one one-thread launch, ``ld_dn_opt_scaler_update``, between the norm and the step:
the squared norm of the scaled gradients is non-finite exactly when one of them is, and from it alone the kernel decides skip or
step, backs the scale off or grows it, and computes Adam's bias corrections for Adam's OWN step count, which a skipped step
does not advance; ``ld_dn_opt_step_scaled`` reads all of that from the state, unscales, clips and steps -- or, on a skip,
leaves parameters and moments alone -- and zeroes the gradients and updates the EMA either way, as the reference does
(ddpm.py:1560-1571).  Nothing waits for the GPU.  The scale is a power of two and the factors are 2 and 0.5 by default, so
every scaling and unscaling is exact and ``(g * inv_scale) * coef`` could as well be multiplied in the other order; with
other ``scaler_kwargs`` factors the order is torch's.  Data parallel: every rank reduces the same gathered bits in rank order,
so ``found_inf`` and the scale are the same on all ranks with nothing new on the wire.

Data.  ``train_step`` and ``fit`` take a list of ``(hr, lr)`` batches, trained on as they are at every step, or a
``dataset.BatchSource`` over a ``DeviceDataset`` -- the reference's ``DataLoader(shuffle=True)`` and augmentation
(ddpm.py:1538-1553): the source is asked for ``batches(self.step)`` at every step, and because its plan is a pure function of
``(seed, step)`` a resumed run and every rank of a data-parallel run see the same global batches.

NOT covered: 16-bit storage, more than one node, ragged shards (a batch size that is no multiple of the world size), a sharded
evaluation (every rank evaluates every test batch), 16-bit gradients on the wire, FID, writing the kernel-layout weight copies from the optimiser launch
(the modules repack after a step, as they do under ``torch.optim.Adam``), handing padded tensors between modules.
"""
import ctypes as C
import math
import os

import torch

from . import _cabi as cabi
from . import checkpoint
from .dataset import BatchSource
from .trainable import (AMP_ATTN_TYPES, SWITCHES, check_amp_attn_precision, check_amp_precision, check_storage_precision, check_switch,
                        stream)
from .unet_grad import TrainableUnet

# the parameters the reference's forward never uses (ddpm.py:437: conv_fusion is called without a time embedding)
NO_GRAD_PARAMS = ("conv_fusion.mlp.1.weight", "conv_fusion.mlp.1.bias")
EMA_KEEP, EMA_COPY, EMA_LERP = 0, 1, 2


def ema_action(s, *, beta=0.995, update_every=10, update_after_step=100, inv_gamma=1.0, power=2 / 3, min_value=0.0,
               initted=True):
    """What ``ema_pytorch.EMA.update()`` does at its call number ``s`` (the number of calls made before this one):
    ``(mode, decay)`` with mode ``EMA_KEEP`` (nothing), ``EMA_COPY`` (ema = online) or ``EMA_LERP`` (ema.lerp_(online,
    1 - decay)).  ``s % update_every != 0``: nothing.  Else ``s <= update_after_step``: copy.  Else lerp with
    ``decay = clamp(1 - (1 + e / inv_gamma) ** -power, min_value, beta)``, ``e = max(s + 1 - update_after_step - 1, 0)``, and
    ``decay = 0`` for ``e <= 0``; an EMA that was never initialised (``initted`` False) copies first, and a lerp from the copy
    towards the same weights is the copy, so that case is ``EMA_COPY`` (the caller sets ``initted``).  Needs no GPU."""
    if s % update_every != 0:
        return EMA_KEEP, 0.0
    if s <= update_after_step:
        return EMA_COPY, 0.0
    e = max(s + 1 - update_after_step - 1, 0)
    decay = 0.0 if e <= 0 else min(max(1.0 - (1.0 + e / inv_gamma) ** -power, min_value), beta)
    return (EMA_LERP if initted else EMA_COPY), decay


def online_kwargs(model):
    """The ``TrainableUnet`` constructor arguments that rebuild ``model`` (an ``ldh.Unet``)."""
    cfg = model.cfg
    return dict(dim=cfg.dim, init_dim=cfg.init_dim, out_dim=cfg.out_dim, dim_mults=tuple(cfg.dim_mults), channels=cfg.channels,
                self_condition=bool(model.self_condition), cond_img=model.cond_img, resnet_block_groups=cfg.resnet_block_groups,
                learned_sinusoidal_cond=bool(model.random_or_learned_sinusoidal_cond), learned_sinusoidal_dim=cfg.learned_sinusoidal_dim,
                sinusoidal_pos_emb_theta=model.theta, attn_dim_head=cfg.attn_dim_head, attn_heads=cfg.attn_heads,
                full_attn=tuple(cfg.full_attn), mode=cfg.mode)


SCALER_DEFAULTS = dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)   # GradScaler's
SCALER_KEYS = ("scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker")           # its state_dict()
MIXED_PRECISION_TYPES = ("fp16", "bf16")


def check_scaler_kwargs(kw):
    """``SCALER_DEFAULTS`` overridden by ``kw`` (None: nothing), validated: ``init_scale`` a positive power of two (every
    scaling is then exact), ``growth_factor`` > 1, 0 < ``backoff_factor`` < 1, ``growth_interval`` an int >= 1.  Needs no GPU."""
    kw = dict(kw or {})
    unknown = sorted(set(kw) - set(SCALER_DEFAULTS))
    if unknown:
        raise ValueError(f"DenoiserTrainer: scaler_kwargs {unknown} are not among {sorted(SCALER_DEFAULTS)}")
    out = {**SCALER_DEFAULTS, **kw}
    for k in ("init_scale", "growth_factor", "backoff_factor"):
        v = out[k]
        if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v):
            raise ValueError(f"DenoiserTrainer: scaler_kwargs {k} = {v!r} must be a finite number")
        out[k] = float(v)
    s = out["init_scale"]
    if s <= 0 or math.frexp(s)[0] != 0.5 or s > 2.0 ** 127 or s < 2.0 ** -126:
        raise ValueError(f"DenoiserTrainer: scaler_kwargs init_scale = {s!r} must be a positive power of two (an fp32 normal)")
    if not out["growth_factor"] > 1.0:
        raise ValueError(f"DenoiserTrainer: scaler_kwargs growth_factor = {out['growth_factor']!r} must be greater than 1")
    if not 0.0 < out["backoff_factor"] < 1.0:
        raise ValueError(f"DenoiserTrainer: scaler_kwargs backoff_factor = {out['backoff_factor']!r} must lie in (0, 1)")
    g = out["growth_interval"]
    if not isinstance(g, int) or isinstance(g, bool) or g < 1:
        raise ValueError(f"DenoiserTrainer: scaler_kwargs growth_interval = {g!r} must be an int of at least 1")
    return out


def check_amp(amp, mixed_precision_type, conv_precision, scaler_kwargs):
    """What ``DenoiserTrainer(amp=, mixed_precision_type=, conv_precision=, scaler_kwargs=)`` means: ``(amp mode of the
    modules, conv_precision, scaler settings or None)``.  ``conv_precision`` None is "not given".  Needs no GPU."""
    if not isinstance(amp, bool):
        raise ValueError(f"DenoiserTrainer: amp = {amp!r} must be True or False")
    if not isinstance(mixed_precision_type, str) or mixed_precision_type not in MIXED_PRECISION_TYPES:
        raise ValueError(f"DenoiserTrainer: mixed_precision_type {mixed_precision_type!r} is not one of "
                         f"{', '.join(repr(v) for v in MIXED_PRECISION_TYPES)}")
    if not amp:
        if scaler_kwargs is not None:
            raise ValueError("DenoiserTrainer: scaler_kwargs without amp=True (there is no loss scaler)")
        return "no", "fp32" if conv_precision is None else conv_precision, None
    if mixed_precision_type == "bf16":
        if conv_precision not in (None, "bf16"):
            raise ValueError(f"DenoiserTrainer: amp=True with mixed_precision_type 'bf16' is conv_precision 'bf16'; "
                             f"conv_precision {conv_precision!r} contradicts it")
        if scaler_kwargs is not None:
            raise ValueError("DenoiserTrainer: scaler_kwargs with mixed_precision_type 'bf16' (bf16 has fp32's range: no loss scaler)")
        return "no", "bf16", None
    conv_precision = "fp32" if conv_precision is None else conv_precision
    check_amp_precision("DenoiserTrainer", "fp16", conv_precision)
    return "fp16", conv_precision, check_scaler_kwargs(scaler_kwargs)


def check_amp_attn(amp_attn, module_amp, attn_precision, full_attn_precision):
    """What ``DenoiserTrainer(amp_attn=)`` needs: a value of ``AMP_ATTN_TYPES``; at ``"fp16"`` a loss scaler (``module_amp``
    ``"fp16"``: ``amp=True`` with ``mixed_precision_type="fp16"``) and neither bf16 attention switch.  Needs no GPU."""
    check_switch("DenoiserTrainer", "amp_attn", amp_attn, AMP_ATTN_TYPES)
    if amp_attn == "fp16" and module_amp != "fp16":
        raise ValueError("DenoiserTrainer: amp_attn 'fp16' needs amp=True with mixed_precision_type 'fp16' (fp16 gradients in "
                         "the attention cores need the loss scaler, and there is none)")
    check_amp_attn_precision("DenoiserTrainer", amp_attn, "attn_precision", attn_precision)
    check_amp_attn_precision("DenoiserTrainer", amp_attn, "full_attn_precision", full_attn_precision)
    return amp_attn


def checkpoint_dict(step, diffusion_sd, online_sd, ema_sd, moments, opt_step, lr, betas, eps, ema_step, initted, scaler=None):
    """The dictionary ``Trainer.save`` writes (ddpm.py:1495-1507), from CPU tensors.  ``diffusion_sd``: the
    ``GaussianDiffusion.state_dict()`` (its ``model.*`` entries give the key order and are replaced); ``online_sd`` / ``ema_sd``:
    the online and the EMA weights by the Unet's names, in the order of ``parameters()``; ``moments``: {name: (exp_avg,
    exp_avg_sq)} of the parameters that have them.  ``model`` = the buffers + ``model.<online>``; ``ema`` = the same under
    ``online_model.``, the buffers + ``model.<ema>`` under ``ema_model.``, ``initted`` and ``step``; ``opt`` = a
    ``torch.optim.Adam.state_dict()`` whose ``state[i]`` exists for the parameters with moments and whose ``step`` is
    ``opt_step`` -- Adam's own count, which under a loss scaler is the number of steps that were not skipped and can be below
    ``step``.  ``scaler``: None (no amp; the reference writes None too) or ``GradScaler.state_dict()``'s five keys
    (``SCALER_KEYS``), written under ``'scaler'`` as plain numbers (ddpm.py:1504)."""
    if scaler is not None:
        if set(scaler) != set(SCALER_KEYS):
            raise ValueError(f"checkpoint_dict: scaler must have the keys {SCALER_KEYS}, not {sorted(scaler)}")
        scaler = {"scale": float(scaler["scale"]), "growth_factor": float(scaler["growth_factor"]),
                  "backoff_factor": float(scaler["backoff_factor"]), "growth_interval": int(scaler["growth_interval"]),
                  "_growth_tracker": int(scaler["_growth_tracker"])}
        if not 0 <= int(opt_step) <= int(step):
            raise ValueError(f"checkpoint_dict: Adam's step count {opt_step} is not within the trainer's {step} steps")
    def with_weights(w):
        return {k: (w[k[6:]] if k.startswith("model.") else v).detach().cpu().clone() for k, v in diffusion_sd.items()}
    missing = [k for k in diffusion_sd if k.startswith("model.") and k[6:] not in online_sd]
    if missing or len(online_sd) != sum(k.startswith("model.") for k in diffusion_sd) or list(online_sd) != list(ema_sd):
        raise ValueError(f"checkpoint_dict: the online / EMA weights do not match the diffusion's model (e.g. {missing[:3]})")
    model = with_weights(online_sd)
    ema = {"online_model." + k: v for k, v in model.items()}
    ema.update({"ema_model." + k: v for k, v in with_weights(ema_sd).items()})
    ema["initted"] = torch.tensor(bool(initted))
    ema["step"] = torch.tensor(int(ema_step))
    state = {}
    for i, name in enumerate(online_sd):
        if name in moments:
            m, v = moments[name]
            state[i] = {"step": torch.tensor(float(opt_step)), "exp_avg": m.detach().cpu().clone(),
                        "exp_avg_sq": v.detach().cpu().clone()}
    opt = {"state": state, "param_groups": checkpoint.adam_param_groups(len(online_sd), lr, betas, eps)}
    return {"step": int(step), "model": model, "opt": opt, "ema": ema, "scaler": scaler}


def shard_rows(n_rows, world, rank):
    """The rows ``[lo, hi)`` of a global batch of ``n_rows`` that ``rank`` of ``world`` trains on (``dist.shard_bounds``).
    ``ValueError`` when the shards would be ragged: their losses would need per-rank weights.  Needs no GPU."""
    from .dist import shard_bounds
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"DenoiserTrainer: rank {rank} of a world of {world}")
    if n_rows < world or n_rows % world:
        raise ValueError(f"DenoiserTrainer: a batch of {n_rows} does not split evenly over {world} ranks (ragged shards are "
                         "not built)")
    return shard_bounds(n_rows, world, rank)


class EmulatedRank:
    """``comm=EmulatedRank(world, rank)``: a rank whose peers live in the same process -- it has no collective, so its
    trainer's ``apply`` needs ``gathered=`` (tests; comparing world sizes on one GPU)."""

    def __init__(self, world, rank):
        self.world, self.rank = int(world), int(rank)

    def all_gather(self, send, recv):
        raise RuntimeError("EmulatedRank has no collective: pass apply(gathered=...)")


def sharded_eval_loss(gathered, sizes, world):
    """The host half of ``DenoiserTrainer.evaluate(sharded=True)``; needs no GPU.  ``gathered``: ``[world, rows, 2]`` float64
    (numpy), copy ``r`` being rank ``r``'s table of per-row ``(sse, n_elem)`` over the rows of all test batches; ``sizes``: the
    batches' row counts.  Each row's pair is read from the copy of the rank that owns the row (``dist.patch_owner`` of its
    index in its batch) -- whatever another copy holds there is ignored and nothing is added across ranks; per batch the
    rows' sums are added in row order and divided by the element count; the result is the mean over the batches in batch
    order.  All in fp64, in one order: every rank gets the same Python float."""
    from .dist import patch_owner
    sizes = [int(n) for n in sizes]
    if not sizes or min(sizes) < 1:
        raise ValueError(f"sharded_eval_loss: batch sizes {sizes}")
    if getattr(gathered, "ndim", 0) != 3 or tuple(gathered.shape) != (world, sum(sizes), 2) or str(gathered.dtype) != "float64":
        raise ValueError(f"sharded_eval_loss: gathered must be float64 [{world}, {sum(sizes)}, 2], got "
                         f"{getattr(gathered, 'dtype', None)} {tuple(getattr(gathered, 'shape', ()))}")
    total, at = 0.0, 0
    for size in sizes:
        sse, count = 0.0, 0.0
        for i in range(size):
            owner = patch_owner(i, size, world)
            sse += float(gathered[owner, at + i, 0])
            count += float(gathered[owner, at + i, 1])
        total += sse / count
        at += size
    return total / len(sizes)


def _positive(name, v, zero_ok=False):
    if not isinstance(v, (int, float)) or isinstance(v, bool) or math.isnan(v) or v < 0 or (v == 0 and not zero_ok):
        raise ValueError(f"DenoiserTrainer: {name} = {v!r} must be a {'non-negative' if zero_ok else 'positive'} number")


class DenoiserTrainer:
    """``DenoiserTrainer(diffusion, *, train_lr=1e-4, adam_betas=(0.9, 0.99), eps=1e-8, max_grad_norm=1.0, ema_decay=0.995,
    ema_update_every=10, ema_update_after_step=100, ema_inv_gamma=1.0, ema_power=2/3, ema_min_value=0.0)``: the defaults are
    the reference's (ddpm.py:1261-1265, 1444, 1449 and ``ema_pytorch``'s).  Refused with ``ValueError`` before any GPU call:
    what ``TrainableUnet`` refuses, ``self_condition``, hyper-parameters out of range, a ``diffusion`` that is not on a GPU.

    ``group`` (a torch process group, or ``"default"`` for the default one) or ``comm`` (an ``LdComm``) makes it one rank of
    a data-parallel run (the module docstring); giving both is refused.  ``world`` and ``rank`` say which; with neither
    (``world`` 1, ``data_parallel`` False) the trainer issues the launches it always did; a group or communicator of one rank
    runs the data-parallel launches on its one copy, to the same bits.

    ``conv_precision="bf16"`` (default ``"fp32"``) trains with the online model's convolutions, and both of their gradients,
    on the bf16 matrix cores (``TrainableUnet.conv_precision``): operands rounded to bf16, fp32 accumulation, everything in
    memory and everything else fp32, no loss scaling; the step stays reproducible bit for bit.  Checkpoints do not record it
    (the weights are the fp32 masters) and the EMA / inference ``Unet`` is not touched.

    ``act_storage="bf16"`` (default ``"fp32"``; with ``conv_precision="bf16"`` only, refused otherwise) keeps the activations
    that only convolutions read as bf16 (``TrainableUnet.act_storage``): less memory and traffic, the same bits in the loss,
    every gradient and every parameter -- so a data-parallel run needs nothing new and a checkpoint does not record it either.

    ``conv_out_storage="bf16"`` (default ``"fp32"``; with ``conv_precision="bf16"`` only, refused otherwise; independent of
    ``act_storage``) keeps the convolution outputs that a ``ResnetBlock``'s GroupNorms read as bf16
    (``TrainableUnet.conv_out_storage``).  This one rounds values that were not rounded before, so the loss and the gradients
    move, by about what the bf16 convolutions move them; the backward is the exact gradient of the rounded forward, the step
    stays reproducible bit for bit, data-parallel replicas stay identical, and a checkpoint does not record it.

    ``attn_precision="bf16"`` (default ``"fp32"``; independent of ``conv_precision``) runs the attention cores of the online
    model's ``LinearAttention`` modules on the bf16 matrix cores (``TrainableUnet.attn_precision``): operands of the 32 x 32
    products rounded to bf16, fp32 accumulation, every sum in a fixed order, so the step stays reproducible bit for bit and
    data-parallel replicas stay identical.  Checkpoints do not record it.

    ``full_attn_precision="bf16"`` (default ``"fp32"``; independent of the other three) does the same for the online model's
    full-softmax ``Attention`` modules (``TrainableUnet.full_attn_precision``): q, k, v, dO and the computed p and ds rounded
    to bf16 for the products, the softmax and its statistics fp32.  The same guarantees: no loss scaling, a step reproducible
    bit for bit, identical replicas, nothing in a checkpoint, the EMA / inference ``Unet`` not involved.

    ``amp=True`` (default False) with ``mixed_precision_type="fp16"`` (the default; the reference's two arguments and
    defaults, ddpm.py:1269-1284) trains with the convolutions on the fp16 matrix cores (``TrainableUnet.amp``) under a loss
    scaler on the device (the module docstring); ``scaler_kwargs`` overrides ``GradScaler``'s defaults (``SCALER_DEFAULTS``:
    ``init_scale`` a power of two, ``growth_factor``, ``backoff_factor``, ``growth_interval``).  It covers what
    ``conv_precision="bf16"`` covers and leaves fp32 what that leaves fp32 (GroupNorm, RMSNorm, the attention cores, the head,
    the time MLP, everything in memory, the master weights and their gradients); ``conv_precision="bf16"`` with it is
    refused, and with that the storage switches.  ``amp=True`` with ``mixed_precision_type="bf16"`` is
    ``conv_precision="bf16"`` and no scaler (an explicit ``conv_precision="fp32"`` contradicts it: ``ValueError``); any other
    type is a ``ValueError``; ``amp=False`` changes nothing at all.  ``scaler_state()`` reads the scaler back;
    ``check_finite()`` does not raise under a scaler (a non-finite norm is a skipped step there).

    ``amp_attn="fp16"`` (default ``"fp32"``; ``trainable.AMP_ATTN_TYPES``) extends ``amp`` to the attention cores: every
    ``LinearAttention`` and ``Attention`` of the online model runs the passes of its core on the fp16 matrix cores
    (``TrainableUnet.amp_attn``).  It needs ``amp=True`` with ``mixed_precision_type="fp16"`` -- without the scaler it is a
    ``ValueError`` -- and is refused together with ``attn_precision="bf16"`` or ``full_attn_precision="bf16"``.  A dO or dctx
    that overflows fp16 under a large scale is a skipped step and a back-off, like an overflow in a convolution.  The step
    stays reproducible bit for bit, replicas stay identical, and a checkpoint does not record it; ``amp_attn="fp32"`` spelled
    out is leaving it out.

    ``step`` counts ``apply()`` calls (the reference's ``Trainer.step``, and without a scaler Adam's step count; with one,
    Adam's count lives on the device and does not advance on a skipped step); ``ema_step`` and ``ema_initted`` are
    ``ema_pytorch``'s two buffers and advance at every call."""

    def __init__(self, diffusion, *, train_lr=1e-4, adam_betas=(0.9, 0.99), eps=1e-8, max_grad_norm=1.0, ema_decay=0.995,
                 ema_update_every=10, ema_update_after_step=100, ema_inv_gamma=1.0, ema_power=2 / 3, ema_min_value=0.0, group=None, comm=None,
                 conv_precision=None, act_storage="fp32", conv_out_storage="fp32", attn_precision="fp32",
                 full_attn_precision="fp32", amp=False, mixed_precision_type="fp16", scaler_kwargs=None,
                 amp_attn="fp32"):
        if conv_precision is not None:
            check_switch("DenoiserTrainer", "conv_precision", conv_precision)
        module_amp, conv_precision, scaler = check_amp(amp, mixed_precision_type, conv_precision, scaler_kwargs)
        switches = dict(conv_precision=conv_precision, act_storage=act_storage, conv_out_storage=conv_out_storage,
                        attn_precision=attn_precision, full_attn_precision=full_attn_precision)
        for switch in SWITCHES:
            check_switch("DenoiserTrainer", switch, switches[switch])
        for switch in ("act_storage", "conv_out_storage"):
            check_storage_precision("DenoiserTrainer", switch, switches[switch], conv_precision)
        check_amp_attn(amp_attn, module_amp, attn_precision, full_attn_precision)
        if group is not None and comm is not None:
            raise ValueError("DenoiserTrainer: give a torch process group or an LdComm, not both")
        model = getattr(diffusion, "model", None)
        if model is None or not hasattr(model, "cfg") or not hasattr(diffusion, "p_losses_grad"):
            raise ValueError("DenoiserTrainer: diffusion must be an ldh.GaussianDiffusion around an ldh.Unet")
        if getattr(diffusion, "self_condition", False) or getattr(model, "self_condition", False):
            raise ValueError("DenoiserTrainer: self_condition is not built for training (no shipped caller of the reference sets it)")
        _positive("train_lr", train_lr)
        _positive("eps", eps, zero_ok=True)
        _positive("max_grad_norm", max_grad_norm, zero_ok=True)
        _positive("ema_inv_gamma", ema_inv_gamma)
        _positive("ema_power", ema_power, zero_ok=True)
        betas = tuple(adam_betas)
        if len(betas) != 2 or not all(isinstance(b, float) and 0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"DenoiserTrainer: adam_betas {adam_betas!r} must be two floats in [0, 1)")
        if not (0.0 <= ema_min_value <= ema_decay <= 1.0):
            raise ValueError(f"DenoiserTrainer: 0 <= ema_min_value {ema_min_value} <= ema_decay {ema_decay} <= 1 does not hold")
        for name, v, lo in (("ema_update_every", ema_update_every, 1), ("ema_update_after_step", ema_update_after_step, 0)):
            if not isinstance(v, int) or isinstance(v, bool) or v < lo:
                raise ValueError(f"DenoiserTrainer: {name} = {v!r} must be an int of at least {lo}")
        # (raises ValueError for what it cannot train)
        online = TrainableUnet(**online_kwargs(model), **switches, amp=module_amp, amp_attn=amp_attn)
        vars(self).update(switches)                   # (what the trainer was built with: self.conv_precision and so on)
        self.amp_attn = amp_attn
        self.amp, self.mixed_precision_type, self.scaler = bool(amp), mixed_precision_type, scaler     # scaler: settings or None
        dev = diffusion.device
        if dev.type != "cuda":
            raise ValueError(f"DenoiserTrainer: diffusion is on {dev}; the trainer runs on HIP kernels only (there is no CPU path)")
        self.diffusion, self.device = diffusion, dev
        self.lr, self.betas, self.eps, self.max_grad_norm = float(train_lr), betas, float(eps), float(max_grad_norm)
        self.ema_kw = dict(beta=float(ema_decay), update_every=ema_update_every, update_after_step=ema_update_after_step,
                           inv_gamma=float(ema_inv_gamma), power=float(ema_power), min_value=float(ema_min_value))
        self.step, self.ema_step, self.ema_initted, self.last_ema = 0, 0, False, None
        self.group, self.comm, self.world, self.rank, self.staged_gather = None, comm, 1, 0, False
        if comm is not None:
            self.world, self.rank = int(comm.world), int(comm.rank)
        elif group is not None:
            import torch.distributed as tdist
            if not (tdist.is_available() and tdist.is_initialized()):
                raise ValueError("DenoiserTrainer: group given but torch.distributed is not initialised")
            self.group = tdist.group.WORLD if isinstance(group, str) and group == "default" else group
            self.world, self.rank = tdist.get_world_size(self.group), tdist.get_rank(self.group)
            # gloo (the test-only mode of several ranks on one GPU) gathers host tensors: the exchange is staged through
            # pinned host memory and waits for the GPU -- a functional path, never a measurement
            self.staged_gather = tdist.get_backend(self.group) == "gloo"
        self.data_parallel = comm is not None or group is not None       # (also at world 1: the same launches, one copy)
        if not 1 <= self.world <= cabi.DN_OPT_MAX_WORLD or not 0 <= self.rank < self.world:
            raise ValueError(f"DenoiserTrainer: rank {self.rank} of a world of {self.world} (1..{cabi.DN_OPT_MAX_WORLD})")
        online.load_state_dict(model.state_dict())
        self.online_model = online.to(dev)
        self._build_table()

    # ------------------------------------------------------------------ the table and the flat buffers
    def _build_table(self):
        dev, lib = self.device, cabi.lib()
        named = list(self.online_model.named_parameters())
        self.names = [k for k, _ in named]
        n = len(named)
        host = (cabi.DnOptTensor * n)()
        for e, (k, p) in zip(host, named):
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"DenoiserTrainer: parameter {k} is {p.dtype}, contiguous {p.is_contiguous()}; fp32 contiguous only")
            e.param, e.count, e.flags = p.data_ptr(), p.numel(), (0 if k in NO_GRAD_PARAMS else cabi.DN_OPT_ADAM)
        flat, wgs = cabi.i64(), cabi.i64()
        cabi.check(lib.ld_dn_opt_layout(host, n, C.byref(flat), C.byref(wgs)), "dn_opt_layout")
        self._n, self._n_wg, self._flat = n, int(wgs.value), int(flat.value)
        self._segments = {k: (int(e.offset), int(e.count), bool(e.flags & cabi.DN_OPT_ADAM)) for e, (k, _) in zip(host, named)}
        self._ptrs = [int(e.param) for e in host]
        self._views = self._params = None
        with torch.cuda.device(dev):
            self._table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
            self._m, self._v, self._ema = (torch.zeros(self._flat, dtype=torch.float32, device=dev) for _ in range(3))
            # what a rank sends: the flat gradient and four more floats, the first of which is its summed loss
            self._send = torch.zeros(self._flat + 4, dtype=torch.float32, device=dev)
            self._grad, self._loss_slot = self._send[:self._flat], self._send[self._flat:]
            self._gathered = self._loss = None
            if self.data_parallel:
                self._loss = torch.zeros(1, dtype=torch.float32, device=dev)
                if not isinstance(self.comm, EmulatedRank):
                    self._gathered = torch.empty(self.world, self._flat + 4, dtype=torch.float32, device=dev)
                if self.staged_gather:
                    self._host_send = torch.empty(self._flat + 4, dtype=torch.float32).pin_memory()
                    self._host_recv = torch.empty(self.world, self._flat + 4, dtype=torch.float32).pin_memory()
            self._work = torch.zeros(1 + int(lib.ld_dn_opt_sqnorm_work_bytes(self._n_wg)) // 8, dtype=torch.float64, device=dev)
            self._scaler_state = self._scale = None
            if self.scaler is not None:                     # ld_dn_scaler_state: 8 dwords; its first is the scale
                self._scaler_state = torch.zeros(C.sizeof(cabi.DnScalerState) // 4, dtype=torch.int32, device=dev)
                self._scale = self._scaler_state[:1].view(torch.float32)
                self._init_scaler(self.scaler["init_scale"], 0, 0)
        with torch.no_grad():                               # ema_pytorch: the EMA model starts as a copy of the online one
            for k, p in named:
                self._segment(self._ema, k).copy_(p.reshape(-1))
        self._attach_grads()

    def _init_scaler(self, scale, adam_steps, growth_tracker, skipped_steps=0):
        with torch.cuda.device(self.device):
            cabi.check(cabi.lib().ld_dn_scaler_init(self._scaler_state.data_ptr(), float(scale), int(adam_steps),
                                                    int(growth_tracker), stream(self.device)), "dn_scaler_init")
            if skipped_steps:
                self._scaler_state[3].fill_(int(skipped_steps))

    def scaler_state(self):
        """The loss scaler as it stands -- the one call that reads ``ld_dn_scaler_state`` back, so it waits for the GPU:
        ``GradScaler.state_dict()``'s five keys (``SCALER_KEYS``) plus ``adam_steps`` (the optimiser steps that were not
        skipped), ``skipped_steps`` and ``found_inf`` (whether the last step was skipped).  ``RuntimeError`` without amp."""
        if self._scaler_state is None:
            raise RuntimeError("DenoiserTrainer: no loss scaler (amp=True with mixed_precision_type 'fp16' makes one)")
        st = cabi.DnScalerState.from_buffer_copy(self._scaler_state.cpu().numpy().tobytes())
        return {"scale": float(st.scale), "growth_factor": self.scaler["growth_factor"],
                "backoff_factor": self.scaler["backoff_factor"], "growth_interval": self.scaler["growth_interval"],
                "_growth_tracker": int(st.growth_tracker), "adam_steps": int(st.adam_steps),
                "skipped_steps": int(st.skipped_steps), "found_inf": bool(st.found_inf)}

    def _segment(self, flat, name):
        off, count, _ = self._segments[name]
        return flat[off:off + count]

    def _attach_grads(self):
        """Every trained parameter's ``.grad`` is the view of its segment of the flat gradient (a ``.grad`` the caller put
        there instead is added to the segment first); the parameters must still be where the table says.  The views are
        made once: a step only checks identities."""
        if self._views is None:
            named = list(self.online_model.named_parameters())
            self._params = [p for _, p in named]
            self._views = [(k, p, ptr, self._segment(self._grad, k).view(p.shape) if self._segments[k][2] else None)
                           for (k, p), ptr in zip(named, self._ptrs)]
        for k, p, ptr, view in self._views:
            if p.data_ptr() != ptr:
                raise RuntimeError(f"DenoiserTrainer: parameter {k} was moved (.to(), assign); build a new trainer")
            if view is None or p.grad is view:
                continue
            if p.grad is not None and p.grad.data_ptr() != view.data_ptr():
                view.add_(p.grad)
            p.grad = view

    # ------------------------------------------------------------------ one batch, one step
    def accumulate(self, hr, lr, scale=1.0, t=None, noise=None):
        """One batch of ddpm.py:1544-1553: adds the gradients of ``scale`` times the training loss of (``hr``, the image,
        ``lr``, the condition image) to the ``.grad``s and returns ``scale * loss`` as a 0-d device tensor.  ``t`` None: drawn
        as ``GaussianDiffusion.forward(train=True)`` draws it (torch's host generator); ``noise`` None: drawn as ``p_losses``
        draws it (the run's noise stream, the offset noise included).  No host synchronisation.  On a rank of a
        data-parallel run this is the local half: ``hr`` / ``lr`` are the rank's rows, given ``t`` / ``noise`` are taken as they
        are, drawn ones are the rank's rows of the draw for the global batch of ``world`` times as many rows, and the value
        is also added to the loss slot that travels with the gradients."""
        gd, dev, lib = self.diffusion, self.device, cabi.lib()
        if not isinstance(hr, torch.Tensor) or hr.dim() != 4:
            raise ValueError("DenoiserTrainer: hr must be a [B, C, H, W] tensor")
        B = hr.shape[0]
        first_row = self.rank * B                           # of the global batch (equal shards)
        if t is None:
            t = torch.randint(0, gd.num_timesteps, (B * self.world,)).long()[first_row:first_row + B]
        if not t.is_cuda:
            t = t.pin_memory()                              # (a pageable copy would wait for the stream)
        self._attach_grads()
        with torch.cuda.device(dev):
            t = t.to(dev, torch.long, non_blocking=True)
            with torch.no_grad():
                x0 = gd.normalize(hr.to(dev, torch.float32)).contiguous()
                cond = lr.to(dev, torch.float32).contiguous()
                noise = gd.training_noise(x0, noise, first_row=first_row)
                t32 = t.to(torch.int32)
                x = torch.empty_like(x0)
                cabi.check(lib.ld_q_sample_t(x0.data_ptr(), noise.data_ptr(), x.data_ptr(), t32.data_ptr(),
                                             gd.sqrt_alphas_cumprod.data_ptr(), gd.sqrt_one_minus_alphas_cumprod.data_ptr(), B,
                                             x0[0].numel(), stream(dev)), "q_sample_t")
            out = self.online_model(x, cond, t)
            with torch.no_grad():
                per_sample = torch.empty(B, dtype=torch.float32, device=dev)
                cabi.check(lib.ld_p_losses(out.data_ptr(), x0.data_ptr(), noise.data_ptr(), t32.data_ptr(),
                                           gd.sqrt_alphas_cumprod.data_ptr(), gd.sqrt_one_minus_alphas_cumprod.data_ptr(),
                                           gd.loss_weight.data_ptr(), per_sample.data_ptr(), B, x0[0].numel(),
                                           cabi.OBJ[gd.objective], stream(dev)), "p_losses")
                value = per_sample.mean() * float(scale)
            # under amp the upstream scalar is scale * the loss scale, read on the device; ``value`` stays unscaled
            out.backward(gd.p_losses_grad(out, x0, noise, t, grad_output=float(scale), grad_scale=self._scale))
            if self.data_parallel:
                self._loss_slot[0].add_(value)
        return value

    def apply(self, gathered=None):
        """ddpm.py:1558-1571: clip the accumulated gradients to ``max_grad_norm``, Adam, zero the gradients, ``ema.update()``
        -- two launches -- and move every parameter's version so that the modules repack their weights.  Nothing waits.

        ``data_parallel``: one all-gather of the rank's ``flat + 4`` floats, then ``ld_dn_opt_reduce`` (the rank-ordered sum into
        the rank's own gradient and the squared norm; ``ld_dn_opt_sqnorm`` is not launched), the loss tail, and
        ``ld_dn_opt_step`` as ever; returns the step's loss summed over the ranks (a 0-d device tensor, the same bits on every
        rank).  ``gathered``: a ready ``[world, flat + 4]`` fp32 device tensor to use in place of the collective (tests)."""
        dev, lib = self.device, cabi.lib()
        self._attach_grads()
        t = self.step + 1
        b1, b2 = self.betas
        step_size = self.lr / (1.0 - b1 ** t)               # bias corrections in double on the host
        bc2_sqrt = math.sqrt(1.0 - b2 ** t)
        mode, decay = ema_action(self.ema_step, initted=self.ema_initted, **self.ema_kw)
        if self.ema_step % self.ema_kw["update_every"] == 0 and self.ema_step > self.ema_kw["update_after_step"]:
            self.ema_initted = True
        loss = None
        with torch.cuda.device(dev):
            st = stream(dev)
            sumsq = self._work.data_ptr()
            if not self.data_parallel and gathered is None:
                cabi.check(lib.ld_dn_opt_sqnorm(self._table.data_ptr(), self._n, self._n_wg, self._grad.data_ptr(), self._flat,
                                                sumsq + 8, sumsq, st), "dn_opt_sqnorm")
            else:
                stride = self._flat + 4
                if gathered is None:
                    gathered = self._exchange()
                elif not (isinstance(gathered, torch.Tensor) and gathered.dtype == torch.float32 and gathered.is_contiguous()
                          and gathered.device == self._send.device and tuple(gathered.shape) == (self.world, stride)):
                    raise ValueError(f"DenoiserTrainer: gathered must be a contiguous [{self.world}, {stride}] fp32 tensor on "
                                     f"{self._send.device}")
                if self._loss is None:
                    self._loss = torch.zeros(1, dtype=torch.float32, device=dev)
                cabi.check(lib.ld_dn_opt_reduce(self._table.data_ptr(), self._n, self._n_wg, gathered.data_ptr(), self.world,
                                                stride, self._grad.data_ptr(), self._flat, sumsq + 8, sumsq, st), "dn_opt_reduce")
                cabi.check(lib.ld_dn_opt_reduce_tail(gathered.data_ptr(), self.world, stride, self._flat,
                                                     self._loss.data_ptr(), st), "dn_opt_reduce_tail")
                self._loss_slot.zero_()
                loss = self._loss[0].clone()
            if self._scaler_state is not None:
                # sumsq is the squared norm of the SCALED gradients: the update kernel takes the scaler's decisions from it and
                # leaves found_inf, 1 / scale and Adam's bias corrections (for Adam's own count) where the step reads them
                sc, state = self.scaler, self._scaler_state.data_ptr()
                cabi.check(lib.ld_dn_opt_scaler_update(state, sumsq, self.lr, b1, b2, sc["growth_factor"], sc["backoff_factor"],
                                                       sc["growth_interval"], st), "dn_opt_scaler_update")
                cabi.check(lib.ld_dn_opt_step_scaled(self._table.data_ptr(), self._n, self._n_wg, self._grad.data_ptr(),
                                                     self._m.data_ptr(), self._v.data_ptr(), self._ema.data_ptr(), self._flat,
                                                     sumsq, state, self.max_grad_norm, b1, b2, self.eps, mode, 1.0 - decay, st),
                           "dn_opt_step_scaled")
            else:
                cabi.check(lib.ld_dn_opt_step(self._table.data_ptr(), self._n, self._n_wg, self._grad.data_ptr(),
                                              self._m.data_ptr(), self._v.data_ptr(), self._ema.data_ptr(), self._flat, sumsq,
                                              self.max_grad_norm, b1, b2, self.eps, step_size, bc2_sqrt, mode, 1.0 - decay, st),
                           "dn_opt_step")
        # the packed-weight caches are keyed on _version, which a raw kernel write does not move
        torch.autograd.graph.increment_version(self._params)
        self.last_ema = (mode, decay)                       # what the launch was told: (EMA_KEEP / EMA_COPY / EMA_LERP, decay)
        self.step += 1
        self.ema_step += 1
        return loss

    def send_buffer(self):
        """What this rank contributes to the exchange: ``flat + 4`` floats, the flat gradient and the loss slot (a view)."""
        return self._send

    def _exchange(self):
        """The one collective of a step: every rank's send buffer into ``[world, flat + 4]``."""
        with cabi.prof_range("exchange"):
            if self.comm is not None:
                self.comm.all_gather(self._send, self._gathered)
            elif self.staged_gather:                       # gloo: through pinned host memory (waits for the GPU; test-only)
                import torch.distributed as tdist
                self._host_send.copy_(self._send)
                tdist.all_gather_into_tensor(self._host_recv.view(-1), self._host_send, group=self.group)
                self._gathered.copy_(self._host_recv)
            else:
                import torch.distributed as tdist
                tdist.all_gather_into_tensor(self._gathered.view(-1), self._send, group=self.group)
        return self._gathered

    def train_step(self, batches, t=None, noise=None):
        """The reference's step: ``accumulate(hr, lr, scale=1 / len(batches))`` over all ``(hr, lr)`` batches, ``apply()``;
        returns the summed loss (the reference's ``total_loss``) on the device.  ``data_parallel`` (``split_batches=True``):
        every rank is handed the same global batches and takes its rows of each, the scale is ``1 / (world * len(batches))``
        and the loss is the sum over the ranks; a batch size that is no multiple of ``world`` is a ``ValueError``.

        ``batches``: a list of ``(hr, lr)``, or a ``dataset.BatchSource``, which is asked for ``batches(self.step)`` -- the
        DataLoader's fresh shuffle and augmentation at every step -- and walked lazily: batch k + 1 is made after batch k has
        been accumulated, and ``len()`` needs no batch.  ``t`` / ``noise``: None (drawn, as ``accumulate`` draws them) or one
        entry per batch for the GLOBAL batch (a rank takes its rows)."""
        if isinstance(batches, BatchSource):
            batches = batches.batches(self.step)
            sizes = list(batches.sizes)
        else:
            batches = list(batches)
            sizes = [int(hr.shape[0]) for hr, _ in batches]
        n = len(batches)
        if not n:
            raise ValueError("DenoiserTrainer: no batches")
        for name, given in (("t", t), ("noise", noise)):
            if given is not None and len(given) != n:
                raise ValueError(f"DenoiserTrainer: {n} batches need {n} entries of {name}, got {len(given)}")
        t = [None] * n if t is None else list(t)
        noise = [None] * n if noise is None else list(noise)
        if self.data_parallel:
            rows = [shard_rows(size, self.world, self.rank) for size in sizes]      # (before any GPU call)
            for (hr, lr), (lo, hi), tk, nk in zip(batches, rows, t, noise):
                self.accumulate(hr[lo:hi], lr[lo:hi], scale=1.0 / (self.world * n), t=None if tk is None else tk[lo:hi],
                                noise=None if nk is None else nk[lo:hi])
            return self.apply()
        total = None
        for (hr, lr), tk, nk in zip(batches, t, noise):
            value = self.accumulate(hr, lr, scale=1.0 / n, t=tk, noise=nk)
            total = value if total is None else total + value
        self.apply()
        return total

    def replica_digest(self):
        """A debugging call that waits for the GPU: ``(sumsq, weight sum, weight xor)`` -- the last step's squared gradient
        norm, the fp64 sum of the online weights and the xor of their bit patterns -- gathered from every rank;
        ``RuntimeError`` naming the first rank whose numbers are not rank 0's, else the digest."""
        import numpy as np
        with torch.no_grad():
            w = torch.cat([p.detach().reshape(-1) for p in self.online_model.parameters()]).cpu().numpy()
            mine = np.array([float(self._work[0].item()) if self.step else 0.0, np.sum(w, dtype=np.float64),
                             float(np.bitwise_xor.reduce(w.view(np.uint32)))], dtype=np.float64)
            every = torch.from_numpy(mine.view(np.int64).copy())[None]            # bit patterns: a NaN compares like any value
            if self.world > 1 and not isinstance(self.comm, EmulatedRank):
                recv = torch.empty(self.world, 3, dtype=torch.int64, device=self.device)
                if self.comm is not None:
                    with torch.cuda.device(self.device):
                        self.comm.all_gather(every[0].to(self.device), recv)
                else:
                    import torch.distributed as tdist
                    if self.staged_gather:
                        recv = recv.cpu()
                    tdist.all_gather_into_tensor(recv.view(-1), every[0].to(recv.device), group=self.group)
                every = recv.cpu()
        for r in range(every.shape[0]):
            if not torch.equal(every[r], every[0]):
                got, want = every[r].numpy().view(np.float64), every[0].numpy().view(np.float64)
                raise RuntimeError(f"DenoiserTrainer: rank {r} differs from rank 0 after step {self.step}: (sumsq, weight sum, "
                                   f"weight xor) = {got.tolist()} against {want.tolist()}")
        return dict(step=self.step, sumsq=float(mine[0]), weight_sum=float(mine[1]), weight_xor=int(mine[2]))

    def check_finite(self):
        """Read the last step's gradient norm back (the one place that does) and raise on a non-finite value; returns it.
        Under a loss scaler it is the norm of the SCALED gradients, and a non-finite one is a skipped step, not an error: it is
        returned (``inf`` / ``nan``) without raising."""
        sumsq = float(self._work[0].item()) if self.step else 0.0
        norm = math.sqrt(sumsq) if sumsq >= 0.0 else sumsq          # (a NaN or a negative garbage value stays what it is)
        if not math.isfinite(norm) and self._scaler_state is None:
            raise FloatingPointError(f"DenoiserTrainer: the gradient norm of step {self.step} is {norm}; the weights and moments "
                                     "took the step as torch would have (they hold NaN now)")
        return norm

    # ------------------------------------------------------------------ state
    def _named(self, flat):
        return {k: self._segment(flat, k).view(p.shape).clone() for k, p in self.online_model.named_parameters()}

    def ema_state_dict(self):
        """The EMA weights by the Unet's names (copies, on the device)."""
        return self._named(self._ema)

    def moments(self):
        """{name: (exp_avg, exp_avg_sq)} of the parameters that have them (copies, on the device)."""
        m, v = self._named(self._m), self._named(self._v)
        return {k: (m[k], v[k]) for k in self.names if self._segments[k][2]}

    def sync_ema(self):
        """Load the EMA weights into ``diffusion.model`` (the reference's ``ema.ema_model``) for sampling and evaluation."""
        self.diffusion.model.load_state_dict(self.ema_state_dict())          # (``Unet.load_state_dict`` invalidates its plans)

    @torch.no_grad()
    def evaluate(self, batches, min_max_val, sharded=False, gathered=None):
        """ddpm.py:1574-1587: sample every ``(hr, lr)`` test batch from ``lr`` with the EMA weights and return the mean over
        the batches of the mean squared error to ``hr``.

        ``sharded=True``: rank ``r`` samples only rows ``dist.shard_bounds(B_k, world, r)`` of test batch ``k``
        (``evaluate_local``), ONE all-gather over the path ``_exchange`` uses leaves every rank's fp64 table of per-row
        ``(sse, n_elem)`` on every rank, and every rank computes ``sharded_eval_loss`` of it on the host: each row's value from
        its owner's copy, nothing added across ranks, so every rank returns the same Python float and takes the same "new
        best" decision.  The squared errors are summed in fp64 (``ld_metric_sums``) where the unsharded path takes fp32
        ``mse_loss``, so the two agree to fp32's summation error, not bit for bit.  ``gathered``: a ready
        ``[world, rows, 2]`` fp64 tensor in place of the collective (an ``EmulatedRank`` needs it).  At world 1 the same path
        runs on one rank."""
        if sharded:
            batches = list(batches)
            send = self.evaluate_local(batches, min_max_val)
            sizes = [int(hr.shape[0]) for hr, _ in batches]
            if gathered is None:
                gathered = self._exchange_eval(send)
            elif not (isinstance(gathered, torch.Tensor) and gathered.dtype == torch.float64
                      and tuple(gathered.shape) == (self.world,) + tuple(send.shape)):
                raise ValueError(f"DenoiserTrainer: gathered must be a [{self.world}, {send.shape[0]}, 2] fp64 tensor")
            return sharded_eval_loss(gathered.cpu().numpy(), sizes, self.world)          # (the evaluation's one wait)
        if gathered is not None:
            raise ValueError("DenoiserTrainer: gathered is an argument of evaluate(sharded=True)")
        self.sync_ema()
        losses = []
        for hr, lr in batches:
            lr = lr.to(self.device, torch.float32)
            out = self.diffusion.sample(lr, None, batch_size=lr.shape[0], mask=None, min_max_val=min_max_val)
            losses.append(float(torch.nn.functional.mse_loss(out, hr.to(self.device, torch.float32))))
        if not losses:
            raise ValueError("DenoiserTrainer: no test batches")
        return sum(losses) / len(losses)

    @torch.no_grad()
    def evaluate_local(self, batches, min_max_val):
        """The part of ``evaluate(sharded=True)`` in front of the collective: sample this rank's rows of every test batch
        (``dist._sample_shard``: the noise stream stands at the shard's first row, so a row is what the whole batch would have
        made of it; a rank without rows in a batch calls ``dist._idle_rank_advances``), ``ld_metric_sums`` on them, and the
        whole-image ``(sse, n_elem)`` of each row into its slot of one fp64 ``[rows of all batches, 2]`` table on the device,
        zeros elsewhere.  Returns that table, the rank's send buffer.  The metric launches and the table writes do not wait for
        the GPU: the call waits no more than ``sync_ema`` and ``sample`` do."""
        from . import dist
        from .metrics import quality_sums
        batches = list(batches)
        if not batches:
            raise ValueError("DenoiserTrainer: no test batches")
        self.sync_ema()
        sizes = [int(hr.shape[0]) for hr, _ in batches]
        table = torch.zeros(sum(sizes), 2, dtype=torch.float64, device=self.device)
        at = 0
        for (hr, lr), size in zip(batches, sizes):
            lo, hi = dist.shard_bounds(size, self.world, self.rank)
            if hi > lo:
                cond = lr[lo:hi].to(self.device, torch.float32)
                out = dist._sample_shard(self.diffusion, lo, hi, hr[0].numel(), lambda: self.diffusion.sample(
                    cond, None, batch_size=hi - lo, mask=None, min_max_val=min_max_val))
                # (data_range only enters the SSIM fields, which this table does not take)
                sums = quality_sums(out.to(torch.float32), hr[lo:hi].to(self.device, torch.float32), None, data_range=1.0)
                table[at + lo:at + hi, 0] = sums[:, 0, 1]
                table[at + lo:at + hi, 1] = sums[:, 0, 0]
            else:
                dist._idle_rank_advances(self.diffusion, None)
            at += size
        return table

    def _exchange_eval(self, send):
        """The sharded evaluation's one collective: every rank's table into ``[world, rows, 2]``, over ``_exchange``'s path."""
        if not self.data_parallel:
            return send[None]
        if isinstance(self.comm, EmulatedRank):
            raise RuntimeError("EmulatedRank has no collective: pass evaluate(sharded=True, gathered=...)")
        recv = torch.empty((self.world,) + tuple(send.shape), dtype=send.dtype, device=send.device)
        with cabi.prof_range("exchange"):
            if self.comm is not None:
                with torch.cuda.device(self.device):
                    self.comm.all_gather(send, recv)
            elif self.staged_gather:                       # gloo: host tensors (waits for the GPU; test-only)
                import torch.distributed as tdist
                host = torch.empty(recv.shape, dtype=recv.dtype)
                tdist.all_gather_into_tensor(host.view(-1), send.cpu().view(-1), group=self.group)
                recv = host
            else:
                import torch.distributed as tdist
                tdist.all_gather_into_tensor(recv.view(-1), send.view(-1), group=self.group)
        return recv

    def state(self):
        """``checkpoint_dict``'s result for this trainer (CPU tensors)."""
        cpu = lambda d: {k: v.detach().cpu() for k, v in d.items()}                        # noqa: E731
        moments = {k: (m.cpu(), v.cpu()) for k, (m, v) in self.moments().items()}
        online = {k: p for k, p in self.online_model.named_parameters()}
        opt_step, scaler = self.step, None
        if self._scaler_state is not None:
            full = self.scaler_state()
            opt_step, scaler = full["adam_steps"], {k: full[k] for k in SCALER_KEYS}
        return checkpoint_dict(self.step, cpu(self.diffusion.state_dict()), cpu(online), cpu(self.ema_state_dict()), moments,
                               opt_step, self.lr, self.betas, self.eps, self.ema_step, self.ema_initted, scaler=scaler)

    def save(self, path):
        """Write the reference's ``Trainer.save`` file (``checkpoint.load_reference_checkpoint`` and the reference's own
        ``Trainer.load`` read it)."""
        torch.save(self.state(), path)

    def load(self, path, trust_pickle=False):
        """Restore what ``save`` wrote (or the reference's ``Trainer.save``): the EMA weights into ``diffusion`` and the EMA
        buffer, the online weights, both moments, Adam's step count and the counters.  A trainer with a loss scaler takes
        ``scale`` and ``_growth_tracker`` from the file's ``'scaler'`` when it has them (else it keeps its own scale) and
        accepts an Adam step count below ``step`` (steps were skipped); one without ignores ``'scaler'``, as the reference
        does (ddpm.py:1526-1527), and keeps the check that the two counts are equal."""
        data = checkpoint._read(path, trust_pickle)
        info = checkpoint.load_reference_checkpoint(data, self.diffusion, use_ema=True)
        if info["source"] != "ema":
            raise RuntimeError(f"DenoiserTrainer.load: the file has no EMA weights (found {info['source']!r})")
        online = {k[6:]: v for k, v in data["model"].items() if k.startswith("model.")}
        self.online_model.load_state_dict(online)                     # (in place: the table's pointers stay good)
        ema = {k[len("ema_model.model."):]: v for k, v in data["ema"].items() if k.startswith("ema_model.model.")}
        state = data["opt"]["state"]
        with torch.no_grad():
            self._m.zero_()
            self._v.zero_()
            self._grad.zero_()
            for i, k in enumerate(self.names):
                self._segment(self._ema, k).copy_(ema[k].reshape(-1))
                if i in state:
                    if not self._segments[k][2]:
                        raise RuntimeError(f"DenoiserTrainer.load: the file has Adam moments for {k}, which gets no gradient")
                    self._segment(self._m, k).copy_(state[i]["exp_avg"].reshape(-1))
                    self._segment(self._v, k).copy_(state[i]["exp_avg_sq"].reshape(-1))
        steps = {int(float(s["step"])) for s in state.values()}
        if len(steps) > 1:
            raise RuntimeError(f"DenoiserTrainer.load: the parameters' Adam step counts differ ({sorted(steps)[:4]})")
        self.step = int(data["step"])
        if self._scaler_state is not None:
            adam_steps = min(steps) if steps else self.step
            if not 0 <= adam_steps <= self.step:
                raise RuntimeError(f"DenoiserTrainer.load: Adam's step count {adam_steps} is not within the trainer's step {self.step}")
            saved = data.get("scaler") or {}
            if "scale" in saved and "_growth_tracker" in saved:
                scale, tracker = float(saved["scale"]), int(saved["_growth_tracker"])
            else:
                scale, tracker = self.scaler_state()["scale"], 0
            self._init_scaler(scale, adam_steps, tracker, skipped_steps=self.step - adam_steps)
        elif steps and steps != {self.step}:
            raise RuntimeError(f"DenoiserTrainer.load: Adam's step count {steps} is not the trainer's step {self.step}")
        self.ema_step, self.ema_initted = int(data["ema"]["step"]), bool(data["ema"]["initted"])
        self._attach_grads()
        return info

    # ------------------------------------------------------------------ the loop
    def fit(self, batches, test_batches, num_steps, save_and_sample_every, out_dir, min_max_val=None, sharded_eval=False):
        """``Trainer.train`` (ddpm.py:1532-1606) until ``step == num_steps``: ``train_step(batches)`` (a list, trained on as it is
        at every step, or a ``BatchSource``, reshuffled and re-augmented at every step); every
        ``save_and_sample_every`` steps ``evaluate(test_batches)`` and, at a new best, ``save`` to
        ``<out_dir>/model-best<step rounded up to 100 (mnist) or 500>.pt``.  ``train_loss.csv`` and ``loss.csv`` have the
        layout pandas gives the reference's frames (an index column, ``epoch``, ``loss``); ``train_loss.csv`` holds every
        step (the reference appends each step's row to the evaluation frame, so its file keeps only the last one).
        ``min_max_val`` defaults to the reference's per data set (ddpm.py:1474-1489).  Returns the best evaluation loss.
        Data-parallel: by default every rank evaluates every test batch (redundant, but no rank sits in a collective for
        minutes); ``sharded_eval=True`` evaluates with ``evaluate(sharded=True)`` -- every rank samples its rows of each test
        batch and one all-gather of the per-row error sums gives every rank the same float, so the replicas take the same "new
        best" decision (the loss is an fp64 sum there: equal to the default's to fp32's summation error, not bit for bit).
        Only rank 0 writes the files, and ``replica_digest()`` runs at every evaluation point."""
        data = str(self.diffusion.config.get("data", ""))
        if min_max_val is None:
            min_max_val = (0.0, 1.0) if data == "mnist" else (-1.0, 1.0) if data == "mri" else (0.0, 2.0)
        os.makedirs(out_dir, exist_ok=True)
        batches = batches if isinstance(batches, BatchSource) else list(batches)      # (a source makes each step's anew)
        test_batches = list(test_batches)
        train_rows, eval_rows, best = [], [], 1e10

        def write(name, rows):
            if self.rank:                                     # one writer: rank 0
                return
            with open(os.path.join(out_dir, name), "w") as f:
                f.write(",epoch,loss\n" + "".join(f"{i},{e},{v}\n" for i, (e, v) in enumerate(rows)))
        while self.step < num_steps:
            at = self.step
            train_rows.append((at, float(self.train_step(batches))))
            write("train_loss.csv", train_rows)
            if self.step % save_and_sample_every == 0:
                if self.world > 1:
                    self.replica_digest()                     # (one wait beside a full sampling run)
                ls = self.evaluate(test_batches, min_max_val, sharded=bool(sharded_eval))
                if best > ls:
                    best = ls
                    num = 100 if data == "mnist" else 500
                    if self.rank == 0:
                        self.save(os.path.join(out_dir, f"model-best{int(math.ceil(self.step / num)) * num}.pt"))
                eval_rows.append((self.step, ls))
                write("loss.csv", eval_rows)
        return best
