#!/usr/bin/env python3
"""Trainer.train-equivalent driver (ddpm.py:1532-1606): trains the denoiser on the GPU with ``ldh.DenoiserTrainer`` and writes
the ``model-best<N>.pt`` files that ``checkpoint.load_reference_checkpoint`` and the reference's ``Trainer.load`` read.

Two ways to give it data.  ``--store`` trains from a RAW store as the reference's ``Trainer`` does (ddpm.py:1305-1384, 1538-1553):
the store lives on the GPU (``ldh.DeviceDataset``), and at EVERY step the batches are regrouped by a fresh shuffle and, with
``--augmentations`` (the config's ``augmentations``), every sample is rotated by a fresh angle in [-15, 15) degrees and flipped
vertically with probability 0.5 before its condition image is derived from it (``ldh.BatchSource``; csrc/dataset.hip).
  mnist  ``--store`` uint8 [N, 28, 28] in file order, ``--labels`` [N]: the first 70 % of the FILE (ddpm.py:1339-1346; the
         reference shuffles an index array it then does not use) train, the rest validate; of each part the first 200 / 100
         images of ``--digit`` (8) are kept (``MNIST(num=8, max_file=200 / 100)``, ddpm.py:1349-1350, ``evalio.select_digits``).
         Without ``--labels`` the store is taken as already selected and only split.
  mvtec  ``--store`` uint8 [N, 3, S, S], already resized (the PIL resize is a one-off host step); 70 % / 30 % in file order.
  mri    ``--store`` / ``--store-cond`` float [N, R, R] (the image's and the condition's modality), ``--mean-target
         --std-target --mean-cond --std-cond`` (the config's constants), ``--crop`` (224), ``--no-translate-zero``; 80 % / 20 %
         in file order (ddpm.py:1313).
  The reference shuffles the mvtec / mri FILE LISTS (seed 42) before the split; a store has no file names, so put it in the
  order you want split.  ``--no-shuffle`` turns the per-step shuffle off, ``--drop-last`` drops a ragged last batch (needed
  with ``--gpus N`` when it is no multiple of N).  Validation batches are unaugmented, unshuffled, and made once.
``--hr`` / ``--lr`` (the earlier interface, unchanged) read ready pairs from .npy: ``--hr`` [N, C, H, H] float32 (C = 1, or 3 for
mvtec) in the range the reference's loader yields for the data set, ``--lr`` [N, 1 or 3, H, H]; H divisible by the net's downsample
factor.  The first 70 % (after a seeded shuffle) train, the rest validate, and the batches are formed once.
Either way one step runs over EVERY training batch (each loss divided by their number) before the optimiser moves, as in the
reference, and the whole data set is held on the GPU.

  python tools/train_denoiser.py --data mnist --store images.npy --labels labels.npy [--augmentations] [--no-shuffle]
  python tools/train_denoiser.py --data mnist --hr hr.npy --lr lr.npy [--steps 1000] [--batch-size 32] [--timesteps 250]
         [--objective pred_v] [--train-lr 1e-4] [--save-every 100] [--init model.pt] [--out results/denoiser]
         [--gpus N] [--rank-timeout 86400] [--grace 30] [--sharded-eval]
Writes <out>/model-best<step rounded up>.pt (whenever the evaluation loss improves), train_loss.csv, loss.csv.

``--gpus N`` (one node): the tool starts N fresh rank processes of itself (``launch.launch_ranks``; this process makes no GPU
call), each on its own GPU over RCCL (torch.distributed's "nccl").  ``--batch-size`` stays the GLOBAL batch: rank r trains on
its rows of every batch (the reference's ``Accelerator(split_batches=True)``), the gradients are summed in rank order, and the
replicas hold the same bits after every step; every batch size must be a multiple of N.  All ranks are seeded alike, every rank
evaluates (every validation batch by default; with ``--sharded-eval`` its rows of each, one all-gather of the per-row error sums
giving every rank the same loss), rank 0 writes the files, and every rank prints its ``replica_digest()`` at the end.  ``--rank-timeout`` bounds the
whole run, ``--grace`` is what the other ranks get once one has failed.  ``--share-gpu`` is for tests only: the ranks share the
visible GPUs, which RCCL refuses, so they meet over gloo and the gradient exchange is staged through pinned host memory -- a
functional path, never a measurement; the log line says so.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import grad_bench                                                                # noqa: E402
import localdiffusion_hallucination_amd as ldh                                   # noqa: E402
from localdiffusion_hallucination_amd import checkpoint, weights                # noqa: E402

KWARGS = {"mri": dict(mode="mri"), "mnist": dict(dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist"),
          "mvtec": dict(channels=3, out_dim=3, mode="mvtec")}
SWITCH_HELP = {
    "conv_precision": "bf16: the convolutions and their gradients on the bf16 matrix cores (operands rounded, fp32 accumulation)",
    "act_storage": "bf16 (with --conv-precision bf16): activations that only convolutions read are kept as bf16; same results",
    "conv_out_storage": "bf16 (with --conv-precision bf16): the convolution outputs GroupNorm reads are kept as bf16; results move "
                        "by about what the bf16 convolutions move them",
    "attn_precision": "bf16: the LinearAttention cores on the bf16 matrix cores (operands rounded, fp32 accumulation)",
    "full_attn_precision": "bf16: the full-softmax Attention cores on the bf16 matrix cores (operands rounded, fp32 accumulation)",
}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True, choices=sorted(KWARGS))
    ap.add_argument("--hr", default=None)
    ap.add_argument("--lr", default=None)
    ap.add_argument("--store", default=None, help="raw store (.npy): trains with fresh batches every step; replaces --hr / --lr")
    ap.add_argument("--store-cond", default=None, help="mri: the condition modality's store (.npy)")
    ap.add_argument("--labels", default=None, help="mnist: the store's labels (.npy), for the reference's digit selection")
    ap.add_argument("--digit", type=int, default=8)
    ap.add_argument("--augmentations", action="store_true", help="with --store: RandomRotation(15) + RandomVerticalFlip per sample per step")
    ap.add_argument("--no-shuffle", action="store_true", help="with --store: keep the store's order at every step")
    ap.add_argument("--drop-last", action="store_true", help="with --store: drop a ragged last batch")
    for name in ("mean-target", "std-target", "mean-cond", "std-cond"):
        ap.add_argument("--" + name, type=float, default=None, help="mri with --store: the modality's normalisation constant")
    ap.add_argument("--crop", type=int, default=224, help="mri with --store: the centre crop")
    ap.add_argument("--no-translate-zero", action="store_true", help="mri with --store: no + |min| shift")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--timesteps", type=int, default=250)
    ap.add_argument("--objective", default="pred_v", choices=["pred_noise", "pred_x0", "pred_v"])
    ap.add_argument("--train-lr", type=float, default=1e-4)
    grad_bench.add_switch_flags(ap, SWITCH_HELP)
    ap.add_argument("--amp", action="store_true", help="the reference's mixed precision (Trainer(amp=True)): see --mixed-precision-type")
    ap.add_argument("--mixed-precision-type", default="fp16", choices=["fp16", "bf16"],
                    help="with --amp: fp16 = the convolutions on the fp16 matrix cores under a loss scaler on the device "
                         "(GradScaler's defaults); bf16 = --conv-precision bf16, no scaler")
    ap.add_argument("--amp-attn", default="fp32", choices=["fp32", "fp16"],
                    help="fp16 (with --amp and --mixed-precision-type fp16 only): the attention cores on the fp16 matrix cores "
                         "too, under the same loss scaler")
    ap.add_argument("--save-every", type=int, default=100)
    ap.add_argument("--init", default=None, help="reference checkpoint to start from (default: procedural weights, seed 0)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default="results/denoiser")
    ap.add_argument("--gpus", type=int, default=1, help="data-parallel ranks on this node, one GPU each")
    ap.add_argument("--rank-timeout", type=float, default=86400.0, help="--gpus > 1: seconds that bound the whole run")
    ap.add_argument("--grace", type=float, default=30.0, help="--gpus > 1: seconds the other ranks get after one has failed")
    ap.add_argument("--sharded-eval", action="store_true",
                    help="evaluate with DenoiserTrainer.evaluate(sharded=True): every rank samples its rows of each validation batch")
    ap.add_argument("--share-gpu", action="store_true",
                    help="tests only: the ranks share the visible GPUs over gloo, gradients staged through host memory")
    a = ap.parse_args(argv)
    if (a.store is None) == (a.hr is None and a.lr is None) or (a.store is None and (a.hr is None or a.lr is None)):
        ap.error("give either --store (raw data, fresh batches every step) or both --hr and --lr (ready pairs)")
    if a.store is None and (a.augmentations or a.no_shuffle or a.drop_last or a.labels or a.store_cond):
        ap.error("--augmentations / --no-shuffle / --drop-last / --labels / --store-cond need --store")
    return a


def store_sources(a, cfg):
    """``--store``: (training ``BatchSource``, validation batches, image size) as ``Trainer.__init__`` splits the data."""
    from localdiffusion_hallucination_amd import evalio
    from localdiffusion_hallucination_amd.dataset import BatchSource, DeviceDataset
    store = np.load(a.store)
    n = store.shape[0]
    cut = int((0.8 if a.data == "mri" else 0.7) * n)
    if a.data == "mnist":
        tr, va = store[:cut], store[cut:]
        if a.labels:
            labels = np.load(a.labels)
            if labels.shape != (n,):
                raise SystemExit(f"--labels: expected [{n}], got {labels.shape}")
            tr, _ = evalio.select_digits(tr, labels[:cut], a.digit, 200)
            va, _ = evalio.select_digits(va, labels[cut:], a.digit, 100)
        make = lambda x, aug: DeviceDataset.mnist(x, augmentations=aug)                     # noqa: E731
        parts = (tr, va)
    elif a.data == "mvtec":
        make = lambda x, aug: DeviceDataset.sr(x, augmentations=aug)                        # noqa: E731
        parts = (store[:cut], store[cut:])
    else:
        consts = dict(mean_target=a.mean_target, std_target=a.std_target, mean_cond=a.mean_cond, std_cond=a.std_cond)
        if a.store_cond is None or any(v is None for v in consts.values()):
            raise SystemExit("--data mri --store needs --store-cond, --mean-target, --std-target, --mean-cond and --std-cond")
        cond = np.load(a.store_cond)
        make = lambda x, aug: DeviceDataset.mri(x[0], x[1], augmentations=aug, crop=a.crop,        # noqa: E731
                                                translate_zero=not a.no_translate_zero, **consts)
        parts = ((store[:cut], cond[:cut]), (store[cut:], cond[cut:]))
    if min(len(p[0]) if isinstance(p, tuple) else len(p) for p in parts) < 1:
        raise SystemExit("--store: the split leaves nothing to train or to validate on")
    try:
        train_ds, val_ds = make(parts[0], a.augmentations), make(parts[1], False)
        train = BatchSource(train_ds, a.batch_size, shuffle=not a.no_shuffle, seed=a.seed, drop_last=a.drop_last)
        val = list(BatchSource(val_ds, a.batch_size, shuffle=False, drop_last=a.drop_last).batches(0))
    except ValueError as e:
        raise SystemExit(f"--store: {e}")
    if train_ds.channels != cfg.channels or train_ds.image_size % cfg.downsample_factor:
        raise SystemExit(f"--store: {train_ds.channels} channels of {train_ds.image_size}^2; the {a.data} net takes {cfg.channels} "
                         f"and a size divisible by {cfg.downsample_factor}")
    return train, val, train_ds.image_size


def pair_batches(a, cfg):
    """``--hr`` / ``--lr``: (training batches, validation batches, image size), formed once."""
    hr = torch.from_numpy(np.load(a.hr).astype(np.float32))
    lr = torch.from_numpy(np.load(a.lr).astype(np.float32))
    if hr.dim() != 4 or hr.shape[1] != cfg.channels or hr.shape[2] != hr.shape[3] or \
            tuple(lr.shape) != (hr.shape[0], cfg.cond_in_channels, hr.shape[2], hr.shape[3]):
        raise SystemExit(f"--hr / --lr: expected [N, {cfg.channels}, H, H] and [N, {cfg.cond_in_channels}, H, H], got "
                         f"{tuple(hr.shape)} and {tuple(lr.shape)}")
    if hr.shape[2] % cfg.downsample_factor:
        raise SystemExit(f"--hr: H = {hr.shape[2]} must be divisible by {cfg.downsample_factor}")
    order = np.random.RandomState(a.seed).permutation(hr.shape[0])
    n_train = max(1, int(0.7 * hr.shape[0]))
    tr_idx, va_idx = order[:n_train], order[n_train:]
    if len(va_idx) == 0:
        raise SystemExit("fewer than two images: nothing to validate on")
    hr, lr = hr.cuda(), lr.cuda()

    def batches(idx):
        sel = [torch.from_numpy(np.asarray(idx[i:i + a.batch_size])).cuda() for i in range(0, len(idx), a.batch_size)]
        return [(hr[s], lr[s]) for s in sel]

    return batches(tr_idx), batches(va_idx), int(hr.shape[2])


def setup(a, **trainer_kw):
    """The trainer and its (train, validation) batches for the parsed arguments, on the current GPU."""
    net = ldh.Unet(dim=32, init_dim=32, **KWARGS[a.data])
    cfg = net.cfg
    if a.store is not None:
        train, val, image_size = store_sources(a, cfg)
    else:
        train, val, image_size = pair_batches(a, cfg)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_state_dict(cfg, 0).items()})
    config = dict(branch_out=False, start_intermediate=False, start_timestep=2, data=a.data, mask_x=False, ood_AD=False,
                  ood_confidence=False, classifier=False, use_gt=False)
    gd = ldh.GaussianDiffusion(config, net, image_size=image_size, timesteps=a.timesteps, objective=a.objective)
    if a.init:
        print("init:", checkpoint.load_reference_checkpoint(a.init, gd))
    switches = grad_bench.switch_values(a, SWITCH_HELP)
    if getattr(a, "amp", False):
        if a.mixed_precision_type == "bf16" and switches["conv_precision"] == "fp32":
            del switches["conv_precision"]                    # (the flag's default: --amp chooses)
        trainer_kw = dict(trainer_kw, amp=True, mixed_precision_type=a.mixed_precision_type)
    if getattr(a, "amp_attn", "fp32") != "fp32":
        trainer_kw = dict(trainer_kw, amp_attn=a.amp_attn)
    trainer = ldh.DenoiserTrainer(gd.to(torch.device("cuda", torch.cuda.current_device())), train_lr=a.train_lr, **switches,
                                  **trainer_kw)
    return trainer, train, val


def main(argv=None):
    a = parse(argv)
    if a.gpus > 1 and "RANK" not in os.environ:              # the parent: starts the ranks, makes no GPU call itself
        from localdiffusion_hallucination_amd.launch import launch_ranks
        log_dir = os.path.join(a.out, "ranks")                # rank<r>.out / rank<r>.err
        try:
            rc = launch_ranks([sys.executable, os.path.abspath(__file__)] + list(sys.argv[1:] if argv is None else argv), a.gpus,
                              timeout_s=a.rank_timeout, grace_s=a.grace, log_dir=log_dir, share_gpu=a.share_gpu)
        except ValueError as e:
            raise SystemExit(f"train_denoiser.py: {e}")
        for r in range(a.gpus):                              # rank 0's output, and every rank's digest line
            try:
                for line in open(os.path.join(log_dir, f"rank{r}.out"), errors="replace"):
                    if r == 0 or line.startswith("replica digest"):
                        sys.stdout.write(line)
            except OSError:
                pass
        sys.exit(rc)
    kw, world, rank = {}, int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if a.gpus > 1:
        import torch.distributed as dist
        if world != a.gpus:
            raise SystemExit(f"train_denoiser.py: --gpus {a.gpus} but WORLD_SIZE={world}")
        ldh.configure_runtime()                              # before the first GPU call
        local = int(os.environ.get("LOCAL_RANK", "0"))
        if a.share_gpu:
            # several ranks on one GPU, which RCCL refuses: gloo, and the trainer stages its exchange through pinned host
            # memory (this torch's gloo is not asked to gather device tensors)
            local %= max(1, torch.cuda.device_count())
            dist.init_process_group("gloo", rank=rank, world_size=world)
            print("[--share-gpu: ranks share a GPU over gloo, gradients staged through host memory -- functional test, "
                  "not a measurement]")
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))   # RCCL
        torch.cuda.set_device(local)
        kw = dict(group="default")
    trainer, train, val = setup(a, **kw)
    torch.manual_seed(a.seed)                                # every rank alike: t comes from this generator
    best = trainer.fit(train, val, a.steps, a.save_every, a.out, sharded_eval=a.sharded_eval)
    if rank == 0:
        n_train = len(train.dataset) if a.store is not None else sum(b[0].shape[0] for b in train)
        print(f"train images {n_train}, validation images {sum(b[0].shape[0] for b in val)}, "
              f"steps {trainer.step}, ranks {trainer.world}")
        print(f"last gradient norm: {trainer.check_finite():.4f}")
        if trainer.scaler is not None:
            s = trainer.scaler_state()
            print(f"loss scaler: scale {s['scale']:.0f}, {s['adam_steps']} optimiser steps, {s['skipped_steps']} skipped")
        print(f"best evaluation loss: {best:.6f}")
    d = trainer.replica_digest()
    print(f"replica digest: step {d['step']} sumsq {d['sumsq']!r} weight_sum {d['weight_sum']!r} "
          f"weight_xor {d['weight_xor']:#010x}", flush=True)
    if a.gpus > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
