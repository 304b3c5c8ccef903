#!/usr/bin/env python3
"""Trainer.train-equivalent driver (ddpm.py:1532-1606): trains the denoiser on the GPU with ``ldh.DenoiserTrainer`` and writes
the ``model-best<N>.pt`` files that ``checkpoint.load_reference_checkpoint`` and the reference's ``Trainer.load`` read.

Reads the images and their condition images from .npy: ``--hr`` [N, C, H, H] float32 (C = 1, or 3 for mvtec) in the range the
reference's loader yields for the data set, ``--lr`` [N, 1 or 3, H, H]; H divisible by the net's downsample factor.  The first
70 % (after a seeded shuffle) train, the rest validate.  As in the reference, one step runs over EVERY training batch (each
loss divided by their number) before the optimiser moves; the batches are formed once.  The whole data set is held on the GPU.
The reference's dataset classes and augmentation are not part of this.

  python tools/train_denoiser.py --data mnist --hr hr.npy --lr lr.npy [--steps 1000] [--batch-size 32] [--timesteps 250]
         [--objective pred_v] [--train-lr 1e-4] [--save-every 100] [--init model.pt] [--out results/denoiser]
Writes <out>/model-best<step rounded up>.pt (whenever the evaluation loss improves), train_loss.csv, loss.csv.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import localdiffusion_hallucination_amd as ldh                                   # noqa: E402
from localdiffusion_hallucination_amd import checkpoint, weights                # noqa: E402

KWARGS = {"mri": dict(mode="mri"), "mnist": dict(dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist"),
          "mvtec": dict(channels=3, out_dim=3, mode="mvtec")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True, choices=sorted(KWARGS))
    ap.add_argument("--hr", required=True)
    ap.add_argument("--lr", required=True)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--timesteps", type=int, default=250)
    ap.add_argument("--objective", default="pred_v", choices=["pred_noise", "pred_x0", "pred_v"])
    ap.add_argument("--train-lr", type=float, default=1e-4)
    ap.add_argument("--save-every", type=int, default=100)
    ap.add_argument("--init", default=None, help="reference checkpoint to start from (default: procedural weights, seed 0)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default="results/denoiser")
    a = ap.parse_args()
    hr = torch.from_numpy(np.load(a.hr).astype(np.float32))
    lr = torch.from_numpy(np.load(a.lr).astype(np.float32))
    net = ldh.Unet(dim=32, init_dim=32, **KWARGS[a.data])
    cfg = net.cfg
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

    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_state_dict(cfg, 0).items()})
    config = dict(branch_out=False, start_intermediate=False, start_timestep=2, data=a.data, mask_x=False, ood_AD=False,
                  ood_confidence=False, classifier=False, use_gt=False)
    gd = ldh.GaussianDiffusion(config, net, image_size=int(hr.shape[2]), timesteps=a.timesteps, objective=a.objective)
    if a.init:
        print("init:", checkpoint.load_reference_checkpoint(a.init, gd))
    trainer = ldh.DenoiserTrainer(gd.to("cuda"), train_lr=a.train_lr)
    best = trainer.fit(batches(tr_idx), batches(va_idx), a.steps, a.save_every, a.out)
    print(f"train images {len(tr_idx)}, validation images {len(va_idx)}, steps {trainer.step}")
    print(f"last gradient norm: {trainer.check_finite():.4f}")
    print(f"best evaluation loss: {best:.6f}")


if __name__ == "__main__":
    main()
