#!/usr/bin/env python3
"""train_seg.py-equivalent driver: trains the segmentation U-Net (the OOD-mask producer of ood_detector.seg: True) on the
GPU and writes the ``best_dice.pth`` that test.py:219 / tools/run_seg_eval.py --seg-model read.

Reads images and lesion masks from .npy ([N, C, H, W] float32 with C = 1 or 3, H and W multiples of 16; masks [N, 1, H, W]
of 0 / 1).  Images are the normalised, translated slices the reference's loader yields; they go through
evalio.seg_preprocess (lr - |mini|, test.py:213-216), the form in which the net sees them at evaluation time.  The first 70 %
(after a seeded shuffle, train_seg.py:43-48) train, the rest validate; the training images are reshuffled into new batches
every epoch (the reference's DataLoader(shuffle=True), :52; seeded, so a run is reproducible).  The whole data set is held
on the GPU.  The reference's dataset classes and augmentation are not part of this form.

With --store the reference's ``MedSegDataset`` (data.py:676-743) runs on the device instead: raw slices ([N, R, R], any real
dtype) and their label maps ([N, R, R]) go up once as an fp32 and a u8 store (``DeviceDataset.seg``), slices whose label map
holds a single value are left out (``evalio.lesion_slices``, data.py:695-698), and every batch is made by one launch -- centre
crop, ``(x - mean) / std`` with --store-mean / --store-std (the config's mean_flair / std_flair), target = label > 0.  The same
seeded 70 / 30 split is applied to the store's slices; the training batches come from a ``BatchSource`` (reshuffled every epoch
from --seed; --no-shuffle, --drop-last; --augmentations rotates by up to 15 degrees and flips, an extension: the reference has
its flips commented out), the validation batches from one with ``shuffle=False``.

  python tools/train_seg.py --images img.npy --masks mask.npy [--epochs 2000] [--batch-size 32] [--lr 1e-3]
         [--init t1seg.pth] [--out results/seg]
  python tools/train_seg.py --store flair.npy --store-labels seg.npy --store-mean M --store-std S [--crop 224]
         [--augmentations] [--no-shuffle] [--drop-last] [--epochs ...]
Writes <out>/best_dice.pth (whenever the mean validation dice improves), train.csv, val.csv.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import localdiffusion_hallucination_amd as ldh                                   # noqa: E402
from localdiffusion_hallucination_amd import checkpoint, evalio, weights        # noqa: E402
from localdiffusion_hallucination_amd.dataset import BatchSource, DeviceDataset # noqa: E402

MEAN_T1, STD_T1 = 610.7180906353575, 1018.7631901605115                         # config.yaml:55-56


def fit_and_report(a, n_channels, train, val, n_train, n_val):
    net = ldh.SegUNet(n_channels=n_channels)
    if a.init:
        print("init:", checkpoint.load_seg_checkpoint(a.init, net))
    else:
        net.load_state_dict({k: torch.from_numpy(np.asarray(v))
                             for k, v in weights.procedural_seg_state_dict(0, n_channels=n_channels).items()})
    net = net.to("cuda")
    os.makedirs(a.out, exist_ok=True)
    trainer = ldh.SegTrainer(net, lr=a.lr, pos_weight=a.pos_weight)
    res = trainer.fit(train, val, a.epochs, os.path.join(a.out, "best_dice.pth"), log=a.out)
    print(f"train images {n_train}, validation images {n_val}, epochs {a.epochs}")
    print("last train loss: {:.4f}".format(res["train"][-1][1]))
    print("best dice: {:.4f} (epoch {})".format(res["best_dice"], res["best_epoch"]))


def main_store(a):
    """--store: ``MedSegDataset`` on the device."""
    if a.store_labels is None or a.store_mean is None or a.store_std is None:
        raise SystemExit("--store needs --store-labels, --store-mean and --store-std")
    if a.masks is not None:
        raise SystemExit("--masks belongs to --images; the labels of --store are --store-labels")
    images, labels = np.load(a.store), np.load(a.store_labels)
    if images.ndim != 3 or images.shape[1] != images.shape[2] or labels.shape != images.shape:
        raise SystemExit(f"--store / --store-labels: expected [N, R, R] twice, got {images.shape} and {labels.shape}")
    if a.crop % 16:
        raise SystemExit(f"--crop: {a.crop} must be a multiple of 16")
    keep = evalio.lesion_slices(labels)
    print(f"{len(keep)} of {images.shape[0]} slices hold a lesion")
    order = keep[np.random.RandomState(a.seed).permutation(len(keep))]
    n_train = max(1, int(0.7 * len(order)))
    tr_idx, va_idx = order[:n_train], order[n_train:]
    if len(va_idx) == 0:
        raise SystemExit("fewer than two slices with a lesion: nothing to validate on")
    last = len(tr_idx) % a.batch_size
    if last and not a.drop_last and last * (a.crop // 16) ** 2 < 2:           # BatchNorm needs two values per channel
        raise SystemExit(f"the last of the {len(tr_idx)} training slices' batches of {a.batch_size} holds {last} slice(s) of "
                         f"{a.crop // 16} x {a.crop // 16} at the deepest level: BatchNorm needs two values per channel; pass --drop-last")
    try:
        kw = dict(mean=a.store_mean, std=a.store_std, crop=a.crop)
        train = BatchSource(DeviceDataset.seg(images[tr_idx], labels[tr_idx], augmentations=a.augmentations, **kw), a.batch_size,
                            shuffle=not a.no_shuffle, seed=a.seed, drop_last=a.drop_last)
        val = BatchSource(DeviceDataset.seg(images[va_idx], labels[va_idx], **kw), a.batch_size, shuffle=False)
    except ValueError as e:
        raise SystemExit(str(e))
    fit_and_report(a, 1, train, val, len(tr_idx), len(va_idx))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", default=None)
    ap.add_argument("--masks", default=None)
    ap.add_argument("--store", default=None, help="raw slices [N, R, R] (.npy): batches are made on the device")
    ap.add_argument("--store-labels", default=None, help="label maps [N, R, R] (.npy) of --store")
    ap.add_argument("--store-mean", type=float, default=None)
    ap.add_argument("--store-std", type=float, default=None)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--augmentations", action="store_true")
    ap.add_argument("--no-shuffle", action="store_true")
    ap.add_argument("--drop-last", action="store_true")
    ap.add_argument("--epochs", type=int, default=2000)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--pos-weight", type=float, default=10.0)
    ap.add_argument("--init", default=None, help="state_dict to start from (default: procedural weights, seed 0)")
    ap.add_argument("--mean-t1", type=float, default=MEAN_T1)
    ap.add_argument("--std-t1", type=float, default=STD_T1)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default="results/seg")
    a = ap.parse_args()
    if (a.images is None) == (a.store is None):
        raise SystemExit("give exactly one of --images (with --masks) and --store (with --store-labels, --store-mean, --store-std)")
    if a.store is not None:
        return main_store(a)
    if a.masks is None:
        raise SystemExit("--images needs --masks")
    x = torch.from_numpy(np.load(a.images).astype(np.float32))
    y = torch.from_numpy(np.load(a.masks).astype(np.float32))
    if x.dim() != 4 or x.shape[1] not in (1, 3) or tuple(y.shape) != (x.shape[0], 1, x.shape[2], x.shape[3]):
        raise SystemExit(f"--images / --masks: expected [N, 1 or 3, H, W] and [N, 1, H, W], got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[2] % 16 or x.shape[3] % 16:
        raise SystemExit(f"--images: H, W = {x.shape[2]}, {x.shape[3]} must be multiples of 16")
    x = evalio.seg_preprocess(x, a.mean_t1, a.std_t1)
    order = np.random.RandomState(a.seed).permutation(x.shape[0])
    n_train = max(1, int(0.7 * x.shape[0]))
    tr_idx, va_idx = order[:n_train], order[n_train:]
    if len(va_idx) == 0:
        raise SystemExit("fewer than two images: nothing to validate on")

    x, y = x.cuda(), y.cuda()

    def batches(idx):
        out = []
        for i in range(0, len(idx), a.batch_size):
            sel = torch.from_numpy(np.asarray(idx[i:i + a.batch_size])).cuda()
            if len(sel) * (x.shape[2] // 16) * (x.shape[3] // 16) >= 2:           # BatchNorm needs two values per channel
                out.append((x[sel], y[sel]))
        return out

    def train_batches(epoch):                                                     # DataLoader(shuffle=True)
        return batches(tr_idx[np.random.RandomState(a.seed + 1 + epoch).permutation(len(tr_idx))])

    fit_and_report(a, x.shape[1], train_batches, batches(va_idx), len(tr_idx), len(va_idx))


if __name__ == "__main__":
    main()
