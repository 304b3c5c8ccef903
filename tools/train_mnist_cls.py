#!/usr/bin/env python3
"""train_mnist_cls.py-equivalent driver: trains the MNIST digit classifier (SimpleCNN) on the GPU and writes the best
checkpoint and the loss CSV as the reference's script does (train_mnist_cls.py:79-119).

Reads the four idx(.gz) files through evalio.read_idx; the paths are arguments (the reference hard-codes ./MNIST/raw/...).
Images are 2 * u8 / 255 (data.py:809), the range of the sampler's output for min_max_val = (0, 2).  The training digits are
reshuffled into new batches every epoch (the reference's DataLoader(shuffle=True), :69; seeded, so a run is reproducible).
The whole data set is held on the GPU.

With --device-data the digits stay u8 on the device (``DeviceDataset.mnist_cls``: a quarter of the fp32 tensors' bytes) and
every batch is made there by one launch from a ``BatchSource``'s seeded plan -- the epoch's shuffle and, with --augmentations,
the ``RandomRotation(15)`` + ``RandomVerticalFlip`` of data.py:783-786 -- while the step before it runs; no list of an epoch's
batches is built.  The test digits come from a second source (``shuffle=False``, batches of 512).

  python tools/train_mnist_cls.py --train-images train-images-idx3-ubyte.gz --train-labels train-labels-idx1-ubyte.gz
         --test-images t10k-images-idx3-ubyte.gz --test-labels t10k-labels-idx1-ubyte.gz
         [--epochs 1000] [--batch-size 64] [--lr 1e-3] [--init cls.pth] [--out results/mnist_cls]
         [--device-data [--augmentations]]
Writes <out>/mnist_cls_best_model.pth (whenever the test accuracy improves) and <out>/mnist_cls_loss.csv.
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


def read(images, labels, max_n=None):
    x, y = evalio.read_idx(images), evalio.read_idx(labels)
    if x.ndim != 3 or tuple(x.shape[1:]) != (28, 28) or y.shape != (x.shape[0],):
        raise SystemExit(f"{images} / {labels}: expected [N, 28, 28] images and [N] labels, got {x.shape} and {y.shape}")
    return x[:max_n].copy(), y[:max_n].copy()                                     # (read_idx's arrays view the file's bytes)


def load(images, labels, max_n=None):
    x, y = read(images, labels, max_n)
    x = 2.0 * (torch.from_numpy(np.ascontiguousarray(x).astype(np.float32))[:, None] / 255.0)
    return x.cuda(), torch.from_numpy(y.astype(np.int64)).cuda()


def main():
    ap = argparse.ArgumentParser()
    for name in ("train-images", "train-labels", "test-images", "test-labels"):
        ap.add_argument("--" + name, required=True)
    ap.add_argument("--epochs", type=int, default=1000)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--max-train", type=int, default=None)
    ap.add_argument("--init", default=None, help="state_dict to start from (default: procedural weights, seed 0)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default="results/mnist_cls")
    ap.add_argument("--device-data", action="store_true", help="u8 stores on the device, one launch per batch (BatchSource)")
    ap.add_argument("--augmentations", action="store_true", help="with --device-data: RandomRotation(15) + RandomVerticalFlip")
    a = ap.parse_args()
    if a.augmentations and not a.device_data:
        raise SystemExit("--augmentations needs --device-data")
    if a.device_data:
        try:
            x_tr, y_tr = read(a.train_images, a.train_labels, a.max_train)
            x_te, y_te = read(a.test_images, a.test_labels)
            train_batches = BatchSource(DeviceDataset.mnist_cls(x_tr, y_tr.astype(np.int64), augmentations=a.augmentations),
                                        a.batch_size, seed=a.seed)
            test_batches = BatchSource(DeviceDataset.mnist_cls(x_te, y_te.astype(np.int64)), 512, shuffle=False)
        except ValueError as e:
            raise SystemExit(str(e))
    else:
        x_tr, y_tr = load(a.train_images, a.train_labels, a.max_train)
        x_te, y_te = load(a.test_images, a.test_labels)

        def train_batches(epoch):                                                 # DataLoader(shuffle=True)
            order = torch.from_numpy(np.random.RandomState(a.seed + epoch).permutation(x_tr.shape[0])).cuda()
            return [(x_tr[order[i:i + a.batch_size]], y_tr[order[i:i + a.batch_size]]) for i in range(0, len(order), a.batch_size)]

        test_batches = [(x_te[i:i + 512], y_te[i:i + 512]) for i in range(0, x_te.shape[0], 512)]
    net = ldh.MnistClassifier()
    if a.init:
        print("init:", checkpoint.load_mnist_classifier(a.init, net))
    else:
        net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.procedural_mnistcls_state_dict(0).items()})
    net = net.to("cuda")
    os.makedirs(a.out, exist_ok=True)
    trainer = ldh.MnistClassifierTrainer(net, lr=a.lr)
    res = trainer.fit(train_batches, test_batches, a.epochs, os.path.join(a.out, "mnist_cls_best_model.pth"),
                      os.path.join(a.out, "mnist_cls_loss.csv"))
    print(f"train digits {x_tr.shape[0]}, test digits {x_te.shape[0]}, epochs {a.epochs}")
    print("mean train loss over all steps: {:.4f}".format(res["rows"][-1][1]))
    print("best accuracy: {:.2f} % (epoch {})".format(res["best_acc"], res["best_epoch"]))


if __name__ == "__main__":
    main()
