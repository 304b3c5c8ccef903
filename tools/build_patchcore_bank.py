#!/usr/bin/env python3
"""Builds a PatchCore memory bank, what anomaly_model_train.py:339-385 does without its datasets: training images ->
PatchCore.embed (wide_resnet50_2 layer2 + layer3) -> KCenterGreedy coreset (sampling ratio 0.1) -> np.save of the
selected rows, fp32 [n, 1536], the file that checkpoint.load_patchcore and test.py:169-175 read.

  python tools/build_patchcore_bank.py --images train.npy --backbone wrn50_2.pth --data mnist --out memory_bank_mnist_train.npy
  python tools/build_patchcore_bank.py --procedural --data mnist --out bank.npy        # procedural weights and images

--images is a .npy array [N, C, H, W] (or [N, H, W]) in the training loader's value range; it is prepared as at bank
time (evalio.patchcore_bank_preprocess: three channels, / 2 when a batch's max is above 1 outside mri, 224 x 224, ImageNet
Normalize) in batches of --batch.  --backbone is a torchvision / timm / anomalib state_dict of wide_resnet50_2.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import localdiffusion_hallucination_amd as ldh                    # noqa: E402
from localdiffusion_hallucination_amd import checkpoint, evalio, weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", help=".npy training images [N, C, H, W] or [N, H, W]")
    ap.add_argument("--backbone", help="wide_resnet50_2 state_dict (.pth / .pt / .safetensors)")
    ap.add_argument("--procedural", action="store_true", help="procedural weights and 16 random 28x28 images")
    ap.add_argument("--data", default="mnist", help="mnist, mri or mvtec (the bank-time preparation differs for mri)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--ratio", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0, help="seed of the projection and the start row")
    ap.add_argument("--trust-pickle", action="store_true")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if not args.procedural and not (args.images and args.backbone):
        ap.error("pass --images and --backbone, or --procedural")
    dev = "cuda"
    size = (84, 84) if args.data == "mnist" else (224, 224)
    m = ldh.PatchCore(size)
    if args.procedural:
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_patchcore_state_dict(args.seed).items()}
        m.feature_extractor.load_state_dict(sd)
        imgs = np.random.default_rng(args.seed).uniform(0.0, 2.0, (16, 1, 28, 28)).astype(np.float32)
    else:
        checkpoint.load_patchcore(args.backbone, np.zeros((1, 1536), np.float32), m, trust_pickle=args.trust_pickle)
        imgs = np.load(args.images).astype(np.float32)
        if imgs.ndim == 3:
            imgs = imgs[:, None]
    m = m.to(dev).eval()
    x = torch.from_numpy(imgs)
    batches = [evalio.patchcore_bank_preprocess(x[i:i + args.batch], args.data) for i in range(0, len(x), args.batch)]
    idx = m.build_memory_bank(batches, args.ratio, seed=args.seed)
    checkpoint.save_patchcore_bank(m, args.out)
    print(f"{len(x)} images -> {idx.numel()} bank rows -> {args.out}")


if __name__ == "__main__":
    main()
