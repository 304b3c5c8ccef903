#!/usr/bin/env python3
"""test.py-equivalent driver for the MRI configuration with the segmentation OOD detector (config.yaml ood_detector.seg:
True): reads LR / HR slices from .npy ([N, 1, H, W] float32, already normalised and translated as the reference's data
loader leaves them; BRATS PNG decoding is not part of this), builds the OOD mask with the segmentation U-Net
(evalio.seg_ood_mask: lr - |mini|, sigmoid > 0.5, test.py:214-221, 284-289), samples with branch + fusion on the GPU and
writes hr_all / lr_all / pred_all / ad_masks .npy.

  python tools/run_seg_eval.py --lr lr.npy --hr hr.npy [--seg-model t1seg.pth] [--checkpoint model-best.pt]
         [--timesteps 1000] [--ddim 0] [--out eval_out] [--metrics]
Without --seg-model / --checkpoint the procedural weights of the tests are used (no trained weights ship with the reference).
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

MEAN_T1, STD_T1 = 610.7180906353575, 1018.7631901605115                         # config.yaml:55-56


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lr", required=True)
    ap.add_argument("--hr", required=True)
    ap.add_argument("--seg-model", default=None, help="state_dict of the segmentation U-Net (train_seg.py's output)")
    ap.add_argument("--checkpoint", default=None, help="Trainer.save file of the denoiser")
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--ddim", type=int, default=0, help="sampling_timesteps (0 = ancestral DDPM)")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--seg-dtype", default="fp32", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--mean-t1", type=float, default=MEAN_T1)
    ap.add_argument("--std-t1", type=float, default=STD_T1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--metrics", action="store_true",
                    help="MSE / PSNR / SSIM per image and per region (whole image, OOD mask, the rest); metrics.json with --out")
    a = ap.parse_args()
    lr = torch.from_numpy(np.load(a.lr).astype(np.float32))
    hr = torch.from_numpy(np.load(a.hr).astype(np.float32))
    if lr.dim() != 4 or lr.shape != hr.shape or lr.shape[2] != lr.shape[3]:
        raise SystemExit(f"--lr / --hr: expected two [N, 1, H, H] arrays, got {tuple(lr.shape)} and {tuple(hr.shape)}")
    H = lr.shape[-1]

    seg = ldh.SegUNet(n_channels=lr.shape[1], compute_dtype=a.seg_dtype)
    if a.seg_model:
        print("seg model:", checkpoint.load_seg_checkpoint(a.seg_model, seg))
    else:
        seg.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_seg_state_dict(0).items()})
    seg = seg.to("cuda").eval()
    masks = []
    with torch.no_grad():
        for i in range(lr.shape[0]):                       # one image at a time, as test.py's loader (batch size 1)
            _, binary = evalio.seg_ood_mask(seg, lr[i:i + 1].cuda(), a.mean_t1, a.std_t1)
            masks.append(binary.cpu())
    masks = torch.cat(masks)
    print(f"OOD mask: {float(masks.mean()) * 100:.1f} % of pixels")

    config = dict(branch_out=True, start_intermediate=True, start_timestep=2, data="mri", mask_x=True, mask_cond=False,
                  ood_AD=True, ood_confidence=False, classifier=False, use_gt=False, use_gt_timestep=100)
    net = ldh.Unet(dim=32, init_dim=32, mode="mri", compute_dtype=a.dtype)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.procedural_state_dict(net.cfg, 0).items()})
    gd = ldh.GaussianDiffusion(config, net, image_size=H, timesteps=a.timesteps, beta_schedule="sigmoid",
                               objective="pred_x0", sampling_timesteps=a.ddim or None)
    if a.checkpoint:
        print("checkpoint:", checkpoint.load_reference_checkpoint(a.checkpoint, gd))
    gd = gd.to("cuda")
    lo_hi = (float(min(lr.min(), hr.min())), float(max(lr.max(), hr.max())))
    res = evalio.evaluate(gd, hr, lr, masks, lo_hi, out_dir=a.out, metrics=a.metrics)
    print("Test loss: {:.4f}".format(res["test_loss"]))
    print("Average sampling time: {:.4f}".format(res["avg_sampling_time"]))
    if a.metrics:
        evalio.print_quality(res["quality"])


if __name__ == "__main__":
    main()
