"""Data formats either side of the sampling path: what the reference's
``test.py`` does before and after ``sample()``, restated host-side so an end-to-end run is comparable
with the authors' script.

* MNIST idx(.gz) reader (the reference uses ``idx2numpy``; files under ``MNIST/raw``);
* ``MNIST.__getitem__`` LR/HR pair (/root/reference/data.py:808-829): HR = 2x/255; LR: the reference indexes the
  [1,1,28,28] image with ``img[:, ::2, ::2]`` -- dims 0, 1, 2 -- so only the ROWS are decimated (-> [1,1,14,28]),
  then bilinear resize back to 28x28 (align_corners=False: rows x2, columns unchanged), then 2*/255.  Pinned by
  tests/golden/g4_cfg1_mnist.npz, whose ``cond`` comes from the reference's own dataset class;
* the hand-drawn OOD mask of the released script (columns 0..6 = 1, /root/reference/test.py:379-381) and
  the soft mask derived from a thresholded anomaly map (/root/reference/test.py:259-262);
* the evaluation loop: one ``sample()`` per image (batch size 1, test.py:108,190,393), MSE of the last
  channel vs HR (:416), mean wall time (:445), ``hr_all / lr_all / pred_all / ad_masks .npy`` (:429-442).
"""
import gzip
import os
import struct
import time

import numpy as np
import torch
import torch.nn.functional as F

_IDX_DTYPES = {0x08: np.uint8, 0x09: np.int8, 0x0B: ">i2", 0x0C: ">i4", 0x0D: ">f4", 0x0E: ">f8"}


def read_idx(path):
    """Parse an idx file (optionally gzip-compressed): magic = 0, 0, dtype code, ndim; big-endian dims."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as f:
        raw = f.read()
    zero, dcode, ndim = struct.unpack(">HBB", raw[:4])
    if zero != 0 or dcode not in _IDX_DTYPES:
        raise ValueError(f"{path}: not an idx file (magic {raw[:4].hex()})")
    dims = struct.unpack(">" + "I" * ndim, raw[4:4 + 4 * ndim])
    data = np.frombuffer(raw, dtype=_IDX_DTYPES[dcode], offset=4 + 4 * ndim)
    if data.size != int(np.prod(dims)):
        raise ValueError(f"{path}: payload has {data.size} items, header says {dims}")
    return data.reshape(dims)


def select_digits(images, labels, digits, max_n=None):
    """Images whose label is in ``digits`` in file order (MNIST.__init__, data.py:770-776)."""
    digits = [digits] if np.isscalar(digits) else list(digits)
    idx = np.nonzero(np.isin(labels, digits))[0]
    if max_n is not None:
        idx = idx[:max_n]
    return images[idx].copy(), labels[idx].copy()


def mnist_pairs(images_u8):
    """uint8 [N,28,28] -> (hr, lr) float32 [N,1,28,28] in [0, 2]  (data.py:808-829)."""
    x = torch.from_numpy(np.ascontiguousarray(images_u8).astype(np.float32))[:, None]
    # data.py:817 slices dims (0, 1, 2) of the [1,1,H,W] tensor: rows only
    lr = F.interpolate(x[:, :, ::2, :], size=(x.shape[-2], x.shape[-1]), mode="bilinear", align_corners=False)
    return 2.0 * (x / 255.0), 2.0 * (lr / 255.0)


def lesion_slices(labels):
    """Indices of the slices of ``labels`` [N, H, W] that hold more than one distinct value -- ``MedSegDataset.__init__``'s
    filter ``len(np.unique(slice)) > 1`` (data.py:695-698): an all-background slice, or one label throughout, is left out.
    Host-side; applied once to images and labels before a ``DeviceDataset.seg`` store is built."""
    a = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if a.ndim != 3:
        raise ValueError(f"lesion_slices: labels must be [N, H, W], got {a.shape}")
    flat = a.reshape(a.shape[0], -1)
    if flat.shape[1] == 0:
        return np.zeros(0, dtype=np.int64)
    return np.nonzero((flat != flat[:, :1]).any(axis=1))[0].astype(np.int64)


def band_mask(n, h, w, ncols=7):
    """The released script's manual OOD mask: ones in the first ``ncols`` columns (test.py:379-381)."""
    m = torch.zeros(n, 1, h, w)
    m[:, :, :, :ncols] = 1.0
    return m


def anomaly_map_to_mask(anomaly_map, threshold):
    """Soft OOD mask from an anomaly map (test.py:259-262): -> (mask_pred in [0,1], binary_mask)."""
    a = anomaly_map.detach().cpu().float()
    binary = (a > threshold).float()
    m = torch.clip(a, min=threshold - float(a.std()), max=threshold)
    m = (m - m.min()) / (threshold - m.min())
    return m ** 2, binary


def seg_preprocess(lr, mean_t1, std_t1, translate_zero=True):
    """The segmentation net's input (test.py:213-216): lr - |(0 - mean_t1) / std_t1|.  The reference defines that
    constant (``mini``) only under ``translate_zero``; without it test.py:216 raises NameError, and so does this."""
    if not translate_zero:
        raise NameError("name 'mini' is not defined: the reference's segmentation path (test.py:214-216) uses the "
                        "translate_zero shift, which is only defined with translate_zero=True")
    mini = (0 - mean_t1) / std_t1
    return lr - abs(float(torch.tensor(mini)))


def seg_ood_mask(seg, lr, mean_t1, std_t1, translate_zero=True):
    """The reference's segmentation OOD mask (test.py:203-221, 284-289): ``seg`` (a ``SegUNet``) on lr - |mini|, then
    sigmoid(logits) > 0.5.  Returns (mask_pred, binary_mask), both [B, 1, H, W] fp32 on ``lr``'s device, with
    mask_pred = binary_mask as test.py:289 sets it."""
    lr_ad = seg_preprocess(lr.float(), mean_t1, std_t1, translate_zero)
    _, binary = seg.predict_mask(lr_ad)
    return binary, binary


def digit_report(classifier, images, labels, batch_size=512):
    """The MNIST experiment's read-out: which digit does ``classifier`` (a ``MnistClassifier``) see in each image?
    ``images`` [N, 1, 28, 28] (or [N, 28, 28]) in the dataset's range [0, 2] -- HR images or the sampler's output for
    ``min_max_val = (0, 2)`` -- as a tensor or numpy array, ``labels`` [N] the true digits.  Returns
    {'pred': int64 [N], 'accuracy': float, 'confusion': int64 [10, 10] with rows = true digit, columns = predicted}."""
    x = torch.as_tensor(np.asarray(images) if not torch.is_tensor(images) else images).to(torch.float32)
    if x.dim() == 3:
        x = x[:, None]
    y = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).astype(np.int64).reshape(-1)
    if x.dim() != 4 or x.shape[0] != y.shape[0]:
        raise ValueError(f"digit_report: images {tuple(x.shape)} for {y.shape[0]} labels")
    if y.size and (y.min() < 0 or y.max() > 9):
        raise ValueError("digit_report: label outside 0..9")
    dev = next(classifier.parameters()).device
    preds = [classifier.predict(x[i:i + batch_size].to(dev))[0] for i in range(0, x.shape[0], batch_size)]
    pred = torch.cat(preds).cpu().numpy() if preds else np.zeros(0, np.int64)
    confusion = np.zeros((10, 10), np.int64)
    np.add.at(confusion, (y, pred), 1)
    return {"pred": pred, "accuracy": float((pred == y).mean()) if y.size else float("nan"), "confusion": confusion}


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PATCHCORE_RULES = {"8to3": "mnist", "8to5": "mnist", "t12flair": "mri", "flair2t1": "mri", "transistor": "mvtec",
                   "toothbrush": "mvtec", "grid": "mvtec"}


def patchcore_preprocess(lr, data, mean_t1=None, std_t1=None, translate_zero=True):
    """PatchCore's input from the conditioning image lr [B, C, H, W] (test.py:200-238, 243): three channels, then
    * mri: the translate_zero shift undone (lr - |mini|), channel 0 de-normalised (* std_t1 + mean_t1), / 4096, repeated
      to three channels -- as test.py writes it, [B, H, W].repeat(1, 3, 1, 1) is [1, 3B, H, W];
    * mnist / mvtec*: / 2 when max > 1, bilinear resize (align_corners=False) to 84 (mnist) or 224 (mvtec);
    and the ImageNet ``Normalize``.  ``data`` is the config's ``data`` ('mnist', 'mri' or a name containing 'mvtec')."""
    lr_ad = lr.repeat(1, 3, 1, 1) if lr.shape[1] != 3 else lr.clone()
    if data == "mri":
        if mean_t1 is None or std_t1 is None:
            raise ValueError("patchcore_preprocess: mri needs mean_t1 and std_t1")
        if translate_zero:
            mini = (0 - mean_t1) / std_t1
            lr_ad = lr_ad - torch.abs(torch.tensor(mini))
        lr_ad = lr_ad[:, 0] * std_t1 + mean_t1
        lr_ad = lr_ad / 4096.0
        lr_ad = lr_ad.repeat(1, 3, 1, 1)
    elif "mvtec" in data or data == "mnist":
        if lr_ad.shape[1] == 1:
            lr_ad = lr_ad.repeat(1, 3, 1, 1)
        if lr_ad.max() > 1.0:
            lr_ad = lr_ad / 2
        size = 224 if "mvtec" in data else 84
        lr_ad = F.interpolate(lr_ad, size=(size, size), mode="bilinear", align_corners=False)
    else:
        raise ValueError(f"patchcore_preprocess: data {data!r} (mnist, mri or mvtec*)")
    mean = torch.tensor(IMAGENET_MEAN, dtype=lr_ad.dtype, device=lr_ad.device).view(-1, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=lr_ad.dtype, device=lr_ad.device).view(-1, 1, 1)
    return (lr_ad - mean) / std


def patchcore_bank_preprocess(x, data):
    """PatchCore's input when a memory bank is built (anomaly_model_train.py:354-361), which differs from
    ``patchcore_preprocess``: three channels; outside 'mri', / 2 when the max of the whole batch is above 1; bilinear
    resize (align_corners=False) to 224 x 224 in every mode, mnist included; the ImageNet ``Normalize``."""
    x = x.repeat(1, 3, 1, 1) if x.shape[1] != 3 else x
    if data != "mri" and x.max() > 1.0:
        x = x / 2.0
    x = F.interpolate(x, size=(224, 224), mode="bilinear", align_corners=False)
    mean = torch.tensor(IMAGENET_MEAN, dtype=x.dtype, device=x.device).view(-1, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=x.dtype, device=x.device).view(-1, 1, 1)
    return (x - mean) / std


def _pc_threshold(rule, a):
    """(threshold, clip floor) of test.py's branch for ``rule`` on the map a, or None where it falls back to ones."""
    mx = a.max()
    if rule == "8to3":
        if not mx > 37.0:
            return None
        thr = 41.7 if mx > 44 else (38.2 if mx > 40.0 else 35.0)
        return thr, thr - a.std()
    if rule == "8to5":
        if not mx > 58.5:
            return None
        thr = 61.0 if mx > 71.0 else (57.0 if mx > 65 else 55.0)
        return thr, thr - a.std()
    if rule == "t12flair":
        if not mx > 43:
            return None
        thr = mx - 12 if mx > 60 else (47 if mx > 51 else (44 if mx > 48.5 else 42))
        return thr, thr - a.std()
    if rule == "flair2t1":
        if not mx > 43:
            return None
        thr = 47 if mx > 60 else (43 if mx > 50 else 42)
        return thr, thr - a.std()
    if rule == "transistor":
        if not mx > 32:
            return None
        if mx > 40.0:
            thr = 33.5
        elif mx > 36.8:
            thr = mx - 2 * a.std()
        elif mx > 35.0:
            thr = mx - 1 * a.std()
        else:
            thr = 29.5
        return thr, thr - 0.5 * a.std()
    if rule == "toothbrush":
        if not mx > 35:
            return None
        return (40.0 if mx > 49 else 28.0), a.min()
    if rule == "grid":
        if not mx > 27:
            return None
        return (35.0 if mx > 40 else (30.0 if mx > 35.0 else 26.5)), a.min()
    raise ValueError(f"patchcore_ood_mask: rule {rule!r} (one of {sorted(PATCHCORE_RULES)})")


def patchcore_ood_mask(anomaly_map, rule, img_size=None):
    """The reference's OOD mask from a PatchCore anomaly map (test.py:245-375): for the mnist and mvtec rules the map is
    first resized (bilinear, align_corners=False) to img_size x img_size when img_size is given (test.py:245-246); then
    the rule's threshold ladder (mnist '8to3' / '8to5', mri 't12flair' / 'flair2t1', mvtec 'transistor' / 'toothbrush' /
    'grid'), the clip to [floor, threshold] and the squared min-max scaling, or all ones below the rule's first cut.
    Returns (mask_pred, binary_mask) [B, 1, H, W] fp32 on the CPU, as test.py holds them."""
    if rule not in PATCHCORE_RULES:
        raise ValueError(f"patchcore_ood_mask: rule {rule!r} (one of {sorted(PATCHCORE_RULES)})")
    a = anomaly_map.detach().float()
    if img_size is not None and PATCHCORE_RULES[rule] in ("mnist", "mvtec"):
        a = F.interpolate(a, size=(img_size, img_size), mode="bilinear", align_corners=False)
    a = a.cpu()
    cut = _pc_threshold(rule, a)
    if cut is None:
        return torch.ones_like(a), torch.ones_like(a)
    thr, floor = cut
    binary = (a > thr).float()
    m = torch.clip(a, min=floor, max=thr)
    m = (m - m.min()) / (thr - m.min())
    return m ** 2, binary


def print_quality(quality):
    """One line per region of a ``quality`` report (``evaluate(metrics=True)``)."""
    for region in ("all", "ood", "ind"):
        q = quality[region]
        print(f"{region:>3}: MSE {q['mean_mse']:.6f}  PSNR {q['mean_psnr']:.2f} dB  SSIM {q['mean_ssim']:.4f}  "
              f"({q['n_images']} images)")


def evaluate(diffusion, hr, lr, masks, min_max_val, out_dir=None, device="cuda", batch_size=1, metrics=False, data_range=None):
    """test.py's loop: sample every LR image, compare with HR.  Returns a dict of metrics.

    ``metrics=True`` adds ``"quality"``: ``metrics.quality_report`` of the final fused image against ``hr`` over ALL channels,
    with ``masks`` as the region mask (``"all"`` / ``"ood"`` = mask >= 1 / ``"ind"``: per-image ``mse``, ``psnr``, ``ssim``, their
    means and the counts), computed on the device with one read-back at the end, and ``metrics.json`` in ``out_dir``.
    ``data_range`` defaults to ``min_max_val[1] - min_max_val[0]``.  ``test_loss`` keeps the reference's definition -- the LAST
    channel only (test.py:416), a mean of per-batch fp32 means -- so for 3-channel data it is not ``quality["all"]["mse"]``.
    A result that is not one fused [n, C, H, W] image per input (the two-branch layouts) is a ``ValueError`` with it."""
    if metrics:
        from . import metrics as _metrics
        if data_range is None:
            data_range = float(min_max_val[1]) - float(min_max_val[0])
        sums = []
    preds, losses, times = [], [], []
    n = hr.shape[0]
    for i in range(0, n, batch_size):
        sl = slice(i, min(n, i + batch_size))
        cond = lr[sl].to(device)
        mask = None if masks is None else masks[sl].to(device)
        if str(device).startswith("cuda"):
            torch.cuda.synchronize()
        t0 = time.time()
        out = diffusion.sample(cond, hr[sl].to(device), batch_size=cond.shape[0], mask=mask, min_max_val=min_max_val)
        if str(device).startswith("cuda"):
            torch.cuda.synchronize()
        times.append(time.time() - t0)
        if isinstance(out, list):
            out = torch.stack(out)
        if metrics:
            if out.dim() != 4 or out.shape[0] != cond.shape[0]:
                raise ValueError(f"evaluate(metrics=True): the sampler returned {tuple(out.shape)}, not one fused image per input")
            sums.append(_metrics.quality_sums(out.detach().to(torch.float32), hr[sl].to(device, torch.float32),
                                              None if mask is None else mask.to(torch.float32), data_range=data_range))
        out = out.detach().cpu()
        losses.append(float(torch.nn.functional.mse_loss(out[..., [-1], :, :] if out.dim() == 4 else out[-1][:, [-1]],
                                                         hr[sl][:, [-1]])))
        preds.append(out.numpy())
    res = {"test_loss": float(np.mean(losses)), "avg_sampling_time": float(np.mean(times)),
           "n": n, "pred": np.concatenate(preds) if preds[0].ndim == 4 else np.stack(preds)}
    if metrics:
        res["quality"] = _metrics.report_from_sums(torch.cat(sums).cpu().numpy(), data_range)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(out_dir, "hr_all.npy"), hr.numpy())
        np.save(os.path.join(out_dir, "lr_all.npy"), lr.numpy())
        np.save(os.path.join(out_dir, "pred_all.npy"), res["pred"])
        if masks is not None:
            np.save(os.path.join(out_dir, "ad_masks.npy"), masks.numpy())
        if metrics:
            import json
            with open(os.path.join(out_dir, "metrics.json"), "w") as f:
                json.dump(dict(_metrics.report_to_json(res["quality"]), test_loss=res["test_loss"], n=n), f, indent=1)
    return res
