"""Image-quality metrics on the device: MSE, PSNR and SSIM per image, over the whole image and inside / outside a region mask.

The paper's claim is restoration inside the out-of-distribution (OOD) region without loss in the in-distribution (IND)
region, reported as PSNR and SSIM per region; the reference stops at ``hr_all / pred_all / ad_masks .npy``.  ``quality_sums``
is the HIP kernel (``ld_metric_sums``, include/localdiff_hip.h: the definitions live there); ``quality_report`` is its one
read-back and the quotients.

Regions: ``"all"``; ``"ood"`` = ``mask >= 1`` (``ld_recompose``'s convention); ``"ind"`` = the rest.  An element belongs to the
region of its own pixel, an SSIM window (11 x 11 Gaussian, sigma 1.5, no padding) to the region of its centre pixel.  Not
covered: MS-SSIM, LPIPS, FID, padded-border SSIM variants, the unfused two-branch result layouts.
"""
import math

import numpy as np
import torch

from . import _cabi as cabi

REGIONS = ("all", "ood", "ind")
FIELDS = ("n_elem", "sse", "n_win", "ssim_sum")
WINDOW = 11
FLT_MAX = 3.4028234663852886e38          # data_range travels as a C float


def _check(pred, ref, mask, data_range):
    """Everything ``quality_sums`` refuses, before any GPU call."""
    for name, t in (("pred", pred), ("ref", ref)) + ((("mask", mask),) if mask is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"quality_sums: {name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"quality_sums: {name} must be float32, got {t.dtype}")
        if t.device != pred.device:
            raise ValueError(f"quality_sums: {name} is on {t.device}, pred on {pred.device}")
    if pred.dim() != 4 or tuple(ref.shape) != tuple(pred.shape):
        raise ValueError(f"quality_sums: pred {tuple(pred.shape)} and ref {tuple(ref.shape)} must be the same [B, C, H, W]")
    B, C, H, W = (int(s) for s in pred.shape)
    if B < 1 or C < 1:
        raise ValueError(f"quality_sums: empty batch or no channels: {tuple(pred.shape)}")
    if H < WINDOW or W < WINDOW:
        raise ValueError(f"quality_sums: H {H}, W {W}: the {WINDOW} x {WINDOW} SSIM window does not fit")
    if mask is not None and tuple(mask.shape) != (B, 1, H, W):
        raise ValueError(f"quality_sums: mask {tuple(mask.shape)} must be [{B}, 1, {H}, {W}]")
    if isinstance(data_range, bool) or not isinstance(data_range, (int, float)) or not math.isfinite(data_range) \
            or data_range <= 0 or data_range > FLT_MAX:
        raise ValueError(f"quality_sums: data_range {data_range!r} must be a finite positive number")
    return B, C, H, W


def quality_sums(pred, ref, mask=None, *, data_range):
    """``ld_metric_sums``: float64 ``[B, 3, 4]`` on the device -- regions ``REGIONS`` by fields ``FIELDS`` -- for fp32 NCHW
    ``pred`` and ``ref`` and an optional ``[B, 1, H, W]`` fp32 region mask.  Does not wait for the GPU.  ``ValueError`` before
    any GPU call: device, dtype or shape mismatches, ``H`` or ``W`` below 11, a ``data_range`` that is not finite and positive.
    Sample ``b``'s row has the same bits whatever the batch around it."""
    B, C, H, W = _check(pred, ref, mask, data_range)
    dev = pred.device
    if dev.type != "cuda":
        raise RuntimeError("quality_sums runs on the GPU (ld_metric_sums); there is no CPU fallback")
    lib = cabi.lib()
    n_work = int(lib.ld_metric_work_doubles(B, C, H, W))
    if n_work <= 0:
        raise ValueError(f"quality_sums: shape {tuple(pred.shape)} is refused by ld_metric_sums")
    pred, ref = pred.contiguous(), ref.contiguous()
    mask = None if mask is None else mask.contiguous()
    with torch.cuda.device(dev):
        work = torch.empty(n_work, dtype=torch.float64, device=dev)
        out = torch.empty(B, len(REGIONS), len(FIELDS), dtype=torch.float64, device=dev)
        cabi.check(lib.ld_metric_sums(pred.data_ptr(), ref.data_ptr(), cabi.ptr(mask), work.data_ptr(), out.data_ptr(), B, C, H, W,
                                      float(data_range), torch.cuda.current_stream(dev).cuda_stream), "metric_sums")
    return out


def report_from_sums(sums, data_range):
    """The quotients of a ``[B, 3, 4]`` table of sums (numpy float64, on the host): per region a dict of per-image arrays
    ``mse = sse / n_elem``, ``psnr = 10 log10(L^2 / mse)`` (``inf`` at ``mse == 0``), ``ssim = ssim_sum / n_win`` -- ``nan``
    where the region is empty in that image -- the counts ``n_elem`` / ``n_win`` (int64), and ``mean_mse`` / ``mean_psnr`` /
    ``mean_ssim`` over the images whose region is not empty (``nan`` when there is none), with ``n_images`` of them."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 3 or sums.shape[1:] != (len(REGIONS), len(FIELDS)):
        raise ValueError(f"report_from_sums: sums {sums.shape} must be [B, {len(REGIONS)}, {len(FIELDS)}]")
    L2 = float(data_range) ** 2
    rep = {"data_range": float(data_range)}
    for r, region in enumerate(REGIONS):
        n_elem, sse, n_win, ssim_sum = (sums[:, r, f] for f in range(len(FIELDS)))
        with np.errstate(divide="ignore", invalid="ignore"):
            mse = np.where(n_elem > 0, sse / n_elem, np.nan)
            psnr = np.where(mse == 0, np.inf, 10.0 * np.log10(L2 / mse))
            ssim = np.where(n_win > 0, ssim_sum / n_win, np.nan)
        d = {"mse": mse, "psnr": psnr, "ssim": ssim, "n_elem": n_elem.astype(np.int64), "n_win": n_win.astype(np.int64)}
        for key, n in (("mse", n_elem), ("psnr", n_elem), ("ssim", n_win)):
            have = n > 0
            d["mean_" + key] = float(np.mean(d[key][have])) if have.any() else float("nan")
        d["n_images"] = int((n_elem > 0).sum())
        rep[region] = d
    return rep


def quality_report(pred, ref, mask=None, *, data_range):
    """``quality_sums`` and ONE read-back: ``{"all": ..., "ood": ..., "ind": ..., "data_range": L}`` as ``report_from_sums``
    lays it out.  Without a mask the ``"ood"`` and ``"ind"`` regions are empty."""
    return report_from_sums(quality_sums(pred, ref, mask, data_range=data_range).cpu().numpy(), data_range)


def report_to_json(rep):
    """A ``quality_report`` as plain lists and floats (``metrics.json``); non-finite values become ``NaN`` / ``Infinity``
    as Python's ``json`` writes them."""
    def plain(v):
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        if isinstance(v, np.ndarray):
            return v.tolist()
        return v
    return plain(rep)
