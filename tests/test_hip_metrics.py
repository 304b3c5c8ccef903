"""GPU tests of csrc/metrics.hip (``ld_metric_sums``) and ``metrics.quality_sums`` / ``quality_report``.

Yardstick: tests/metrics_ref.py's fp64 statement of the definition (``sums64``; proved against a direct 11 x 11 evaluation in
tests/test_metrics_ref.py).  Counts are exact, ``sse`` is within 1e-12 relative, and the per-image SSIM of every region that
has windows is within ``2 * metrics_ref.D_SSIM``: ``D_SSIM`` is the largest distance of the fp32 restatement in the kernel's
order from the yardstick over these same inputs, measured on the CPU by
tests/test_metrics_ref.py::test_measured_distance_of_the_restatement; the kernel follows the restatement's order, and the
factor 2 leaves room for a different but equivalent instruction choice.  The bitwise properties use ``torch.equal``."""
import gzip
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import metrics

from hip_helpers import DEV, NAN, st
import metrics_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
CANARY, PAD = 7.5, 32


def gpu_sums(pred, ref, mask, L):
    return metrics.quality_sums(pred.to(DEV), ref.to(DEV), None if mask is None else mask.to(DEV), data_range=L).cpu()


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_fp64_yardstick(shape):
    """Every data range and mask of the case list at one shape: counts exact, sse to 1e-12 relative, per-image SSIM per region
    to 2 D_SSIM."""
    worst_ssim, worst_sse = 0.0, 0.0
    for L in R.RANGES:
        pred, ref = R.images(shape, L)
        for kind in R.MASKS:
            mask = R.make_mask(kind, shape)
            want = R.sums64(pred, ref, mask, L)
            got = gpu_sums(pred, ref, mask, L)
            have = want[:, :, 2] > 0
            d = float((R.per_image_ssim(got) - R.per_image_ssim(want))[have].abs().max())
            e = float(((got[:, :, 1] - want[:, :, 1]).abs() / want[:, :, 1].clamp_min(1e-300))[want[:, :, 0] > 0].max())
            worst_ssim, worst_sse = max(worst_ssim, d), max(worst_sse, e)
            print(f"{shape} L {L} mask {kind}: per-image SSIM distance {d:.3e} (bound {2 * R.D_SSIM:.2e}), sse relative {e:.2e}")
            assert torch.equal(got[:, :, 0], want[:, :, 0]) and torch.equal(got[:, :, 2], want[:, :, 2]), (L, kind)
            assert R.passes(got, want), (L, kind, d, e)
            if mask is None:
                assert torch.equal(got[:, 1:], torch.zeros(shape[0], 2, 4, dtype=F64))
            else:                                  # regions 1 and 2 add up to region 0 in the two integer fields
                assert torch.equal(got[:, 1, 0] + got[:, 2, 0], got[:, 0, 0]) and torch.equal(got[:, 1, 2] + got[:, 2, 2], got[:, 0, 2])
    print(f"{shape}: worst per-image SSIM distance {worst_ssim:.3e}, worst sse relative {worst_sse:.2e}")


def test_two_runs_and_a_sample_alone_give_the_same_bits():
    """(3, 3, 43, 45): two runs agree bit for bit; sample b evaluated alone -- its planes then start 4 and 8 bytes off the
    16-byte grid for b = 1, 2, so the element-load path runs -- equals sample b inside the batch of 3."""
    shape, L = (3, 3, 43, 45), 2.0
    pred, ref = (t.to(DEV) for t in R.images(shape, L))
    mask = R.make_mask("rect", shape).to(DEV)
    mask[1] = torch.roll(mask[1], 7, dims=-1)
    a = metrics.quality_sums(pred, ref, mask, data_range=L)
    b = metrics.quality_sums(pred, ref, mask, data_range=L)
    assert torch.equal(a, b)
    assert len({float(v) for v in a[:, 0, 3]}) == 3                  # (the samples differ: equality below says something)
    for i in range(3):
        alone_view = metrics.quality_sums(pred[i:i + 1], ref[i:i + 1], mask[i:i + 1], data_range=L)
        alone_copy = metrics.quality_sums(pred[i:i + 1].clone(), ref[i:i + 1].clone(), mask[i:i + 1].clone(), data_range=L)
        assert pred[i:i + 1].data_ptr() % 16 == (4 * 5805 * i) % 16
        assert torch.equal(alone_view[0], a[i]) and torch.equal(alone_copy[0], a[i]), i
    nomask = metrics.quality_sums(pred, ref, None, data_range=L)
    assert torch.equal(nomask[:, 0], a[:, 0])


def test_the_call_alone_between_canaries():
    """``ld_metric_sums`` itself: ``out`` and ``work`` sit between canaries that stay, every word in between is written, the work
    size is what ``ld_metric_work_doubles`` says, and a refusal on the device leaves both buffers alone."""
    lib = cabi.lib()
    shape, L = (2, 3, 43, 45), 1.0
    B, Cc, H, W = shape
    pred, ref = (t.to(DEV) for t in R.images(shape, L))
    mask = R.make_mask("rect", shape).to(DEV)
    n_work = int(lib.ld_metric_work_doubles(*shape))
    assert n_work == B * Cc * 4 * 12
    out = torch.full((2 * PAD + B * 12,), CANARY, dtype=F64, device=DEV)
    work = torch.full((2 * PAD + n_work,), CANARY, dtype=F64, device=DEV)
    out[PAD:-PAD], work[PAD:-PAD] = NAN, NAN
    args = (pred.data_ptr(), ref.data_ptr(), mask.data_ptr(), work.data_ptr() + 8 * PAD, out.data_ptr() + 8 * PAD, B, Cc, H, W)
    assert lib.ld_metric_sums(*args[:6], Cc, H, 10, L, st()) == -1 and b"window" in lib.ld_last_error()
    assert lib.ld_metric_sums(*args, 0.0, st()) == -1 and b"data_range" in lib.ld_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[PAD:-PAD]).all()) and bool(torch.isnan(work[PAD:-PAD]).all())
    cabi.check(lib.ld_metric_sums(*args, L, st()), "metric_sums")
    torch.cuda.synchronize()
    for buf in (out, work):
        assert bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all())
        assert bool(torch.isfinite(buf[PAD:-PAD]).all())
    got = out[PAD:-PAD].view(B, 3, 4).cpu()
    assert R.passes(got, R.sums64(pred.cpu(), ref.cpu(), mask.cpu(), L))
    # the second launch's order: a sample's partial sums added in (channel, tile row, tile column) order
    parts = work[PAD:-PAD].view(B, Cc * 4, 12).cpu()
    acc = torch.zeros(B, 12, dtype=F64)
    for i in range(Cc * 4):
        acc = acc + parts[:, i]
    assert torch.equal(acc.view(B, 3, 4), got)


def test_report_on_identical_tensors_and_no_wait():
    """``quality_report`` on identical tensors: SSIM exactly 1.0 and an infinite PSNR in every region that is not empty; and
    ``quality_sums`` does not wait for the GPU (``set_sync_debug_mode('error')``: a lone ``.item()`` raises, the call does not)."""
    shape, L = (2, 3, 43, 45), 2.0
    x = R.images(shape, L)[0].to(DEV)
    mask = R.make_mask("rect", shape).to(DEV)
    rep = metrics.quality_report(x, x.clone(), mask, data_range=L)
    for region in metrics.REGIONS:
        d = rep[region]
        assert np.all(d["n_win"] > 0) and np.all(d["ssim"] == 1.0) and np.all(np.isinf(d["psnr"])) and np.all(d["mse"] == 0.0)
        assert d["mean_ssim"] == 1.0 and d["n_images"] == 2
    rep = metrics.quality_report(x, x.clone(), None, data_range=L)
    assert np.all(rep["all"]["ssim"] == 1.0) and np.all(np.isnan(rep["ood"]["ssim"])) and rep["ind"]["n_images"] == 0
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        with pytest.raises(RuntimeError):
            probe.item()
        sums = metrics.quality_sums(x, x, mask, data_range=L)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert sums.dtype == F64 and tuple(sums.shape) == (2, 3, 4) and sums.device.type == "cuda"


def _write_idx(path, arr):
    hdr = struct.pack(">HBB", 0, 0x08, arr.ndim) + struct.pack(">" + "I" * arr.ndim, *arr.shape)
    with (gzip.open if str(path).endswith(".gz") else open)(path, "wb") as f:
        f.write(hdr + arr.astype(np.uint8).tobytes())


def test_run_eval_tool_writes_metrics_json(tmp_path):
    """``tools/run_eval.py --metrics`` on golden MNIST digits (a fresh process): ``metrics.json`` holds the three regions, and on
    this single-channel data the mean ``"all"`` MSE is ``test_loss`` -- a mean of per-image fp32 means of 784 squares against
    fp64 sums, so within the (n - 1) 2^-24 bound of an fp32 sum, held here at the 2e-4 of the sharded evaluation's tests."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "g20_mnist_digits.npz"))
    _write_idx(tmp_path / "images.idx3-ubyte.gz", d["images"][:64])
    _write_idx(tmp_path / "labels.idx1-ubyte", d["labels"][:64])
    digit = int(np.bincount(d["labels"][:64]).argmax())
    out_dir = tmp_path / "out"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_eval.py"), "--images", str(tmp_path / "images.idx3-ubyte.gz"),
                          "--labels", str(tmp_path / "labels.idx1-ubyte"), "--digit", str(digit), "--n", "2", "--timesteps", "4",
                          "--out", str(out_dir), "--metrics"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "Test loss" in run.stdout and "PSNR" in run.stdout and "ood" in run.stdout
    rep = json.load(open(out_dir / "metrics.json"))
    assert rep["n"] == 2 and rep["data_range"] == 2.0 and all(len(rep[r]["mse"]) == 2 for r in metrics.REGIONS)
    assert rep["all"]["n_elem"] == [784, 784] and rep["ood"]["n_elem"] == [28 * 7] * 2 and rep["ind"]["n_elem"] == [28 * 21] * 2
    assert rep["all"]["n_win"] == [18 * 18] * 2 and rep["ood"]["n_win"] == [18 * 2] * 2          # centres in columns 5, 6
    loss, mse = rep["test_loss"], rep["all"]["mean_mse"]
    print(f"run_eval.py: test_loss {loss!r}, mean all-region MSE {mse!r} (relative {abs(loss - mse) / mse:.2e})")
    assert abs(loss - mse) <= 2e-4 * mse
    for name in ("hr_all.npy", "lr_all.npy", "pred_all.npy", "ad_masks.npy"):
        assert (out_dir / name).exists()
    # the report restated from the files the reference's script leaves (pred_all / hr_all / ad_masks): the fp32 restatement in
    # the kernel's order has the kernel's value per window, so only the order of the fp64 sums is left (D_SSIM was measured on
    # other inputs and does not apply to these images)
    pred, hr, masks = (torch.from_numpy(np.load(out_dir / n)) for n in ("pred_all.npy", "hr_all.npy", "ad_masks.npy"))
    want = metrics.report_from_sums(R.sums32(pred, hr, masks, 2.0).numpy(), 2.0)
    for region in metrics.REGIONS:
        d = np.abs(np.array(rep[region]["ssim"]) - want[region]["ssim"]).max()
        print(f"run_eval.py {region}: SSIM {rep[region]['ssim']} against the restatement's, distance {d:.2e}")
        assert np.allclose(rep[region]["mse"], want[region]["mse"], rtol=1e-12, atol=0.0)
        assert d <= 1e-9
