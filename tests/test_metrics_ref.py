"""tests/metrics_ref.py proved on the CPU, and everything of the quality metrics that needs no GPU: the fp64 yardstick against
a direct 11 x 11 evaluation, the exact properties of the fp32 restatement, the region rules, the mutation check, the measured
distance ``d`` that tests/test_hip_metrics.py takes its SSIM bound from, ``ld_metric_sums``'s refusals through the library,
``quality_sums``'s ``ValueError``s, the report's quotients, and the host half of ``DenoiserTrainer.evaluate(sharded=True)``."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import metrics
from localdiffusion_hallucination_amd.denoiser_train import sharded_eval_loss
from localdiffusion_hallucination_amd.dist import shard_bounds

import metrics_ref as R

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------ the references
def test_taps_are_the_library_s():
    """The window: normalised in double, rounded once; the library's host-side taps have the same bits."""
    got = (C.c_float * 11)()
    assert cabi.lib().ld_metric_taps(got) == 0
    assert np.array_equal(np.frombuffer(got, dtype=np.float32).view(np.uint32), R.taps32().view(np.uint32))
    assert abs(R.taps64().sum() - 1.0) < 1e-15 and np.array_equal(R.taps32(), R.taps32()[::-1])


def test_yardstick_against_a_direct_evaluation():
    """A 13 x 14 image: 3 x 4 windows, each written out as a sum over its 121 pixels in numpy fp64."""
    for L in R.RANGES:
        pred, ref = R.images((1, 1, 13, 14), L)
        got = R.ssim_map64(pred, ref, L)[0, 0].numpy()
        want = R.direct_ssim_map(pred[0, 0].numpy(), ref[0, 0].numpy(), L)
        assert got.shape == want.shape == (3, 4)
        assert np.abs(got - want).max() <= 1e-12


def test_identical_images_are_exactly_one():
    """x == y: 2 mu mu == mu^2 + mu^2 and 2 sxy == sx + sy bit for bit in fp32, so every window's SSIM is exactly 1.0;
    sse is 0 and the PSNR infinite."""
    for shape in R.SHAPES:
        for L in R.RANGES:
            x, _ = R.images(shape, L)
            assert torch.equal(R.ssim_map32(x, x.clone(), L), torch.ones(shape[0], shape[1], shape[2] - 10, shape[3] - 10))
            t = R.sums32(x, x.clone(), R.make_mask("rect", shape), L)
            assert torch.equal(t[:, :, 3], t[:, :, 2]) and torch.equal(t[:, :, 1], torch.zeros(shape[0], 3, dtype=F64))
            rep = metrics.report_from_sums(t.numpy(), L)
            for region in metrics.REGIONS:
                d = rep[region]
                assert np.all(d["n_elem"] > 0) and np.all(np.isinf(d["psnr"])) and np.all(d["mse"] == 0) and d["mean_psnr"] == math.inf
                if shape[2:] == (11, 11) and region == "ind":          # the one window's centre lies in the rectangle
                    assert np.all(d["n_win"] == 0) and np.all(np.isnan(d["ssim"]))
                else:
                    assert np.all(d["n_win"] > 0) and np.all(d["ssim"] == 1.0) and d["mean_ssim"] == 1.0


def test_empty_regions_are_nan_with_zero_counts():
    shape, L = (2, 3, 43, 45), 2.0
    pred, ref = R.images(shape, L)
    for kind, empty in (("none", ("ood", "ind")), ("zeros", ("ood",)), ("ones", ("ind",))):
        t = R.sums64(pred, ref, R.make_mask(kind, shape), L)
        rep = metrics.report_from_sums(t.numpy(), L)
        for region in metrics.REGIONS:
            d = rep[region]
            if region in empty:
                assert np.all(d["n_elem"] == 0) and np.all(d["n_win"] == 0) and d["n_images"] == 0
                assert all(np.all(np.isnan(d[k])) for k in ("mse", "psnr", "ssim"))
                assert all(math.isnan(d["mean_" + k]) for k in ("mse", "psnr", "ssim"))
            else:
                assert np.all(d["n_elem"] == 3 * 43 * 45) and np.all(d["n_win"] == 3 * 33 * 35) and d["n_images"] == 2
                assert np.array_equal(d["mse"], rep["all"]["mse"]) and np.array_equal(d["ssim"], rep["all"]["ssim"])
    # an image whose region is empty is left out of that region's mean
    mask = R.make_mask("zeros", shape)
    mask[1, 0, 20:30, 20:30] = 1.0
    rep = metrics.report_from_sums(R.sums64(pred, ref, mask, L).numpy(), L)
    assert rep["ood"]["n_images"] == 1 and math.isnan(rep["ood"]["ssim"][0]) and rep["ood"]["mean_ssim"] == rep["ood"]["ssim"][1]
    assert rep["ood"]["mean_psnr"] == rep["ood"]["psnr"][1] == pytest.approx(10.0 * math.log10(L * L / rep["ood"]["mse"][1]), rel=1e-14)


def test_a_window_belongs_to_the_region_of_its_centre():
    """A one-pixel mask at (y, x): the OOD region has C elements; it has C windows -- the ones whose centre is (y, x), with the
    map's values at (y - 5, x - 5) -- when a whole window fits around the pixel, and none otherwise."""
    shape, L = (1, 3, 43, 45), 1.0
    pred, ref = R.images(shape, L)
    smap = R.ssim_map64(pred, ref, L)
    for (y, x), inside in (((5, 5), True), ((37, 39), True), ((20, 9), True), ((4, 20), False), ((38, 20), False), ((20, 40), False),
                           ((0, 0), False)):
        mask = torch.zeros(1, 1, 43, 45)
        mask[0, 0, y, x] = 1.0
        for t in (R.sums64(pred, ref, mask, L), R.sums32(pred, ref, mask, L)):
            assert t[0, 1, 0] == 3 and t[0, 2, 0] == 3 * 43 * 45 - 3
            assert t[0, 1, 2] == (3 if inside else 0) and t[0, 1, 2] + t[0, 2, 2] == t[0, 0, 2] == 3 * 33 * 35
        if inside:
            want = float(smap[0, :, y - 5, x - 5].sum())
            assert abs(float(R.sums64(pred, ref, mask, L)[0, 1, 3]) - want) <= 1e-12


# ------------------------------------------------------------------------------------------------ d and the mutation check
def _distance(a, b):
    have = b[:, :, 2] > 0
    return float((R.per_image_ssim(a) - R.per_image_ssim(b))[have].abs().max())


@pytest.fixture(scope="module")
def cases():
    out = []
    for shape, L, kind in R.case_list():
        pred, ref = R.images(shape, L)
        mask = R.make_mask(kind, shape)
        out.append((shape, L, kind, pred, ref, mask, R.sums64(pred, ref, mask, L)))
    return out


def test_measured_distance_of_the_restatement(cases):
    """The fp32 restatement's own distance from the yardstick over the GPU test's inputs: the largest per-image SSIM
    difference and the largest relative sse difference.  metrics_ref.D_SSIM / D_SSE_REL are these figures rounded up."""
    d_ssim, d_sse, where = 0.0, 0.0, None
    for shape, L, kind, pred, ref, mask, want in cases:
        got = R.sums32(pred, ref, mask, L)
        assert torch.equal(got[:, :, 0], want[:, :, 0]) and torch.equal(got[:, :, 2], want[:, :, 2])
        d = _distance(got, want)
        if d > d_ssim:
            d_ssim, where = d, (shape, L, kind)
        nz = want[:, :, 1] > 0
        d_sse = max(d_sse, float(((got[:, :, 1] - want[:, :, 1]).abs()[nz] / want[:, :, 1][nz]).max()))
        assert R.passes(got, want)
    print(f"fp32 restatement against the fp64 yardstick: per-image SSIM d = {d_ssim:.4e} at {where}; sse relative {d_sse:.2e}")
    assert d_ssim <= R.D_SSIM <= 1.25 * d_ssim
    assert d_sse <= R.D_SSE_REL <= 1e-12


@pytest.mark.parametrize("mutant", [dict(sigma=1.0), dict(unbiased=True), dict(pad=True)], ids=["sigma1", "unbiased", "padded"])
def test_mutants_fall_outside_the_gpu_tolerance(cases, mutant):
    """A restatement with another sigma, with sample (co)variances or with zero-padded borders fails the GPU test's own
    comparison (metrics_ref.passes) on every one of its cases."""
    for shape, L, kind, pred, ref, mask, want in cases:
        assert not R.passes(R.sums32(pred, ref, mask, L, **mutant), want), (shape, L, kind)


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def test_metric_sums_refusals_need_no_gpu():
    """Every refusal returns -1 with the error text set and leaves ``out`` alone; nothing is launched (there is no GPU here to
    launch on, and the image pointers are never read)."""
    lib = cabi.lib()
    out = (C.c_double * 16)(*([7.5] * 16))
    work = (C.c_double * 64)(*([7.5] * 64))
    img = (C.c_float * 4)()
    p, o, w = C.addressof(img), C.addressof(out), C.addressof(work)
    good = dict(pred=p, ref=p, mask=None, work=w, out=o, B=1, C=1, H=11, W=11, L=1.0)
    bad = [("null", dict(pred=None)), ("null", dict(ref=None)), ("null", dict(work=None)), ("null", dict(out=None)),
           ("at least 1", dict(B=0)), ("at least 1", dict(C=0)), ("at least 1", dict(H=0)), ("at least 1", dict(W=-3)),
           ("window", dict(H=10)), ("window", dict(W=10)),
           ("data_range", dict(L=0.0)), ("data_range", dict(L=-1.0)), ("data_range", dict(L=math.inf)), ("data_range", dict(L=math.nan)),
           ("8-byte", dict(out=o + 4)), ("8-byte", dict(work=w + 4))]
    for text, change in bad:
        a = dict(good, **change)
        rc = lib.ld_metric_sums(a["pred"], a["ref"], a["mask"], a["work"], a["out"], a["B"], a["C"], a["H"], a["W"], a["L"], None)
        assert rc == -1 and text.encode() in lib.ld_last_error(), (change, lib.ld_last_error())
        assert list(out) == [7.5] * 16 and list(work) == [7.5] * 64, change
    assert int(lib.ld_metric_work_doubles(1, 1, 11, 11)) == 12
    assert int(lib.ld_metric_work_doubles(2, 3, 43, 45)) == 2 * 3 * 2 * 2 * 12
    assert int(lib.ld_metric_work_doubles(1, 1, 75, 33)) == 3 * 12
    for shape in ((0, 1, 11, 11), (1, 0, 11, 11), (1, 1, 10, 11), (1, 1, 11, 10), (1 << 20, 1 << 10, 75, 75)):
        assert int(lib.ld_metric_work_doubles(*shape)) == 0, shape


def test_quality_sums_value_errors():
    x = torch.zeros(2, 1, 28, 28)
    m = torch.zeros(2, 1, 28, 28)
    bad = [dict(ref=torch.zeros(2, 1, 28, 27)), dict(ref=torch.zeros(1, 1, 28, 28)), dict(pred=x[0], ref=x[0]),
           dict(ref=x.double()), dict(pred=x.half(), ref=x.half()), dict(mask=m.bool()), dict(mask=m[:, 0]), dict(mask=m[:1]),
           dict(mask=torch.zeros(2, 3, 28, 28)), dict(pred=torch.zeros(2, 1, 10, 28), ref=torch.zeros(2, 1, 10, 28), mask=None),
           dict(pred=torch.zeros(2, 1, 28, 10), ref=torch.zeros(2, 1, 28, 10), mask=None),
           dict(pred=torch.zeros(0, 1, 28, 28), ref=torch.zeros(0, 1, 28, 28), mask=None),
           dict(data_range=0.0), dict(data_range=-2.0), dict(data_range=math.nan), dict(data_range=math.inf), dict(data_range=None),
           dict(data_range=True), dict(data_range=1e39), dict(ref=x.numpy()), dict(ref=x.to("meta"))]
    for change in bad:
        a = dict(dict(pred=x, ref=x, mask=m, data_range=2.0), **change)
        with pytest.raises(ValueError):
            metrics.quality_sums(a["pred"], a["ref"], a["mask"], data_range=a["data_range"])
    with pytest.raises(TypeError):
        metrics.quality_sums(x, x, m)                                   # data_range is required
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):                  # valid arguments on the CPU: no fallback
            metrics.quality_sums(x, x, m, data_range=2.0)
    assert ldh.quality_sums is metrics.quality_sums and ldh.quality_report is metrics.quality_report and ldh.metrics is metrics


def test_report_quotients():
    sums = np.zeros((2, 3, 4))
    sums[0, 0] = [100, 4.0, 10, 5.0]
    sums[1, 0] = [100, 1.0, 10, 9.0]
    sums[1, 1] = [40, 0.0, 4, 4.0]
    sums[1, 2] = [60, 1.0, 6, 5.0]
    rep = metrics.report_from_sums(sums, 2.0)
    assert rep["all"]["mse"].tolist() == [0.04, 0.01] and rep["all"]["ssim"].tolist() == [0.5, 0.9]
    assert rep["all"]["psnr"].tolist() == pytest.approx([20.0, 10 * math.log10(400.0)], rel=1e-14)
    assert rep["all"]["mean_mse"] == np.mean([0.04, 0.01]) and rep["all"]["n_images"] == 2
    assert math.isnan(rep["ood"]["mse"][0]) and rep["ood"]["psnr"][1] == math.inf and rep["ood"]["mean_ssim"] == 1.0
    assert rep["ind"]["n_elem"].tolist() == [0, 60] and rep["ind"]["n_win"].dtype == np.int64
    import json
    json.dumps(metrics.report_to_json(rep))


# ------------------------------------------------------------------------------------------------ the sharded evaluation's host half
SIZES = (3, 2)


def _tables(world, plant=None):
    """Hand-made gathered tables for test batches of 3 and 2 rows: rank r's copy holds (sse, n_elem) of its own rows and
    ``plant`` (zeros as ``evaluate_local`` leaves them, or a decoy) everywhere else."""
    rows = sum(SIZES)
    sse = np.array([0.1, 0.7, 1e-3, 3.0, 0.25])                     # (not symmetric: another row or batch order shows)
    cnt = np.array([784.0] * 3 + [784.0] * 2)
    g = np.zeros((world, rows, 2)) if plant is None else np.full((world, rows, 2), plant)
    at = 0
    for size in SIZES:
        for r in range(world):
            lo, hi = shard_bounds(size, world, r)
            g[r, at + lo:at + hi, 0] = sse[at + lo:at + hi]
            g[r, at + lo:at + hi, 1] = cnt[at + lo:at + hi]
        at += size
    return g, sse, cnt


@pytest.mark.parametrize("world", [1, 2, 3])
def test_sharded_eval_host_half(world):
    """Worlds 1, 2 and 3 over batches of 3 and 2 rows (ragged at world 2; at world 3 rank 2 has no row of the second batch):
    each row comes from its owner's copy, rows are added in row order, batches in batch order, and what a non-owner's copy
    holds in a slot is ignored."""
    g, sse, cnt = _tables(world)
    want = (((sse[0] + sse[1]) + sse[2]) / ((cnt[0] + cnt[1]) + cnt[2]) + (sse[3] + sse[4]) / (cnt[3] + cnt[4])) / 2
    assert sharded_eval_loss(g, SIZES, world) == want
    if world == 3:
        assert shard_bounds(2, 3, 2) == (2, 2)                       # the idle rank
    # decoys in every slot a rank does not own: the same float
    decoy, _, _ = _tables(world, plant=1e6)
    assert sharded_eval_loss(decoy, SIZES, world) == want
    # a value planted in the OWNER's slot does move the result (the selection looks where it should)
    moved = g.copy()
    owner_of_row4 = [r for r in range(world) if shard_bounds(2, world, r)[0] <= 1 < shard_bounds(2, world, r)[1]][0]
    moved[owner_of_row4, 4, 0] += 1.0
    assert sharded_eval_loss(moved, SIZES, world) != want
    # the order is the documented one: fed rows whose fp64 sum depends on the order
    tricky = g.copy()
    vals = [1.0, 2.0 ** -53, 2.0 ** -53]
    for i, v in enumerate(vals):
        for r in range(world):
            lo, hi = shard_bounds(3, world, r)
            if lo <= i < hi:
                tricky[r, i, 0] = v
    got = sharded_eval_loss(tricky, SIZES, world)
    assert got == (((1.0 + 2.0 ** -53) + 2.0 ** -53) / (3 * 784.0) + (sse[3] + sse[4]) / (2 * 784.0)) / 2
    assert (1.0 + 2.0 ** -53) + 2.0 ** -53 != 1.0 + (2.0 ** -53 + 2.0 ** -53)
    for bad in (g[:, :4], g.astype(np.float32), g[0]):
        with pytest.raises(ValueError):
            sharded_eval_loss(bad, SIZES, world)
    with pytest.raises(ValueError):
        sharded_eval_loss(g, (), world)
