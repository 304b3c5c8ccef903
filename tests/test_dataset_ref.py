"""CPU tests of the data path's yardsticks (tests/dataset_ref.py) and of ``BatchSource``: the restatements agree with what the
repository already pins (``evalio.mnist_pairs``), the two forms of the rotation agree on the screened angles, the screen keeps
enough of its candidates, and a step's plan is a pure function of ``(seed, step)``.  No GPU, no reference tree."""
import numpy as np
import pytest
import torch

from localdiffusion_hallucination_amd import evalio, rng
from localdiffusion_hallucination_amd.dataset import BatchSource, DeviceDataset, cos_sin, crop_offset, table_rows

import dataset_ref as D

SIZES = (16, 28)


def u8(shape, key):
    return (rng.bits64(int(np.prod(shape)), 77, key) >> np.uint64(56)).astype(np.uint8).reshape(shape)


def f32(shape, key, lo=0.0, hi=4096.0):
    return rng.uniform(shape, 77, key, lo, hi)


def test_mnist_restatement_is_mnist_pairs():
    store = u8((5, 28, 28), 1)
    hr, lr = D.mnist_batch(store, list(range(5)))
    want_hr, want_lr = evalio.mnist_pairs(store)
    assert hr.shape == (5, 1, 28, 28) and torch.equal(hr, want_hr) and torch.equal(lr, want_lr)


@pytest.mark.parametrize("S", SIZES)
def test_the_screen_keeps_most_candidates(S):
    kept = D.screened_angles(S, S)
    print(f"{S}^2: kept {len(kept)} of {len(D.CANDIDATE_ANGLES)}; margins "
          + " ".join(f"{a:g}:{D.tie_margin(a, S, S):.1e}" for a in D.CANDIDATE_ANGLES))
    assert 10 * len(kept) >= 8 * len(D.CANDIDATE_ANGLES)
    assert 0.0 in kept and any(a < 0 for a in kept) and any(0 < abs(a) <= 1 for a in kept)
    assert {0.0, 15.0, -15.0} <= set(D.CANDIDATE_ANGLES)


@pytest.mark.parametrize("S", SIZES)
def test_grid_sample_form_equals_the_direct_form(S):
    x = torch.from_numpy(f32((2, 3, S, S), 10 + S, 1.0, 255.0))           # (no zero: a zero fill shows)
    for a in D.screened_angles(S, S):
        g, d = D.rotate_grid(x, a), D.rotate_direct(x, a)
        assert torch.equal(g, d), a
        if abs(a) >= 5:
            assert bool((d == 0).any()) and not torch.equal(d, x), a      # (the corners left the image)


def test_angle_zero_ninety_and_the_flip_order():
    x = torch.from_numpy(f32((1, 2, 16, 16), 3, 1.0, 2.0))
    for form in ("direct", "grid"):
        assert torch.equal(D.augment(x, 0.0, False, form), x)
        assert torch.equal(D.augment(x, 90.0, False, form), torch.rot90(x, 1, (2, 3)))
        # the flip reverses the rows of the ROTATED image
        assert torch.equal(D.augment(x, 90.0, True, form), torch.flip(torch.rot90(x, 1, (2, 3)), dims=(2,)))
        assert not torch.equal(D.augment(x, 90.0, True, form), torch.rot90(torch.flip(x, dims=(2,)), 1, (2, 3)))
    assert cos_sin(0.0) == (1.0, 0.0) and cos_sin(12.5) == D.cos_sin(12.5)


def test_mri_crop_shared_parameters_and_minimum():
    assert crop_offset(256, 224) == 16 == D.crop_offset(256, 224) and crop_offset(24, 16) == 4 and crop_offset(20, 20) == 0
    assert crop_offset(21, 16) == 2 and crop_offset(19, 16) == 2          # round half to even: 2.5 -> 2, 1.5 -> 2
    t, c = f32((24, 24), 5, 100.0, 900.0), f32((24, 24), 6, 100.0, 900.0)
    kw = dict(mean_target=400.0, std_target=150.0, mean_cond=350.0, std_cond=120.0, crop=16)
    a = [x for x in D.screened_angles(16, 16) if x >= 10][0]
    hr, lr = D.mri_item(t, c, translate_zero=False, **kw)
    assert torch.equal(hr[0], (torch.from_numpy(t)[4:20, 4:20] - 400.0) / 150.0)
    assert torch.equal(lr[0], (torch.from_numpy(c)[4:20, 4:20] - 350.0) / 120.0)
    # the same image in both stores comes out the same way: both got the same rotation and flip
    hr, lr = D.mri_item(t, t, translate_zero=False, angle_deg=a, flip=True, **dict(kw, mean_cond=400.0, std_cond=150.0))
    assert torch.equal(hr, lr) and not torch.equal(hr, D.mri_item(t, t, translate_zero=False, angle_deg=a, **kw)[0])
    # all raw values are above the mean's zero point of the fill: the minimum is the zero fill's (0 - mean) / std, so it is
    # taken AFTER the rotation, and the corners come out as exactly 0
    hr, _ = D.mri_item(t, c, translate_zero=True, angle_deg=a, **kw)
    plain, _ = D.mri_item(t, c, translate_zero=False, angle_deg=a, **kw)
    fill = abs((torch.tensor(0.0) - 400.0) / 150.0)
    assert float(plain.min()) == -float(fill) and torch.equal(hr, plain + fill) and float(hr[0, 0, 0]) == 0.0
    unrot, _ = D.mri_item(t, c, translate_zero=True, **kw)
    assert float(unrot.min()) == 0.0 and float((unrot - D.mri_item(t, c, translate_zero=False, **kw)[0]).max()) < float(fill)


def test_table_rows_refusals():
    rows = table_rows([3, 0, 3], 4, [0.0, 15.0, -15.0], [0, 1, 0])
    assert rows["src"].tolist() == [3, 0, 3] and rows["flip"].tolist() == [0, 1, 0] and rows.itemsize == 16
    assert float(rows["cos_a"][0]) == 1.0 and float(rows["sin_a"][0]) == 0.0 and rows["sin_a"][1] == -rows["sin_a"][2]
    assert table_rows([1], 2)["cos_a"].tolist() == [1.0]
    for bad in ([4], [-1], [], [0.5]):
        with pytest.raises(ValueError):
            table_rows(bad, 4)
    with pytest.raises(ValueError):
        table_rows([0, 1], 4, [1.0])
    with pytest.raises(ValueError):
        table_rows([0, 1], 4, None, [1])
    with pytest.raises(ValueError):
        DeviceDataset.sr(np.zeros((2, 3, 13, 13), np.uint8))               # odd S, refused on the host
    with pytest.raises(ValueError):
        DeviceDataset.mnist(np.zeros((2, 28, 28), np.float32))
    with pytest.raises(ValueError):
        DeviceDataset.mri(np.zeros((2, 20, 20)), np.zeros((2, 20, 20)), mean_target=0.0, std_target=1.0, mean_cond=0.0,
                          std_cond=1.0, crop=24)


class FakeDataset:
    """Records what it is asked for, and when."""

    def __init__(self, n, augmentations):
        self.n, self.augmentations, self.log = n, augmentations, []

    def __len__(self):
        return self.n

    def batch(self, indices, angles_deg=None, flips=None):
        self.log.append(("batch", [int(i) for i in indices]))
        return len(self.log), (angles_deg, flips)


@pytest.mark.parametrize("aug", (False, True))
def test_plan_is_a_pure_permutation(aug):
    ds = FakeDataset(11, aug)
    src = BatchSource(ds, 4)
    assert len(src) == 3 and len(BatchSource(ds, 4, drop_last=True)) == 2 and len(BatchSource(ds, 11)) == 1
    p, q = src.plan(5), BatchSource(FakeDataset(11, aug), 4).plan(5)
    assert sorted(p["indices"].tolist()) == list(range(11)) and p["indices"].dtype == np.int64
    assert p["indices"].tolist() == q["indices"].tolist() == src.plan(5)["indices"].tolist()
    assert p["indices"].tolist() != src.plan(6)["indices"].tolist()
    assert p["indices"].tolist() != BatchSource(ds, 4, seed=43).plan(5)["indices"].tolist()
    assert p["indices"].tolist() != list(range(11))
    assert BatchSource(ds, 4, shuffle=False).plan(5)["indices"].tolist() == list(range(11))
    d = BatchSource(ds, 4, drop_last=True).plan(5)
    assert d["indices"].tolist() == p["indices"][:8].tolist()
    if not aug:
        assert p["angles_deg"] is None and p["flips"] is None
        return
    assert p["angles_deg"].shape == (11,) and p["flips"].shape == (11,) and p["flips"].dtype == bool
    assert np.array_equal(p["angles_deg"], q["angles_deg"]) and np.array_equal(p["flips"], q["flips"])
    assert not np.array_equal(p["angles_deg"], src.plan(6)["angles_deg"]) and d["angles_deg"].shape == (8,)
    many = np.concatenate([BatchSource(FakeDataset(500, True), 64).plan(s)["angles_deg"] for s in range(4)])
    flips = np.concatenate([BatchSource(FakeDataset(500, True), 64).plan(s)["flips"] for s in range(4)])
    assert many.min() >= -15.0 and many.max() < 15.0 and many.min() < -14.0 and many.max() > 14.0 and abs(many.mean()) < 1.0
    assert 0.4 < flips.mean() < 0.6
    with pytest.raises(ValueError):
        BatchSource(FakeDataset(3, aug), 4, drop_last=True)
    with pytest.raises(ValueError):
        BatchSource(ds, 0)


def test_batches_are_lazy_and_sized():
    ds = FakeDataset(10, True)
    src = BatchSource(ds, 4, seed=9)
    step = src.batches(2)
    plan = src.plan(2)
    assert len(step) == 3 and step.sizes == [4, 4, 2] and ds.log == []     # sized without asking for anything
    it = iter(step)
    assert ds.log == []
    for k in range(3):
        ds.log.append(("take", k))
        got, (ang, fl) = next(it)
        assert got == 2 * k + 2                                            # asked only now, after batch k - 1 was handed out
        assert np.array_equal(ang, plan["angles_deg"][4 * k:4 * k + 4]) and np.array_equal(fl, plan["flips"][4 * k:4 * k + 4])
    with pytest.raises(StopIteration):
        next(it)
    want = [e for k in range(3) for e in (("take", k), ("batch", plan["indices"][4 * k:4 * k + 4].tolist()))]
    assert ds.log == want
    assert [len(b[1][0]) for b in src.batches(2)] == [4, 4, 2]             # a second pass asks again
    plain = BatchSource(FakeDataset(10, False), 4)
    assert all(b[1] == (None, None) for b in plain.batches(0))


def test_train_tool_takes_a_store_or_ready_pairs():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_denoiser_tool_ds", os.path.join(root, "tools", "train_denoiser.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse(["--data", "mnist", "--store", "x.npy", "--labels", "y.npy", "--augmentations", "--no-shuffle"])
    assert (a.store, a.labels, a.augmentations, a.no_shuffle, a.hr, a.digit) == ("x.npy", "y.npy", True, True, None, 8)
    b = tool.parse(["--data", "mnist", "--hr", "a.npy", "--lr", "b.npy"])
    assert b.store is None and not b.augmentations and not b.no_shuffle
    for bad in (["--data", "mnist"], ["--data", "mnist", "--hr", "a.npy"], ["--data", "mnist", "--store", "x.npy", "--hr", "a.npy"],
                ["--data", "mnist", "--hr", "a.npy", "--lr", "b.npy", "--augmentations"]):
        with pytest.raises(SystemExit):
            tool.parse(bad)
