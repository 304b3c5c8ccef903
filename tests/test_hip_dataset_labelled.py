"""GPU tests of ``ld_ds_seg_batch`` / ``ld_ds_mnist_cls_batch`` through ``DeviceDataset.seg`` / ``DeviceDataset.mnist_cls`` and
``BatchSource``, of ``SegTrainer.fit`` / ``MnistClassifierTrainer.fit`` on a source, and of the two command lines.

Yardstick: the CPU restatements of tests/dataset_labelled_ref.py (defined through tests/dataset_ref.py, whose conditions
tests/test_dataset_labelled_ref.py checks).  Both paths are chains of single correctly rounded fp32 operations, so every
comparison is ``torch.equal``: there is no tolerance here.  Augmented cases use only angles that pass the tie screen
(``dataset_ref.screened_angles``).  Output buffers start as NaN (labels as -1): every element must be written.  Both trainers
are bit-reproducible, so ``fit`` over a source is held to equality with ``fit`` over the same source's materialised lists."""
import csv
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import checkpoint, rng, weights
from localdiffusion_hallucination_amd.dataset import BatchSource, DeviceDataset, table_rows

from hip_helpers import DEV, nans, st
import dataset_labelled_ref as L
import dataset_ref as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG_KW = dict(mean=412.7, std=151.3)
SEG_SIZES = ((24, 16), (20, 20), (21, 16), (23, 16))      # (R, crop); the last two: half-to-even crop offsets 2 and 4
PLAN_SEED = 2                                             # its plans' angles pass the tie screen at steps 0 and 3 (asserted)


def u8(shape, key):
    return (rng.bits64(int(np.prod(shape)), 77, key) >> np.uint64(56)).astype(np.uint8).reshape(shape)


def seg_stores(R, n=5):
    """fp32 slices in [0, 4096) and u8 label maps drawn from {0, 0, 0, 1, 2, 4}: about half background, non-binary positives."""
    images = rng.uniform((n, R, R), 77, 100 + R, 0.0, 4096.0)
    pick = (rng.bits64(n * R * R, 77, 300 + R) >> np.uint64(32)) % np.uint64(6)
    labels = np.array([0, 0, 0, 1, 2, 4], dtype=np.uint8)[pick.astype(np.int64)].reshape(n, R, R)
    return images, labels


def digit_labels(n, key=0):
    """Labels covering 0..9 and repeating."""
    return np.array([(3 * k + key) % 10 for k in range(n)], dtype=np.int64)


def chunks(angles, n):
    """The screened angles in groups of n (the last group filled up from the front)."""
    angles = list(angles)
    return [(angles + angles)[k:k + n] for k in range(0, len(angles), n)]


def blank(ds, B):
    shape = (B, 1, ds.image_size, ds.image_size)
    if ds.kind == "mnist_cls":
        return nans(*shape), torch.full((B,), -1, dtype=torch.int64, device=DEV)
    return nans(*shape), nans(*shape)


def untouched(pair):
    a, b = pair
    return bool(torch.isnan(a).all()) and bool((torch.isnan(b) if b.is_floating_point() else b == -1).all())


def run(ds, idx, angles=None, flips=None):
    """``ds.batch`` into prefilled buffers -> the pair on the CPU, every element written."""
    out = blank(ds, len(idx))
    a, b = ds.batch(idx, angles, flips, out=out)
    assert a is out[0] and b is out[1]
    a, b = a.cpu(), b.cpu()
    assert bool(torch.isfinite(a).all())
    assert bool(torch.isfinite(b).all()) if b.is_floating_point() else bool((b >= 0).all())
    return a, b


def same(got, want):
    return all(g.dtype == w.dtype and torch.equal(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ 1. seg
@pytest.mark.parametrize("R, crop", SEG_SIZES)
def test_seg_batches_are_the_restatement_bit_for_bit(R, crop):
    images, labels = seg_stores(R)
    idx, kw = [4, 1, 1, 0], dict(SEG_KW, crop=crop)
    plain = DeviceDataset.seg(images, labels, **kw)
    assert (plain.kind, len(plain), plain.channels, plain.image_size) == ("seg", 5, 1, crop)
    want = L.seg_batch(images, labels, idx, **kw)
    got = run(plain, idx)
    assert same(got, want)
    assert set(got[1].unique().tolist()) == {0.0, 1.0}
    fresh = plain.batch(np.asarray(idx))                                  # (its own buffers; indices as an array)
    assert same([t.cpu() for t in fresh], want)
    assert same(run(DeviceDataset.seg(images, labels.astype(np.float64) * 0.5, **kw), idx), want)       # any real dtype: > 0
    aug = DeviceDataset.seg(images, labels, augmentations=True, **kw)
    assert same(run(aug, idx), want)                                      # no parameters: the identity exactly
    screened = D.screened_angles(crop, crop)
    assert len(screened) >= 16
    for n, angles in enumerate(chunks(screened, 4)):
        flips = [(n + k) % 2 for k in range(4)]                           # both values, on every angle's neighbour
        got = run(aug, idx, angles, flips)
        assert same(got, L.seg_batch(images, labels, idx, angles, flips, **kw)), angles
        assert set(got[1].unique().tolist()) <= {0.0, 1.0}
    x, target = run(aug, [2], [90.0], [0])
    px, pt = L.seg_batch(images, labels, [2], **kw)
    assert torch.equal(x, torch.rot90(px, 1, (2, 3))) and torch.equal(target, torch.rot90(pt, 1, (2, 3)))


# ------------------------------------------------------------------------------------------------ 2. mnist_cls
@pytest.mark.parametrize("S, idx", ((28, [3, 0, 6, 3, 5]), (36, [3, 0, 6, 3, 5]), (28, [6])))
def test_mnist_cls_batches_are_the_restatement_bit_for_bit(S, idx):
    """S = 36: 324 groups of four pixels, two blocks per plane -- the tail guard, and the label written once per sample."""
    store, labels = u8((7, S, S), S), digit_labels(7)
    assert set(labels.tolist()) <= set(range(10)) and len(set(labels[idx].tolist())) == len(set(idx))
    plain = DeviceDataset.mnist_cls(store, labels)
    assert (plain.kind, len(plain), plain.channels, plain.image_size) == ("mnist_cls", 7, 1, S)
    want = L.mnist_cls_batch(store, labels, idx)
    x, label = plain.batch(idx)
    assert label.dtype == torch.int64 and label.is_cuda and tuple(label.shape) == (len(idx),)
    assert same((x.cpu(), label.cpu()), want)
    assert same(run(plain, idx), want)
    aug = DeviceDataset.mnist_cls(store, labels.astype(np.uint8), augmentations=True)
    assert same(run(aug, idx), want)
    screened = D.screened_angles(S, S)
    assert len(screened) >= 16
    for n, angles in enumerate(chunks(screened, len(idx))):
        flips = [(n + k) % 2 for k in range(len(idx))]
        assert same(run(aug, idx, angles, flips), L.mnist_cls_batch(store, labels, idx, angles, flips)), angles


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_raise_and_write_nothing():
    store, labels = u8((7, 28, 28), 28), digit_labels(7)
    for bad in (np.where(np.arange(7) == 2, 10, labels), np.where(np.arange(7) == 5, -1, labels), labels[:6], labels.astype(np.float32)):
        with pytest.raises(ValueError):
            DeviceDataset.mnist_cls(store, bad)
    images, seg = seg_stores(24)
    kw = dict(SEG_KW, crop=16)
    with pytest.raises(ValueError):
        DeviceDataset.seg(images, seg[:, :20, :20], **kw)
    with pytest.raises(ValueError):
        DeviceDataset.seg(images, seg[:4], **kw)
    poisoned = images.copy()
    poisoned[3, 5, 7] = np.nan
    with pytest.raises(ValueError):
        DeviceDataset.seg(poisoned, seg, **kw)
    for change in (dict(std=0.0), dict(std=-1.0), dict(std=float("inf")), dict(mean=float("nan")), dict(crop=18), dict(crop=28),
                   dict(crop=16.0), dict(crop=0)):
        with pytest.raises(ValueError):
            DeviceDataset.seg(images, seg, **dict(kw, **change))
    with pytest.raises(ValueError):
        DeviceDataset.seg(images, seg, device="cpu", **kw)

    cls_ds, seg_ds = DeviceDataset.mnist_cls(store, labels), DeviceDataset.seg(images, seg, **kw)
    cls_out, seg_out = blank(cls_ds, 2), blank(seg_ds, 2)
    for ds, out in ((cls_ds, cls_out), (seg_ds, seg_out)):
        for args in (([0, 1], [1.0, 2.0]), ([0, 1], None, [0, 1]), ([0, len(ds)],), ([-1, 0],), ([],)):
            with pytest.raises(ValueError):                               # angles / flips without augmentations; indices
                ds.batch(*args, out=out)
    for out in ((cls_out[0], torch.full((2,), -1, dtype=torch.int32, device=DEV)), (cls_out[0], cls_out[1].cpu()),
                (cls_out[0], torch.full((3,), -1, dtype=torch.int64, device=DEV)), (cls_out[0], cls_out[0]), (cls_out[1], cls_out[1])):
        with pytest.raises(ValueError):
            cls_ds.batch([0, 1], out=out)
    for out in ((seg_out[0], nans(2, 1, 16, 8)), (seg_out[0], cls_out[1]), (seg_out[0], nans(2, 1, 16, 32)[..., :16])):
        with pytest.raises(ValueError):
            seg_ds.batch([0, 1], out=out)

    lib = cabi.lib()
    table = torch.from_numpy(table_rows([0, 1], 2).view(np.uint8).copy()).to(DEV)
    f, lab = torch.zeros(2, 24, 24, device=DEV), torch.zeros(2, 24, 24, dtype=torch.uint8, device=DEV)
    big = (nans(2, 1, 24, 24), nans(2, 1, 24, 24))

    def seg_call(crop=16, B=2, std=1.0, image=f, label=lab, tab=table):
        return lib.ld_ds_seg_batch(cabi.ptr(image), cabi.ptr(label), 2, 24, crop, cabi.ptr(tab), B, 0.0, std, big[0].data_ptr(),
                                   big[1].data_ptr(), st())
    for call, word in ((dict(image=None), b"null"), (dict(label=None), b"null"), (dict(tab=None), b"null"), (dict(B=0), b"empty batch"),
                       (dict(crop=18), b"multiple of 4"), (dict(crop=28), b"crop"), (dict(std=0.0), b"std")):
        assert seg_call(**call) == -1, call
        assert b"ld_ds_seg_batch" in lib.ld_last_error() and word in lib.ld_last_error(), (call, lib.ld_last_error())
    dstore, dlabels = torch.from_numpy(store).to(DEV), torch.from_numpy(labels.astype(np.uint8)).to(DEV)
    spare = torch.full((3,), -1, dtype=torch.int64, device=DEV)

    def cls_call(S=28, B=2, images=dstore, digits=dlabels, label_ptr=None):
        return lib.ld_ds_mnist_cls_batch(cabi.ptr(images), cabi.ptr(digits), 7, S, table.data_ptr(), B, cls_out[0].data_ptr(),
                                         cls_out[1].data_ptr() if label_ptr is None else label_ptr, st())
    for call, word in ((dict(images=None), b"null"), (dict(digits=None), b"null"), (dict(B=0), b"empty batch"), (dict(S=27), b"even"),
                       (dict(label_ptr=spare.data_ptr() + 4), b"8-byte")):
        assert cls_call(**call) == -1, call
        assert b"ld_ds_mnist_cls_batch" in lib.ld_last_error() and word in lib.ld_last_error(), (call, lib.ld_last_error())
    torch.cuda.synchronize()
    assert untouched(cls_out) and untouched(seg_out) and untouched(big) and bool((spare == -1).all())


# ------------------------------------------------------------------------------------------------ 4. BatchSource
def rebuild(kind, stores, plan, sl, **kw):
    args = (plan["indices"][sl].tolist(), plan["angles_deg"][sl], plan["flips"][sl])
    return L.seg_batch(*stores, *args, **kw) if kind == "seg" else L.mnist_cls_batch(*stores, *args)


@pytest.mark.parametrize("kind", ("seg", "mnist_cls"))
def test_batch_source_batches_equal_the_rebuild_from_the_plan(kind):
    if kind == "seg":
        stores, B, S, kw = seg_stores(24), 2, 16, dict(SEG_KW, crop=16)
        ds = DeviceDataset.seg(*stores, augmentations=True, **kw)
    else:
        stores, B, S, kw = (u8((7, 28, 28), 28), digit_labels(7)), 3, 28, {}
        ds = DeviceDataset.mnist_cls(*stores, augmentations=True)
    n = len(ds)
    src = BatchSource(ds, B, seed=PLAN_SEED)
    assert len(src) == -(-n // B)
    for step in (0, 3):
        plan = src.plan(step)
        assert min(D.tie_margin(a, S, S) for a in plan["angles_deg"]) > D.MARGIN       # a condition: PLAN_SEED was chosen by it
        assert sorted(plan["indices"].tolist()) == list(range(n))
        step_batches = src.batches(step)
        assert step_batches.sizes == [B] * (n // B) + [n % B]                        # a ragged last batch
        got = list(step_batches)
        assert len(got) == len(src)
        for k, pair in enumerate(got):
            want = rebuild(kind, stores, plan, slice(k * B, k * B + step_batches.sizes[k]), **kw)
            assert pair[0].shape[0] == step_batches.sizes[k] and same([t.cpu() for t in pair], want), (step, k)
    assert not np.array_equal(src.plan(0)["indices"], src.plan(3)["indices"])
    dropped = BatchSource(ds, B, seed=PLAN_SEED, drop_last=True)
    assert len(dropped) == n // B and dropped.batches(0).sizes == [B] * (n // B)
    assert [p[0].shape[0] for p in dropped.batches(0)] == [B] * (n // B)
    assert np.array_equal(dropped.plan(3)["indices"], src.plan(3)["indices"][:B * (n // B)])


# ------------------------------------------------------------------------------------------------ 5. / 6. the trainers
class CountingSource(BatchSource):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.asked = []

    def batches(self, step):
        self.asked.append(step)
        return super().batches(step)


def state(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def fresh_classifier():
    net = ldh.MnistClassifier()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.procedural_mnistcls_state_dict(0).items()})
    return net.to(DEV)


def test_mnist_classifier_trainer_on_a_source_equals_the_materialised_lists(tmp_path):
    train_store, test_store = u8((24, 28, 28), 501), u8((16, 28, 28), 502)
    train_labels, test_labels = digit_labels(24, 1), digit_labels(16, 2)

    def sources():
        return (CountingSource(DeviceDataset.mnist_cls(train_store, train_labels, augmentations=True), 8, seed=5),
                CountingSource(DeviceDataset.mnist_cls(test_store, test_labels), 8, shuffle=False))
    runs = []
    for mode in ("source", "lists"):
        net, (src, test) = fresh_classifier(), sources()
        tr = ldh.MnistClassifierTrainer(net)
        out, log = str(tmp_path / f"{mode}.pth"), str(tmp_path / f"{mode}.csv")
        if mode == "source":
            res = tr.fit(src, test, 2, out, log)
            assert src.asked == [0, 1] and test.asked == [0, 0]           # the epoch's batches; the same test batches
        else:
            res = tr.fit(lambda e: list(src.batches(e)), list(test.batches(0)), 2, out, log)
        tr.check_labels()                                                  # (labels were validated at construction)
        assert tr.t == 6 and all(math.isfinite(r[1]) for r in res["rows"])
        runs.append((state(net), res, out, open(log).read()))
    (sd_a, res_a, out_a, csv_a), (sd_b, res_b, out_b, csv_b) = runs
    assert sd_a.keys() == sd_b.keys()
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k
    assert res_a == res_b and csv_a == csv_b and len(res_a["rows"]) == 2
    assert res_a["best_epoch"] is not None                                # (MI355X: 12.5 % at epoch 0, so the file is written)
    ck_a, ck_b = torch.load(out_a), torch.load(out_b)
    assert ck_a.keys() == ck_b.keys() == sd_a.keys()
    for k in ck_a:
        assert torch.equal(ck_a[k], ck_b[k]), k


def test_seg_trainer_on_a_source_equals_the_materialised_lists(tmp_path):
    images, labels = seg_stores(40, n=12)                                 # 8 to train on, 4 to validate on
    kw = dict(SEG_KW, crop=32)

    def sources():
        return (CountingSource(DeviceDataset.seg(images[:8], labels[:8], augmentations=True, **kw), 4, seed=5),
                CountingSource(DeviceDataset.seg(images[8:], labels[8:], **kw), 4, shuffle=False))
    runs = []
    for mode in ("source", "lists"):
        net = ldh.SegUNet()
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_seg_state_dict(0).items()})
        net = net.to(DEV)
        src, val = sources()
        tr = ldh.SegTrainer(net)
        out = str(tmp_path / f"{mode}.pth")
        if mode == "source":
            res = tr.fit(src, val, 2, out)
            assert src.asked == [0, 1] and val.asked == [0, 0]
        else:
            res = tr.fit(lambda e: list(src.batches(e)), list(val.batches(0)), 2, out)
        assert tr.t == 4 and all(math.isfinite(r[1]) for r in res["train"]) and all(math.isfinite(r[1]) for r in res["val"])
        runs.append((state(net), res, out))
    (sd_a, res_a, out_a), (sd_b, res_b, out_b) = runs
    assert sd_a.keys() == sd_b.keys() and any("running_mean" in k for k in sd_a)
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k
    assert res_a["train"] == res_b["train"] and res_a["val"] == res_b["val"] and res_a == res_b
    ck_a, ck_b = torch.load(out_a), torch.load(out_b)                     # dice > 0: the first epoch always writes
    assert ck_a.keys() == ck_b.keys()
    for k in ck_a:
        assert torch.equal(ck_a[k], ck_b[k]), k


# ------------------------------------------------------------------------------------------------ 7. the command lines
def tool(name, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + [str(a) for a in args], capture_output=True, text=True,
                          timeout=300)


def finite_csv(path, columns):
    rows = list(csv.reader(open(path)))
    assert rows[0] == list(columns) and len(rows) == 3, rows              # two epochs
    assert all(math.isfinite(float(v)) for row in rows[1:] for v in row)
    return rows


def seg_store_args(tmp_path):
    images, labels = seg_stores(40, n=12)
    labels[3] = 0                                                          # a slice without a lesion: left out
    np.save(tmp_path / "flair.npy", images)
    np.save(tmp_path / "seg.npy", labels)
    return ("--store", tmp_path / "flair.npy", "--store-labels", tmp_path / "seg.npy", "--store-mean", SEG_KW["mean"], "--store-std",
            SEG_KW["std"], "--batch-size", 4, "--epochs", 2)


def test_train_seg_from_a_store_end_to_end(tmp_path):
    out = tmp_path / "out"
    done = tool("train_seg.py", *seg_store_args(tmp_path), "--crop", 32, "--augmentations", "--out", out)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "11 of 12 slices" in done.stdout and "train images 7, validation images 4" in done.stdout
    fresh = ldh.SegUNet()
    assert checkpoint.load_seg_checkpoint(str(out / "best_dice.pth"), fresh) == {"n_tensors": 118}
    assert all(bool(torch.isfinite(v).all()) for v in fresh.state_dict().values())
    finite_csv(out / "train.csv", ("epoch", "loss"))
    finite_csv(out / "val.csv", ("epoch", "dice", "bce"))


@pytest.mark.parametrize("case", ("both", "neither", "ragged"))
def test_train_seg_refuses_at_start_up(tmp_path, case):
    """Both forms or neither: a message and a non-zero exit.  ``ragged``: 7 training slices in batches of 3 at crop 16 -- the
    last batch has one value per channel at the deepest level, which training-mode BatchNorm cannot take."""
    store = seg_store_args(tmp_path)
    if case == "both":
        done, word = tool("train_seg.py", *store, "--images", tmp_path / "flair.npy", "--masks", tmp_path / "seg.npy"), "exactly one of --images"
    elif case == "neither":
        done, word = tool("train_seg.py", "--epochs", 2), "exactly one of --images"
    else:
        done, word = tool("train_seg.py", *store, "--crop", 16, "--batch-size", 3, "--out", tmp_path / "ragged"), "--drop-last"
    assert done.returncode != 0 and word in done.stderr, done.stderr[-2000:]
    assert not (tmp_path / "ragged").exists()


def write_idx(path, a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(struct.pack(">HBB", 0, 0x08, a.ndim) + struct.pack(">" + "I" * a.ndim, *a.shape) + a.tobytes())


def test_train_mnist_cls_with_device_data_end_to_end(tmp_path):
    """The twenty test digits are one image under the labels 0..9, twice: whatever class the net gives it, the accuracy is above
    0 and the checkpoint is written."""
    write_idx(tmp_path / "train-images", u8((24, 28, 28), 601))
    write_idx(tmp_path / "train-labels", digit_labels(24, 1))
    write_idx(tmp_path / "test-images", np.repeat(u8((1, 28, 28), 602), 20, axis=0))
    write_idx(tmp_path / "test-labels", np.arange(20) % 10)
    out = tmp_path / "out"
    done = tool("train_mnist_cls.py", "--train-images", tmp_path / "train-images", "--train-labels", tmp_path / "train-labels",
                "--test-images", tmp_path / "test-images", "--test-labels", tmp_path / "test-labels", "--epochs", 2, "--batch-size", 8,
                "--device-data", "--augmentations", "--out", out)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "train digits 24, test digits 20" in done.stdout
    loaded = ldh.MnistClassifier()
    assert checkpoint.load_mnist_classifier(str(out / "mnist_cls_best_model.pth"), loaded)["n_tensors"] == 8
    assert all(bool(torch.isfinite(v).all()) for v in loaded.state_dict().values())
    rows = finite_csv(out / "mnist_cls_loss.csv", ("epoch", "train_loss", "accuracy"))
    assert float(rows[1][2]) == 10.0                                       # one image under ten labels
