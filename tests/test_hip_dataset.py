"""GPU tests of csrc/dataset.hip through ``DeviceDataset`` / ``BatchSource``, and of ``DenoiserTrainer`` on a source.

Yardstick: the pure-torch CPU restatements of tests/dataset_ref.py (direct fp64 rotation), on random stores.  The mnist and
mri paths are chains of single correctly rounded fp32 operations, so they are held to ``torch.equal``; augmented cases use
only angles that pass the reference's tie screen (``dataset_ref.screened_angles``: no source coordinate within 1e-4 of a
half-integer, ~100 x the fp32 error of a coordinate), for which kernel and yardstick must pick the same source pixel
everywhere.  The SR path's hr is exact; its lr (a two-axis bilinear that ATen may contract to FMAs) is held to 1e-6 absolute:
values <= 2 and at most six fp32 roundings of <= 1.2e-7 each.  Output buffers start as NaN: every element must be written."""
import functools
import math

import numpy as np
import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import rng
from localdiffusion_hallucination_amd.dataset import BatchSource, DeviceDataset, table_rows

from hip_helpers import DEV, NAN, nans, st
import dataset_ref as D
import unet_grad_ref as R

pytestmark = pytest.mark.gpu

MRI_KW = dict(mean_target=412.7, std_target=151.3, mean_cond=388.1, std_cond=97.6)


def u8(shape, key):
    return (rng.bits64(int(np.prod(shape)), 77, key) >> np.uint64(56)).astype(np.uint8).reshape(shape)


def chunks(angles, n):
    """The screened angles in groups of n (the last group filled up from the front)."""
    angles = list(angles)
    return [(angles + angles)[k:k + n] for k in range(0, len(angles), n)]


def run(ds, idx, angles=None, flips=None):
    """``ds.batch`` into NaN-filled buffers: (hr, lr) on the CPU, every element written."""
    shape = (len(idx), ds.channels, ds.image_size, ds.image_size)
    out = (nans(*shape), nans(*shape))
    hr, lr = ds.batch(idx, angles, flips, out=out)
    assert hr is out[0] and lr is out[1]
    hr, lr = hr.cpu(), lr.cpu()
    assert bool(torch.isfinite(hr).all()) and bool(torch.isfinite(lr).all())
    return hr, lr


# ------------------------------------------------------------------------------------------------ the three kernels
def test_mnist_batches_are_the_restatement_bit_for_bit():
    store, idx = u8((7, 28, 28), 1), [3, 0, 6, 3, 5]                       # (a repeated index)
    plain = DeviceDataset.mnist(store)
    assert (len(plain), plain.channels, plain.image_size) == (7, 1, 28)
    hr, lr = run(plain, idx)
    want_hr, want_lr = D.mnist_batch(store, idx)
    assert torch.equal(hr, want_hr) and torch.equal(lr, want_lr)
    fresh_hr, fresh_lr = plain.batch(np.asarray(idx))                     # (its own buffers; indices as an array)
    assert torch.equal(fresh_hr.cpu(), want_hr) and torch.equal(fresh_lr.cpu(), want_lr)
    aug = DeviceDataset.mnist(store, augmentations=True)
    hr, lr = run(aug, idx)                                                # no parameters: the identity exactly
    assert torch.equal(hr, want_hr) and torch.equal(lr, want_lr)
    screened = D.screened_angles(28, 28)
    assert 10 * len(screened) >= 8 * len(D.CANDIDATE_ANGLES)
    for n, angles in enumerate(chunks(screened, 5)):
        flips = [(n + k) % 2 for k in range(5)]                           # both values, on every angle's neighbour
        hr, lr = run(aug, idx, angles, flips)
        want_hr, want_lr = D.mnist_batch(store, idx, angles, flips)
        assert torch.equal(hr, want_hr) and torch.equal(lr, want_lr), angles
    hr, _ = run(aug, [2], [90.0], [0])
    assert torch.equal(hr, torch.rot90(D.mnist_batch(store, [2])[0], 1, (2, 3)))


@pytest.mark.parametrize("S", (12, 16))
@pytest.mark.parametrize("C", (1, 3))
def test_sr_batches(S, C):
    """hr exact, lr within 1e-6 of ATen's bilinear, without and with (screened) angles and flips.  MI355X: lr max abs error
    2.38e-07 (one ulp at 2) in all four cases."""
    store, idx = u8((4, C, S, S), 10 * S + C), [2, 0, 2]
    plain = DeviceDataset.sr(store)
    assert (len(plain), plain.channels, plain.image_size) == (4, C, S)
    cases = [(plain, None, None)]
    aug = DeviceDataset.sr(store, augmentations=True)
    cases += [(aug, a, [k % 2 for k in range(3)]) for a in chunks(D.screened_angles(S, S), 3)]
    worst = 0.0
    for ds, angles, flips in cases:
        hr, lr = run(ds, idx, angles, flips)
        want_hr, want_lr = D.sr_batch(store, idx, angles, flips)
        assert torch.equal(hr, want_hr), angles
        err = float((lr - want_lr).abs().max())
        worst = max(worst, err)
        assert err <= 1e-6, (angles, err)
    print(f"sr S {S} C {C}: lr max abs err {worst:.2e} (bound 1e-6)")


@pytest.mark.parametrize("R_, crop", ((24, 16), (20, 20)))
@pytest.mark.parametrize("translate_zero", (True, False))
def test_mri_batches_are_the_restatement_bit_for_bit(R_, crop, translate_zero):
    target = rng.uniform((5, R_, R_), 77, 100 + R_, 0.0, 4096.0)
    cond = rng.uniform((5, R_, R_), 77, 200 + R_, 0.0, 4096.0)
    idx, kw = [4, 1, 1, 0], dict(MRI_KW, translate_zero=translate_zero, crop=crop)
    plain = DeviceDataset.mri(target, cond, **kw)
    assert (len(plain), plain.channels, plain.image_size) == (5, 1, crop)
    hr, lr = run(plain, idx)
    want_hr, want_lr = D.mri_batch(target, cond, idx, **kw)
    assert torch.equal(hr, want_hr) and torch.equal(lr, want_lr)
    if translate_zero:
        assert float(hr.amin(dim=(1, 2, 3)).max()) == 0.0 and float(lr.amin(dim=(1, 2, 3)).max()) == 0.0
    aug = DeviceDataset.mri(target, cond, augmentations=True, **kw)
    for n, angles in enumerate(chunks(D.screened_angles(crop, crop), 4)):
        flips = [(n + k) % 2 for k in range(4)]
        hr, lr = run(aug, idx, angles, flips)
        want_hr, want_lr = D.mri_batch(target, cond, idx, angles, flips, **kw)
        assert torch.equal(hr, want_hr) and torch.equal(lr, want_lr), angles


def test_refusals_raise_and_write_nothing():
    store = u8((7, 28, 28), 1)
    plain, aug = DeviceDataset.mnist(store), DeviceDataset.mnist(store, augmentations=True)
    out = (nans(2, 1, 28, 28), nans(2, 1, 28, 28))
    for ds, args in ((plain, ([0, 7],)), (plain, ([-1, 0],)), (aug, ([0, 7], [1.0, 2.0], [0, 1])),
                     (plain, ([0, 1], [1.0, 2.0])), (plain, ([0, 1], None, [0, 1])), (aug, ([0, 1], [1.0])), (plain, ([],))):
        with pytest.raises(ValueError):
            ds.batch(*args, out=out)
    with pytest.raises(ValueError):
        plain.batch([0, 1], out=(out[0], nans(2, 1, 28, 14)))
    lib = cabi.lib()
    table = torch.from_numpy(table_rows([0, 1], 2).view(np.uint8).copy()).to(DEV)
    odd = torch.zeros(2, 3, 13, 13, dtype=torch.uint8, device=DEV)
    big = (nans(2, 3, 13, 13), nans(2, 3, 13, 13))
    assert lib.ld_ds_sr_batch(odd.data_ptr(), 2, 3, 13, table.data_ptr(), 2, big[0].data_ptr(), big[1].data_ptr(), st()) == -1
    assert b"even" in lib.ld_last_error()
    assert lib.ld_ds_mnist_batch(odd.data_ptr(), 2, 13, table.data_ptr(), 2, big[0].data_ptr(), big[1].data_ptr(), st()) == -1
    assert lib.ld_ds_sr_batch(odd.data_ptr(), 2, 2, 12, table.data_ptr(), 2, big[0].data_ptr(), big[1].data_ptr(), st()) == -1
    store_dev = torch.from_numpy(store).to(DEV)
    assert lib.ld_ds_mnist_batch(store_dev.data_ptr(), 7, 28, table.data_ptr(), 0, out[0].data_ptr(), out[1].data_ptr(), st()) == -1
    assert b"empty batch" in lib.ld_last_error()
    f = torch.zeros(2, 20, 20, device=DEV)
    work = nans(2 * 2 * cabi.DS_MIN_PARTS)
    mri = (nans(2, 1, 24, 24), nans(2, 1, 24, 24))

    def mri_call(crop, B=2, std=1.0):
        return lib.ld_ds_mri_batch(f.data_ptr(), f.data_ptr(), 2, 20, crop, table.data_ptr(), B, 0.0, std, 0.0, 1.0, 1,
                                   work.data_ptr(), mri[0].data_ptr(), mri[1].data_ptr(), st())
    assert mri_call(24) == -1 and b"crop" in lib.ld_last_error()          # crop > R
    assert mri_call(18) == -1 and b"multiple of 4" in lib.ld_last_error()
    assert mri_call(16, B=0) == -1 and mri_call(16, std=0.0) == -1
    torch.cuda.synchronize()
    for t in out + big + mri + (work,):
        assert bool(torch.isnan(t).all())
    with pytest.raises(ValueError):
        DeviceDataset.mnist(store, device="cpu")


# ------------------------------------------------------------------------------------------------ the trainer on a source
TIMESTEPS, LR, SEED = 250, 1e-3, 9
OPTS = dict(branch_out=False, start_intermediate=False, start_timestep=2, mask_x=False, ood_AD=False, ood_confidence=False,
            classifier=False, use_gt=False, data="mnist")
STORE = u8((6, 28, 28), 31)


def make_trainer(seed=0):
    """The small mnist net of tests/test_hip_denoiser_train.py."""
    inf = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **R.KWARGS["mnist"])
    inf.load_state_dict(R.state("mnist", seed))
    gd = ldh.GaussianDiffusion(OPTS, inf, image_size=28, timesteps=TIMESTEPS, objective="pred_v").to(DEV)
    tr = ldh.DenoiserTrainer(gd, train_lr=LR, ema_update_every=2, ema_update_after_step=2)
    tr.online_model.debug_fill = NAN
    return tr


def draws(step, sizes):
    """Explicit t and noise for the batches of a step."""
    ts, ns = [], []
    for k, B in enumerate(sizes):
        key = 1000 + 10 * step + k
        ts.append(torch.tensor([(37 * (key + b) + 11 * b) % TIMESTEPS for b in range(B)], dtype=torch.long).to(DEV))
        ns.append(torch.from_numpy(rng.randn((B, 1, 28, 28), 7, key + 5000)).to(DEV))
    return ts, ns


class CountingSource(BatchSource):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.asked = []

    def batches(self, step):
        self.asked.append(step)
        return super().batches(step)


def source():
    return CountingSource(DeviceDataset.mnist(STORE, augmentations=True), 4, seed=SEED)


def rebuilt(src, step):
    """The step's batches from ``plan(step)`` by the CPU restatement.  The plan's angles must pass the tie screen (a
    condition of the test: SEED was chosen by it), so that the restatement is exact."""
    plan = src.plan(step)
    assert min(D.tie_margin(a, 28, 28) for a in plan["angles_deg"]) > D.MARGIN
    out = []
    for k in range(len(src)):
        sl = slice(4 * k, 4 * k + 4)
        hr, lr = D.mnist_batch(STORE, plan["indices"][sl].tolist(), plan["angles_deg"][sl], plan["flips"][sl])
        out.append((hr.to(DEV), lr.to(DEV)))
    return out


@functools.lru_cache(maxsize=None)
def source_run(ckpt_dir):
    """Two ``train_step(source)`` steps (augmentation, shuffle, a ragged second batch), a checkpoint after the first."""
    tr, src = make_trainer(), source()
    assert len(src) == 2 and src.batches(0).sizes == [4, 2]
    src.asked.clear()
    losses, digests, steps_seen = [], [], []
    for step in range(2):
        steps_seen.append(tr.step)
        t, noise = draws(step, [4, 2])
        losses.append(tr.train_step(src, t=t, noise=noise).cpu())
        digests.append(tr.replica_digest())
        if step == 0:
            tr.save(ckpt_dir + "/after1.pt")
    return dict(losses=losses, digests=digests, asked=list(src.asked), steps_seen=steps_seen, path=ckpt_dir + "/after1.pt")


@pytest.fixture(scope="module")
def ckpt_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dataset_train"))


def list_run():
    """The same two steps as ``train_step(list)`` on the CPU-rebuilt batches."""
    tr, src = make_trainer(), source()
    losses, digests = [], []
    for step in range(2):
        t, noise = draws(step, [4, 2])
        losses.append(tr.train_step(rebuilt(src, step), t=t, noise=noise).cpu())
        digests.append(tr.replica_digest())
    return losses, digests


def test_trainer_on_a_source_equals_the_rebuilt_lists(ckpt_dir):
    got = source_run(ckpt_dir)
    losses, digests = list_run()
    for step in range(2):
        assert math.isfinite(float(got["losses"][step])) and torch.equal(got["losses"][step], losses[step]), step
        assert got["digests"][step] == digests[step], step
    assert got["digests"][0] != got["digests"][1] and not torch.equal(got["losses"][0], got["losses"][1])


def test_source_is_asked_once_per_step_with_the_trainers_step(ckpt_dir):
    got = source_run(ckpt_dir)
    assert got["asked"] == [0, 1] == got["steps_seen"]


def test_resumed_trainer_sees_the_same_step(ckpt_dir):
    got = source_run(ckpt_dir)
    tr, src = make_trainer(seed=5), source()                               # (other weights until the load)
    tr.load(got["path"])
    assert tr.step == 1
    t, noise = draws(1, [4, 2])
    loss = tr.train_step(src, t=t, noise=noise).cpu()
    assert src.asked == [1] and torch.equal(loss, got["losses"][1]) and tr.replica_digest() == got["digests"][1]


def test_a_list_still_trains_as_accumulate_and_apply():
    a, b, src = make_trainer(), make_trainer(), source()
    for step in range(2):
        batches = rebuilt(src, step)
        t, noise = draws(step, [4, 2])
        got = a.train_step(iter(batches), t=t, noise=noise)               # (any iterable, as before)
        total = None
        for (hr, lr), tk, nk in zip(batches, t, noise):
            value = b.accumulate(hr, lr, scale=0.5, t=tk, noise=nk)
            total = value if total is None else total + value
        b.apply()
        assert torch.equal(got.cpu(), total.cpu()) and a.replica_digest() == b.replica_digest(), step
    torch.manual_seed(11)
    drawn = a.train_step(rebuilt(src, 0))                                  # t and noise drawn, as without the new arguments
    assert math.isfinite(float(drawn)) and a.step == 3
    with pytest.raises(ValueError):
        a.train_step([])
    with pytest.raises(ValueError):
        a.train_step(rebuilt(src, 0), t=[None])
