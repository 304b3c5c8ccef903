"""GPU tests of ``DenoiserTrainer.evaluate(sharded=True)`` / ``evaluate_local``: emulated ranks of worlds 1, 2 and 3 on the
one GPU over test batches of 3 and 2 MNIST-sized images (ragged shards; at world 3 rank 2 has no row of the second batch),
the fp64 host evaluation of the same definition, the unsharded ``evaluate``, the shards' rows against the whole batch's, and
world 1 through the real collective.  The host half alone is proved on the CPU in tests/test_metrics_ref.py."""
import math

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import rng
from localdiffusion_hallucination_amd.denoiser_train import EmulatedRank
from localdiffusion_hallucination_amd.dist import LdComm, patch_owner

from hip_helpers import DEV
import unet_grad_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
OPTS = dict(branch_out=False, start_intermediate=False, start_timestep=2, mask_x=False, ood_AD=False, ood_confidence=False,
            classifier=False, use_gt=False)
TIMESTEPS, SIZE = 4, 28
SIZES = (3, 2)
MIN_MAX = (0.0, 1.0)
PER_ROW = SIZE * SIZE                                       # elements of one image
DELTA = 1e-5                                                # tests/test_hip_dist.py's pin on a shard against the whole batch


def make_trainer(**kw):
    inf = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **R.KWARGS["mnist"])
    inf.load_state_dict(R.state("mnist", 0))
    gd = ldh.GaussianDiffusion(dict(OPTS, data="mnist"), inf, image_size=SIZE, timesteps=TIMESTEPS, objective="pred_v").to(DEV)
    assert gd.noise_source == "device"
    return ldh.DenoiserTrainer(gd, train_lr=1e-3, **kw)


def eval_batches():
    n = sum(SIZES)
    hr = torch.from_numpy(rng.uniform((n, 1, SIZE, SIZE), 7, 1, *MIN_MAX)).to(DEV)
    lr = torch.from_numpy(rng.uniform((n, 1, SIZE, SIZE), 7, 2, *MIN_MAX)).to(DEV)
    return [(hr[:SIZES[0]], lr[:SIZES[0]]), (hr[SIZES[0]:], lr[SIZES[0]:])]


@pytest.fixture(scope="module")
def runs():
    """For every world: the ranks' send buffers (stacked) and every rank's result of ``evaluate(sharded=True, gathered=...)``."""
    batches = eval_batches()
    out = {}
    for world in (1, 2, 3):
        ranks = [make_trainer(comm=EmulatedRank(world, r)) for r in range(world)]
        sends = [tr.evaluate_local(batches, MIN_MAX) for tr in ranks]
        gathered = torch.stack(sends).contiguous()
        values = [tr.evaluate(batches, MIN_MAX, sharded=True, gathered=gathered) for tr in ranks]
        out[world] = dict(gathered=gathered.cpu(), values=values, trainer=ranks[0])
    return batches, out


def owner_rows(gathered, world):
    """[rows, 2]: every row's (sse, n_elem) from its owner's copy."""
    rows, at = [], 0
    for size in SIZES:
        rows += [gathered[patch_owner(i, size, world), at + i] for i in range(size)]
        at += size
    return torch.stack(rows)


def test_every_rank_returns_the_same_float(runs):
    _, out = runs
    for world, run in out.items():
        assert all(isinstance(v, float) and math.isfinite(v) and v > 0.0 for v in run["values"])
        assert all(v == run["values"][0] for v in run["values"]), (world, run["values"])
        g = run["gathered"]
        assert g.dtype == F64 and tuple(g.shape) == (world, sum(SIZES), 2)
        # a rank's buffer holds its own rows and zeros elsewhere
        at = 0
        for size in SIZES:
            for i in range(size):
                for r in range(world):
                    mine = patch_owner(i, size, world) == r
                    assert (float(g[r, at + i, 1]) == PER_ROW) == mine and (float(g[r, at + i, 0]) > 0.0) == mine, (world, r, i)
            at += size
    with pytest.raises(RuntimeError, match="gathered"):
        out[2]["trainer"].evaluate(runs[0], MIN_MAX, sharded=True)          # an EmulatedRank has no collective
    with pytest.raises(ValueError):
        out[2]["trainer"].evaluate(runs[0], MIN_MAX, sharded=True, gathered=out[3]["gathered"].to(DEV))


def test_world_one_against_the_host_and_the_unsharded_evaluation(runs):
    """World 1 equals the fp64 host evaluation of the same definition on images sampled directly with ``diffusion.sample``
    (1e-12 relative) and is within 2e-4 relative of the unsharded ``evaluate``: (n - 1) 2^-24 = 1.4e-4 for an fp32 sum of
    n = 2,352 non-negative terms."""
    batches, out = runs
    tr, got = out[1]["trainer"], out[1]["values"][0]
    tr.sync_ema()
    per_batch = []
    for hr, lr in batches:
        img = tr.diffusion.sample(lr, None, batch_size=lr.shape[0], mask=None, min_max_val=MIN_MAX)
        d = (img.to(F32) - hr).to(F64).cpu()
        rows = [float((d[i] * d[i]).sum()) for i in range(d.shape[0])]
        total = 0.0
        for v in rows:
            total += v
        per_batch.append(total / (d.shape[0] * PER_ROW))
    want = sum(per_batch) / len(per_batch)
    plain = tr.evaluate(batches, MIN_MAX)
    print(f"sharded at world 1 {got!r}, host fp64 {want!r} (relative {abs(got - want) / want:.2e}), unsharded {plain!r} "
          f"(relative {abs(got - plain) / plain:.2e})")
    assert abs(got - want) <= 1e-12 * want
    assert (SIZES[0] * PER_ROW - 1) * 2.0 ** -24 <= 2e-4
    assert abs(got - plain) <= 2e-4 * plain


@pytest.mark.parametrize("world", [2, 3])
def test_shards_against_the_whole_batch_per_row(runs, world):
    """Per row, ``|sse_W - sse_1| <= 2 delta sqrt(n sse_1) + n delta^2``: what a per-element distance of at most delta = 1e-5
    between a shard's image and the whole batch's (the pin of tests/test_hip_dist.py) can move a sum of n squares by."""
    _, out = runs
    one, many = owner_rows(out[1]["gathered"], 1), owner_rows(out[world]["gathered"], world)
    assert torch.equal(one[:, 1], many[:, 1]) and bool((one[:, 1] == PER_ROW).all())
    for i in range(one.shape[0]):
        s1, sw = float(one[i, 0]), float(many[i, 0])
        bound = 2.0 * DELTA * math.sqrt(PER_ROW * s1) + PER_ROW * DELTA * DELTA
        print(f"world {world} row {i}: sse {sw!r} against {s1!r}, difference {abs(sw - s1):.3e} (bound {bound:.3e})")
        assert abs(sw - s1) <= bound, (world, i)


def test_world_one_through_the_real_collective(runs, monkeypatch):
    """An ``LdComm`` of one rank: ``evaluate(sharded=True)`` runs its all-gather and returns the emulated world 1's float; a
    plain trainer (no communicator) takes the same path without a collective, to the same float.  And what ``evaluate_local``
    adds around the sampler -- ``ld_metric_sums`` on the rank's rows and the writes into the table -- does not wait for the GPU:
    with ``sync_ema`` and ``sample`` stubbed (they repack and upload weights) it runs under ``set_sync_debug_mode('error')``."""
    batches, out = runs
    want = out[1]["values"][0]
    with LdComm.bootstrap(world=1, rank=0) as comm:
        tr = make_trainer(comm=comm)
        assert tr.data_parallel and (tr.world, tr.rank) == (1, 0)
        assert tr.evaluate(batches, MIN_MAX, sharded=True) == want
    plain = make_trainer()
    assert not plain.data_parallel and plain.evaluate(batches, MIN_MAX, sharded=True) == want
    images = iter([plain.diffusion.sample(lr, None, batch_size=lr.shape[0], mask=None, min_max_val=MIN_MAX) for _, lr in batches])
    monkeypatch.setattr(plain.diffusion, "sample", lambda *a, **kw: next(images))
    monkeypatch.setattr(plain, "sync_ema", lambda: None)
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        with pytest.raises(RuntimeError):
            probe.item()
        send = plain.evaluate_local(batches, MIN_MAX)               # raises if anything synchronises
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(send.cpu(), out[1]["gathered"][0])
