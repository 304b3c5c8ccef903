"""Data-parallel denoiser training on one GPU: ``ld_dn_opt_reduce`` alone on a synthetic table, emulated ranks against
micro-batch accumulation, the drawn values, world 1 through the real collective, save / load across world sizes, and two
real rank processes of ``tools/train_denoiser.py``."""
import ctypes as C
import importlib.util
import io
import os
import sys

import numpy as np
import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import launch
from localdiffusion_hallucination_amd.denoiser_train import EmulatedRank
from localdiffusion_hallucination_amd.dist import LdComm

from hip_helpers import DEV, NAN, st
import denoiser_dp_ref as D
import denoiser_train_ref as T
import unet_grad_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
CANARY, PAD = 7.5, 64
LR = 1e-3
OPTS = dict(branch_out=False, start_intermediate=False, start_timestep=2, mask_x=False, ood_AD=False, ood_confidence=False,
            classifier=False, use_gt=False)
TIMESTEPS = 250
CASE = R.CASES[1]                                           # mnist, 2 x 1 x 12 x 12: the smallest net the trainer tests train


def bits(t):
    return t.view(torch.int64 if t.dtype == F64 else torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
class Table:
    """A synthetic table (test_hip_denoiser_train.py's, restated for the reduction): the parameters in one canaried buffer,
    the flat gradient and the work buffer between canaries, and ``world`` gathered copies of ``flat + 4`` floats between
    canaries that hold NaN wherever the kernel must not read."""

    def __init__(self, world):
        lib = cabi.lib()
        n = len(D.SIZES)
        starts, at = [], PAD
        for c in D.SIZES:
            at = (at + 3) // 4 * 4
            starts.append(at)
            at += c
        self.params = torch.full((at + PAD,), CANARY, dtype=F32, device=DEV)
        host = (cabi.DnOptTensor * n)()
        for i, (e, c) in enumerate(zip(host, D.SIZES)):
            e.param, e.count, e.flags = self.params.data_ptr() + 4 * starts[i], c, (0 if i in D.NO_MOMENTS else 1)
        flat, wgs = cabi.i64(), cabi.i64()
        cabi.check(lib.ld_dn_opt_layout(host, n, C.byref(flat), C.byref(wgs)), "dn_opt_layout")
        self.n, self.flat, self.n_wg, self.world = n, int(flat.value), int(wgs.value), world
        self.off = [int(e.offset) for e in host]
        assert (self.off, self.flat) == D.offsets() and self.n_wg == sum((c + 4095) // 4096 for c in D.SIZES)
        self.stride = self.flat + D.TAIL
        self.adam = [i for i in range(n) if i not in D.NO_MOMENTS]
        self.table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
        self.grad = torch.full((self.flat + 2 * PAD,), CANARY, dtype=F32, device=DEV)
        self.work = torch.full((self.n_wg + 1 + 2 * PAD,), CANARY, dtype=F64, device=DEV)
        # the copies: NaN in the padding, the segments without moments and the tail's unused floats
        self.values = D.values(world, self.stride)
        rows = torch.full((world, self.stride), NAN, dtype=F32)
        vals = torch.from_numpy(self.values)
        for i in self.adam:
            rows[:, self.off[i]:self.off[i] + D.SIZES[i]] = vals[:, self.off[i]:self.off[i] + D.SIZES[i]]
        rows[:, self.flat] = vals[:, self.flat]
        self.gathered = torch.full((world * self.stride + 2 * PAD,), CANARY, dtype=F32, device=DEV)
        self.gathered[PAD:PAD + world * self.stride] = rows.reshape(-1).to(DEV)
        # the left-to-right fp32 sum of the copies, made with torch on the device
        copies = self.gathered[PAD:PAD + world * self.stride].view(world, self.stride)
        want = copies[0].clone()
        for r in range(1, world):
            want = want + copies[r]
        self.want = want

    def gptr(self, t=None):
        return (self.gathered if t is None else t).data_ptr() + 4 * PAD

    def reduce(self, gathered_ptr, grad_ptr, work):
        return cabi.lib().ld_dn_opt_reduce(self.table.data_ptr(), self.n, self.n_wg, gathered_ptr, self.world, self.stride, grad_ptr,
                                           self.flat, work.data_ptr() + 8 * PAD + 8, work.data_ptr() + 8 * PAD, st())

    def sqnorm_of(self, flat_values):
        """``ld_dn_opt_sqnorm``'s work buffer (sumsq, then the partial of every workgroup) on a flat buffer."""
        buf = torch.full((self.flat + 2 * PAD,), NAN, dtype=F32, device=DEV)
        buf[PAD:PAD + self.flat] = flat_values
        work = torch.full_like(self.work, CANARY)
        cabi.check(cabi.lib().ld_dn_opt_sqnorm(self.table.data_ptr(), self.n, self.n_wg, buf.data_ptr() + 4 * PAD, self.flat,
                                               work.data_ptr() + 8 * PAD + 8, work.data_ptr() + 8 * PAD, st()), "dn_opt_sqnorm")
        return work

    def trained(self):
        keep = torch.zeros(self.flat, dtype=torch.bool, device=DEV)
        for i in self.adam:
            keep[self.off[i]:self.off[i] + D.SIZES[i]] = True
        return keep


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_reduce_on_a_synthetic_table(world):
    """Sizes 1, 3, 4, 5, 4,095, 4,096, 4,097 and 8,193 with moments, 2 and 4,099 without: ``grad`` is bit-equal to the
    left-to-right fp32 sum of the copies (torch on the device, and numpy on the host), ``*sumsq`` and every workgroup's
    partial to ``ld_dn_opt_sqnorm``'s on that sum; canaries, padding and the segments without moments stay; the in-place form
    gives the same bits and leaves the other copies alone; the loss tail is the rank-ordered sum."""
    tb = Table(world)
    trained = tb.trained()
    host_sum = torch.from_numpy(D.ordered_sum(tb.values))
    assert torch.equal(bits(tb.want[:tb.flat][trained].cpu()), bits(host_sum[:tb.flat][trained.cpu()]))
    if world >= 3:                                           # the inputs tell the order: the reverse sum has other bits
        rev = torch.from_numpy(D.ordered_sum(tb.values[::-1]))
        assert not torch.equal(bits(rev[:tb.flat][trained.cpu()]), bits(host_sum[:tb.flat][trained.cpu()]))
    want_work = tb.sqnorm_of(torch.where(trained, tb.want[:tb.flat], torch.full_like(tb.want[:tb.flat], NAN)))
    before = tb.gathered.clone()
    cabi.check(tb.reduce(tb.gptr(), tb.grad.data_ptr() + 4 * PAD, tb.work), "dn_opt_reduce")
    got = tb.grad[PAD:PAD + tb.flat]
    assert torch.equal(bits(got[trained]), bits(tb.want[:tb.flat][trained]))
    assert bool((got[~trained] == CANARY).all())            # the padding and the segments without moments
    assert bool((tb.grad[:PAD] == CANARY).all()) and bool((tb.grad[PAD + tb.flat:] == CANARY).all())
    assert torch.equal(bits(tb.work), bits(want_work))      # sumsq, every partial, and the canaries around them
    assert bool(tb.work[PAD].isfinite()) and float(tb.work[PAD]) > 0.0
    assert torch.equal(bits(tb.gathered), bits(before))     # (the input is read only)
    if world == 1:
        assert torch.equal(bits(got[trained]), bits(tb.gathered[PAD:PAD + tb.flat][trained]))
    # in place: grad = the rank's own copy
    for rank in sorted({0, world - 1}):
        g = before.clone()
        work = torch.full_like(tb.work, CANARY)
        cabi.check(tb.reduce(tb.gptr(g), tb.gptr(g) + 4 * rank * tb.stride, work), "dn_opt_reduce in place")
        rows, orig = g[PAD:PAD + world * tb.stride].view(world, tb.stride), before[PAD:PAD + world * tb.stride].view(world, tb.stride)
        assert torch.equal(bits(rows[rank, :tb.flat][trained]), bits(tb.want[:tb.flat][trained])), rank
        assert bool(rows[rank, :tb.flat][~trained].isnan().all()) and torch.equal(bits(rows[rank, tb.flat:]), bits(orig[rank, tb.flat:]))
        for r in range(world):
            assert r == rank or torch.equal(bits(rows[r]), bits(orig[r])), (rank, r)
        assert bool((g[:PAD] == CANARY).all()) and bool((g[PAD + world * tb.stride:] == CANARY).all())
        assert torch.equal(bits(work), bits(want_work)), rank
    # the loss tail
    out = torch.full((3,), CANARY, dtype=F32, device=DEV)
    cabi.check(cabi.lib().ld_dn_opt_reduce_tail(tb.gptr(), world, tb.stride, tb.flat, out.data_ptr() + 4, st()), "reduce_tail")
    assert torch.equal(bits(out[1]), bits(tb.want[tb.flat])) and float(out[0]) == CANARY and float(out[2]) == CANARY
    assert torch.equal(bits(out[1].cpu()), bits(host_sum[tb.flat]))


def test_reduce_refusals_write_nothing():
    """A world of 0 or 65, a misaligned pointer or stride, a stride below the flat length, a null pointer and a gradient that
    overlaps the copies askew return -1 and write nothing."""
    tb = Table(3)
    lib = cabi.lib()
    before = [t.clone() for t in (tb.gathered, tb.grad, tb.work)]
    a = dict(table=tb.table.data_ptr(), n=tb.n, n_wg=tb.n_wg, gathered=tb.gptr(), world=3, stride=tb.stride,
             grad=tb.grad.data_ptr() + 4 * PAD, flat=tb.flat, work=tb.work.data_ptr() + 8 * PAD + 8, sumsq=tb.work.data_ptr() + 8 * PAD)

    def call(**kw):
        return lib.ld_dn_opt_reduce(*dict(a, **kw).values(), st())
    for world in (0, -1, 65):
        assert call(world=world) == -1 and b"world" in lib.ld_last_error(), world
    for k in ("gathered", "grad", "table", "work", "sumsq"):
        assert call(**{k: a[k] + 4}) == -1 and b"aligned" in lib.ld_last_error(), k
        assert call(**{k: None}) == -1 and b"null" in lib.ld_last_error(), k
    assert call(stride=tb.flat - 4) == -1 and b"rank_stride" in lib.ld_last_error()
    assert call(stride=tb.stride + 1) == -1 and b"rank_stride" in lib.ld_last_error()
    assert call(grad=a["gathered"] + 16) == -1 and b"overlaps" in lib.ld_last_error()
    assert call(n=0) == -1 and call(n_wg=0) == -1 and call(flat=tb.flat + 2) == -1
    out = torch.full((1,), CANARY, dtype=F32, device=DEV)
    assert lib.ld_dn_opt_reduce_tail(tb.gptr(), 0, tb.stride, tb.flat, out.data_ptr(), st()) == -1
    assert lib.ld_dn_opt_reduce_tail(tb.gptr(), 3, tb.stride, tb.stride, out.data_ptr(), st()) == -1
    assert lib.ld_dn_opt_reduce_tail(tb.gptr(), 3, tb.stride, tb.flat, None, st()) == -1
    torch.cuda.synchronize()
    for was, t in zip(before, (tb.gathered, tb.grad, tb.work)):
        assert torch.equal(bits(was), bits(t))
    assert float(out[0]) == CANARY


# ------------------------------------------------------------------------------------------------ 2. the trainer
def make_diffusion(sd=None, image_size=28, timesteps=TIMESTEPS, objective="pred_v", seed=0):
    inf = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **R.KWARGS["mnist"])
    inf.load_state_dict(R.state("mnist", seed) if sd is None else sd)
    return ldh.GaussianDiffusion(dict(OPTS, data="mnist"), inf, image_size=image_size, timesteps=timesteps, objective=objective).to(DEV)


def make_trainer(diffusion=None, **kw):
    args = dict(train_lr=LR, ema_update_every=1, ema_update_after_step=1)
    args.update(kw)
    tr = ldh.DenoiserTrainer(make_diffusion() if diffusion is None else diffusion, **args)
    tr.online_model.debug_fill = NAN
    return tr


def dev_batch(step, j):
    return tuple(v.to(DEV) for v in T.batch(CASE, step, j, TIMESTEPS))


def state_of(tr):
    """Everything a step moves: the online weights, both moments, the EMA buffer and the squared norm (device tensors)."""
    return dict(online=torch.cat([p.detach().reshape(-1) for p in tr.online_model.parameters()]), m=tr._m.clone(), v=tr._v.clone(),
                ema=tr._ema.clone(), sumsq=tr._work[:1].clone())


def same_state(a, b, what):
    sa, sb = state_of(a), state_of(b)
    for k in sa:
        assert torch.equal(bits(sa[k]), bits(sb[k])), (what, k)
    assert (a.step, a.ema_step, a.ema_initted, a.last_ema) == (b.step, b.ema_step, b.ema_initted, b.last_ema), what


def emulated_step(ranks, step, first=0):
    """One step of ``len(ranks)`` emulated ranks: rank r accumulates micro-batch ``first + r`` of the step, the send buffers
    are stacked into ``gathered``, every rank applies it.  Returns the ranks' losses."""
    W = len(ranks)
    for r, tr in enumerate(ranks):
        hr, lr, t, noise = dev_batch(step, first + r)
        tr.accumulate(hr, lr, scale=1.0 / W, t=t, noise=noise)
    gathered = torch.stack([tr.send_buffer() for tr in ranks]).contiguous()
    return [tr.apply(gathered=gathered) for tr in ranks]


def plain_step(tr, step, W):
    total = None
    for j in range(W):
        hr, lr, t, noise = dev_batch(step, j)
        value = tr.accumulate(hr, lr, scale=1.0 / W, t=t, noise=noise)
        total = value if total is None else total + value
    assert tr.apply() is None
    return total


@pytest.mark.parametrize("W", [2, 3])
def test_emulated_ranks_equal_micro_batch_accumulation(W):
    """W trainers as ranks 0 .. W-1 (two rows each, explicit ``t`` and noise) against one plain trainer that accumulates the
    same W micro-batches in order: after every one of four steps (``ema_update_every = ema_update_after_step = 1``: two
    copies, the copy that initialises the EMA, and the first lerp) the online weights, both moments, the EMA buffer, the
    squared norm and the loss hold the same bits on every rank and on the plain trainer."""
    ranks = [make_trainer(comm=EmulatedRank(W, r)) for r in range(W)]
    plain = make_trainer()
    assert [(t.world, t.rank) for t in ranks] == [(W, r) for r in range(W)] and (plain.world, plain.rank) == (1, 0)
    modes = []
    for step in range(4):
        losses = emulated_step(ranks, step)
        want = plain_step(plain, step, W)
        for r in range(W):
            same_state(ranks[r], plain, (step, r))
            assert torch.equal(bits(losses[r]), bits(want)), (step, r, float(losses[r]), float(want))
            assert bool((ranks[r].send_buffer() == 0).all())                # gradients and the loss slot are zeroed
        assert float(want) > 0.0 and float(plain._work[0]) > 0.0
        modes.append(plain.last_ema[0])
    assert modes == [1, 1, 1, 2] and plain.ema_initted


@pytest.mark.parametrize("strength", [0.0, 0.1])
def test_drawn_values_are_slices_of_the_global_draw(strength):
    """With ``t`` and the noise left to the trainer, what two ranks draw for their rows, concatenated, is what a one-rank
    trainer draws for the global batch of four (offset noise off and on); afterwards the rank's diffusion samples what it
    sampled before: its noise offset is back."""
    W = 2
    hr = torch.cat([dev_batch(0, j)[0] for j in range(W)])
    lr = torch.cat([dev_batch(0, j)[1] for j in range(W)])
    kw = dict(image_size=12, timesteps=4, objective="pred_x0")

    def drawn(tr, hr, lr):
        seen = {}
        inner = tr.diffusion.training_noise

        def spy(*a, **k):
            seen["noise"] = inner(*a, **k)
            return seen["noise"]
        tr.diffusion.training_noise = spy
        hook = tr.online_model.time_mlp.register_forward_pre_hook(lambda mod, args: seen.__setitem__("t", args[0].detach().clone()))
        torch.manual_seed(123)                               # every rank alike
        tr.accumulate(hr, lr)
        hook.remove()
        del tr.diffusion.training_noise
        return seen["t"], seen["noise"]
    plain = make_trainer(make_diffusion(**kw))
    plain.diffusion.offset_noise_strength = strength
    want_t, want_noise = drawn(plain, hr, lr)
    assert want_noise.shape == hr.shape and plain.diffusion._train_draw == (1 if strength else 0)
    ts, noises = [], []
    for r in range(W):
        tr = make_trainer(make_diffusion(**kw), comm=EmulatedRank(W, r))
        tr.diffusion.offset_noise_strength = strength
        cond = lr[:2]
        sample = lambda: tr.diffusion.sample(cond, None, batch_size=2, min_max_val=(0.0, 1.0))      # noqa: E731
        before = sample()
        t, noise = drawn(tr, hr[2 * r:2 * r + 2], lr[2 * r:2 * r + 2])
        ts.append(t)
        noises.append(noise)
        assert tr.diffusion.noise_offset == 0 and tr.diffusion._train_draw == plain.diffusion._train_draw
        assert torch.equal(bits(sample()), bits(before)), r
    assert torch.equal(torch.cat(ts), want_t) and len(set(want_t.tolist())) > 1
    assert torch.equal(bits(torch.cat(noises)), bits(want_noise))
    assert not torch.equal(noises[0], noises[1])


def test_world_one_through_the_real_collective():
    """An ``LdComm`` of one rank: the all-gather, ``ld_dn_opt_reduce`` on the one copy and the loss tail leave the bits of the
    plain trainer over two steps; ``replica_digest`` returns; and the step still does not synchronise (a lone ``.item()``
    under ``set_sync_debug_mode('error')`` raises, the step does not)."""
    with LdComm.bootstrap(world=1, rank=0) as comm:
        tr, plain = make_trainer(comm=comm), make_trainer()
        assert tr.data_parallel and not plain.data_parallel and (tr.world, tr.rank) == (1, 0)
        for step in range(2):
            hr, lr, t, noise = dev_batch(step, 0)
            for x in (tr, plain):
                x.accumulate(hr, lr, t=t, noise=noise)
            loss = tr.apply()
            assert plain.apply() is None
            same_state(tr, plain, step)
        d = tr.replica_digest()
        assert d["step"] == 2 and d["sumsq"] == float(plain._work[0]) and d == dict(plain.replica_digest())
        probe = torch.ones(1, device=DEV)
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        try:
            torch.cuda.set_sync_debug_mode("error")
            with pytest.raises(RuntimeError):
                probe.item()
            tr.accumulate(hr, lr, scale=0.5, t=t, noise=noise)           # raises if anything synchronises
            tr.accumulate(hr, lr, scale=0.5)                             # t and noise drawn by the trainer
            loss = tr.apply()
            total = tr.train_step([(hr, lr)])
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        assert np.isfinite(float(loss)) and np.isfinite(float(total)) and tr.step == 4 and tr.check_finite() > 0.0


def test_save_at_two_ranks_load_at_one(tmp_path):
    """Two emulated ranks train two steps and rank 0 saves; a plain trainer built on other weights loads the file; one more
    step of the ranks and of the loaded trainer (accumulating the same two micro-batches) leaves the same bits."""
    ranks = [make_trainer(comm=EmulatedRank(2, r)) for r in range(2)]
    for step in range(2):
        emulated_step(ranks, step)
    path = str(tmp_path / "model-best100.pt")
    ranks[0].save(path)
    loaded = make_trainer(make_diffusion(seed=5))
    info = loaded.load(path)
    assert info["source"] == "ema" and (loaded.step, loaded.ema_step) == (2, 2)
    losses = emulated_step(ranks, 2)
    want = plain_step(loaded, 2, 2)
    same_state(ranks[0], loaded, "after the load")
    same_state(ranks[1], loaded, "after the load")
    assert torch.equal(bits(losses[0]), bits(want))
    # ... and the other way round: a file saved by the plain trainer, loaded by two ranks
    loaded.save(path)
    again = [make_trainer(make_diffusion(seed=6), comm=EmulatedRank(2, r)) for r in range(2)]
    for tr in again:
        tr.load(path)
    emulated_step(again, 3)
    plain_step(loaded, 3, 2)
    same_state(again[0], loaded, "two ranks from a one-rank file")


# ------------------------------------------------------------------------------------------------ 3. two processes
def load_tool():
    spec = importlib.util.spec_from_file_location("train_denoiser_tool", os.path.join(ROOT, "tools", "train_denoiser.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_two_rank_processes_train_like_two_emulated_ranks(tmp_path):
    """``tools/train_denoiser.py --gpus 2`` for three steps on six 12 x 12 images (one training batch of four, two rows per
    rank; over RCCL with two GPUs visible, else ``--share-gpu``): exit status 0, both ranks print the same digest line, and
    rank 0's checkpoint holds the online, EMA and moment tensors of two emulated ranks run in this process on the same
    data with the same seed.  The tree is started once; on failure the launcher's report (the first failing rank's stderr
    tail) is the assertion message."""
    hr = R.uniform((6, 1, 12, 12), 4100).numpy()
    lr = R.uniform((6, 1, 12, 12), 4101).numpy()
    np.save(tmp_path / "hr.npy", hr)
    np.save(tmp_path / "lr.npy", lr)
    out_dir, log_dir = str(tmp_path / "out"), str(tmp_path / "ranks")
    argv = ["--data", "mnist", "--hr", str(tmp_path / "hr.npy"), "--lr", str(tmp_path / "lr.npy"), "--steps", "3", "--batch-size", "4",
            "--timesteps", "4", "--train-lr", "1e-3", "--save-every", "3", "--seed", "11", "--out", out_dir, "--gpus", "2"]
    share = launch.visible_gpus() < 2
    if share:
        argv.append("--share-gpu")
    print("two ranks " + ("share one GPU over gloo (staged exchange)" if share else "over RCCL"))
    report = io.StringIO()
    rc = launch.launch_ranks([sys.executable, os.path.join(ROOT, "tools", "train_denoiser.py")] + argv, 2, timeout_s=150.0,
                             grace_s=10.0, log_dir=log_dir, share_gpu=share, out=report)
    assert rc == 0, report.getvalue()
    digests = [[ln for ln in open(os.path.join(log_dir, f"rank{r}.out")) if ln.startswith("replica digest")] for r in range(2)]
    assert len(digests[0]) == 1 and digests[0] == digests[1] and "step 3" in digests[0][0], digests
    assert os.path.exists(os.path.join(out_dir, "train_loss.csv")) and os.path.exists(os.path.join(out_dir, "loss.csv"))
    data = torch.load(os.path.join(out_dir, "model-best100.pt"), map_location="cpu", weights_only=True)
    # the same run in this process: two emulated ranks set up by the tool's own code
    tool = load_tool()
    a = tool.parse(argv)
    ranks, train = [], None
    for r in range(2):
        tr, train, _ = tool.setup(a, comm=EmulatedRank(2, r))
        ranks.append(tr)
    assert len(train) == 1 and train[0][0].shape[0] == 4
    torch.manual_seed(a.seed)
    for _ in range(3):
        host_rng = torch.get_rng_state()
        for r, tr in enumerate(ranks):
            torch.set_rng_state(host_rng)                    # every rank draws t from the same generator state
            for bhr, blr in train:
                tr.accumulate(bhr[2 * r:2 * r + 2], blr[2 * r:2 * r + 2], scale=1.0 / (2 * len(train)))
        gathered = torch.stack([tr.send_buffer() for tr in ranks]).contiguous()
        for tr in ranks:
            tr.apply(gathered=gathered)
    tr = ranks[0]
    assert data["step"] == 3 and tr.step == 3
    ema, mom = tr.ema_state_dict(), tr.moments()
    for i, (k, p) in enumerate(tr.online_model.named_parameters()):
        assert torch.equal(data["model"]["model." + k], p.detach().cpu()), k
        assert torch.equal(data["ema"]["ema_model.model." + k], ema[k].cpu()), k
        if k in mom:
            assert torch.equal(data["opt"]["state"][i]["exp_avg"], mom[k][0].cpu()), k
            assert torch.equal(data["opt"]["state"][i]["exp_avg_sq"], mom[k][1].cpu()), k
    assert not torch.equal(data["model"]["model.init_conv.weight"], R.state("mnist")["init_conv.weight"])
