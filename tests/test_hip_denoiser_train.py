"""GPU tests of the seventh slice of the denoiser's backward pass: ``ld_dn_opt_sqnorm`` / ``ld_dn_opt_step`` of
csrc/denoiser_opt.hip alone on synthetic tensor tables, then ``DenoiserTrainer`` as a whole.

Yardsticks: CPU ``clip_grad_norm_`` + ``torch.optim.Adam(foreach=False)`` + the EMA rule written out literally
(tests/denoiser_train_ref.py), fed with the same gradients.  Parameters and a lerped EMA are held to the rule of
test_hip_mnistcls.py and test_hip_segtrain.py, ``allclose(rtol 2.4e-7, atol 1e-5 lr)`` of fp32 torch; the moments to a relative
error of 1e-5 of an fp64 replica (where a wrong clip coefficient shows: Adam's update itself is nearly invariant to the
gradient's scale); sums to max(1e-5, 4 d) of the fp64 value, d = fp32 torch's own distance; forwards to test_hip_unet.py's
2e-4 max(1, scale).  Every model runs with ``debug_fill = NaN``; the kernels' flat buffers sit between canaries."""
import ctypes as C
import functools
import math

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import checkpoint, rng

from hip_helpers import DEV, NAN, st
import denoiser_train_ref as T
import unet_grad_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
CANARY, PAD = 7.5, 64
LR = 1e-3
OPTS = dict(branch_out=False, start_intermediate=False, start_timestep=2, mask_x=False, ood_AD=False, ood_confidence=False,
            classifier=False, use_gt=False)
TIMESTEPS = 250


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
SIZES = [1, 3, 2, 5, 32, 1000, 4099, 4097, 294912]        # (2 and 4099: the entries without moments)
NO_MOMENTS = (2, 6)
MISALIGNED = 5                                            # this entry's parameter starts 4 bytes off a 16-byte boundary


class Table:
    """A synthetic table: the parameters lie in one canaried buffer (16-byte aligned starts, one entry off by a float), the
    four flat buffers and the work buffer between canaries."""

    def __init__(self):
        lib = cabi.lib()
        n = len(SIZES)
        starts, at = [], PAD
        for i, c in enumerate(SIZES):
            at = (at + 3) // 4 * 4 + (1 if i == MISALIGNED else 0)
            starts.append(at)
            at += c
        self.starts, self.params = starts, torch.full((at + PAD,), CANARY, dtype=F32, device=DEV)
        host = (cabi.DnOptTensor * n)()
        for i, (e, c) in enumerate(zip(host, SIZES)):
            e.param, e.count, e.flags = self.params.data_ptr() + 4 * starts[i], c, (0 if i in NO_MOMENTS else 1)
        flat, wgs = cabi.i64(), cabi.i64()
        cabi.check(lib.ld_dn_opt_layout(host, n, C.byref(flat), C.byref(wgs)), "dn_opt_layout")
        self.n, self.flat, self.n_wg = n, int(flat.value), int(wgs.value)
        self.off = [int(e.offset) for e in host]
        assert all(o % 4 == 0 for o in self.off) and host[MISALIGNED].param % 16 == 4 and host[0].param % 16 == 0
        self.table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
        self.bufs = {k: torch.full((self.flat + 2 * PAD,), CANARY, dtype=F32, device=DEV) for k in ("grad", "m", "v", "ema")}
        assert int(lib.ld_dn_opt_sqnorm_work_bytes(self.n_wg)) == 8 * self.n_wg
        self.work = torch.full((self.n_wg + 1 + 2 * PAD,), CANARY, dtype=F64, device=DEV)

    def ptr(self, k):
        return self.bufs[k].data_ptr() + 4 * PAD

    def seg(self, k, i):
        t = self.params if k == "p" else self.bufs[k]
        at = self.starts[i] if k == "p" else PAD + self.off[i]
        return t[at:at + SIZES[i]]

    def sumsq_ptr(self):
        return self.work.data_ptr() + 8 * PAD

    def sqnorm(self):
        cabi.check(cabi.lib().ld_dn_opt_sqnorm(self.table.data_ptr(), self.n, self.n_wg, self.ptr("grad"), self.flat,
                                               self.sumsq_ptr() + 8, self.sumsq_ptr(), st()), "dn_opt_sqnorm")

    def step(self, max_norm, t, mode, w):
        cabi.check(cabi.lib().ld_dn_opt_step(self.table.data_ptr(), self.n, self.n_wg, self.ptr("grad"), self.ptr("m"),
                                             self.ptr("v"), self.ptr("ema"), self.flat, self.sumsq_ptr(), max_norm, *T.ADAM["betas"],
                                             T.ADAM["eps"], LR / (1 - T.ADAM["betas"][0] ** t),
                                             math.sqrt(1 - T.ADAM["betas"][1] ** t), mode, w, st()), "dn_opt_step")

    def snapshot(self):
        return {k: v.clone() for k, v in dict(self.bufs, p=self.params, work=self.work).items()}

    def restore(self, snap):
        for k, v in snap.items():
            (self.params if k == "p" else self.work if k == "work" else self.bufs[k]).copy_(v)

    def outside_is_untouched(self):
        """The canaries around and between the segments of every buffer."""
        for k in ("grad", "m", "v", "ema", "p"):
            t = (self.params if k == "p" else self.bufs[k]).cpu()
            keep = torch.ones(t.numel(), dtype=torch.bool)
            for i, c in enumerate(SIZES):
                at = self.starts[i] if k == "p" else PAD + self.off[i]
                keep[at:at + c] = False
            assert bool((t[keep] == CANARY).all()), k
        w = self.work.cpu()
        assert bool((w[:PAD] == CANARY).all()) and bool((w[PAD + 1 + self.n_wg:] == CANARY).all())


def test_kernels_on_a_synthetic_table():
    """Tensor sizes 1, 3, 5, 32, 1,000, 4,097 and 294,912 with moments and 2 and 4,099 without, one parameter off the 16-byte
    grid: ``sqnorm`` under the reduction bound; ``ld_dn_opt_step`` calls at total norms 0.5, 3 and 40 (max_norm 1) with
    ema_mode 1, 2 (w 0.25), 0, and a fourth at norm 0.9 with ema_mode 2 and w 0.63 (the other branch of the lerp) -- parameters, moments, EMA, zeroed gradients, untouched canaries and entries without moments,
    identical bits from the same state.  MI355X: sum of squares at most 1.1e-16 of fp64 (fp32 torch up to 1.1e-7), parameters
    and lerped EMA 0.46 of the allclose bound, exp_avg 1.25e-7, exp_avg_sq 1.81e-7 (bound 1e-5)."""
    tb = Table()
    adam = [i for i in range(tb.n) if i not in NO_MOMENTS]
    p0 = [R.uniform((c,), 3000 + i) for i, c in enumerate(SIZES)]
    for i in range(tb.n):
        tb.seg("p", i).copy_(p0[i])
        tb.seg("ema", i).copy_(R.uniform((SIZES[i],), 3100 + i))
        if i in adam:
            tb.seg("m", i).zero_()
            tb.seg("v", i).zero_()
    rep32 = T.Replica({str(i): p0[i] for i in range(tb.n)}, LR, 1.0, F32, None, no_grad=[str(i) for i in NO_MOMENTS])
    rep64 = T.Replica({str(i): p0[i] for i in range(tb.n)}, LR, 1.0, F64, None, no_grad=[str(i) for i in NO_MOMENTS])
    worst = dict(p=0.0, m=0.0, v=0.0, ema=0.0)
    for call, (norm, mode, w) in enumerate(((0.5, 1, 0.0), (3.0, 2, 0.25), (40.0, 0, 0.0), (0.9, 2, 0.63)), start=1):
        raw = {i: R.uniform((SIZES[i],), 3200 + 10 * call + i) for i in adam}
        scale = norm / math.sqrt(sum(float((g.double() ** 2).sum()) for g in raw.values()))
        grads = {i: (g.double() * scale).float() for i, g in raw.items()}
        for i in range(tb.n):
            tb.seg("grad", i).copy_(grads[i] if i in adam else torch.full((SIZES[i],), NAN))
        before = tb.snapshot()
        ema_before = [tb.seg("ema", i).cpu() for i in range(tb.n)]
        tb.sqnorm()
        ss64 = sum((g.double() ** 2).sum() for g in grads.values())
        ss32 = sum((g ** 2).sum() for g in grads.values())
        got_ss = tb.work[PAD].cpu()
        R.reduction_bound(got_ss, ss64, ss32, f"call {call}: sum of squares (norm {norm})")
        tb.step(1.0, call, mode, w)
        after = tb.snapshot()
        tb.restore(before)                                   # a second run from the same state: identical bits
        tb.sqnorm()
        tb.step(1.0, call, mode, w)
        again = tb.snapshot()
        for k in after:
            assert torch.equal(after[k].view(torch.int32 if k != "work" else torch.int64),
                               again[k].view(torch.int32 if k != "work" else torch.int64)), (call, k)
        tb.outside_is_untouched()
        rep32.step({str(i): g for i, g in grads.items()})
        rep64.step({str(i): g for i, g in grads.items()})
        assert (rep64.norm > 1.0) == (norm > 1.0)
        for i in range(tb.n):
            p, e = tb.seg("p", i).cpu(), tb.seg("ema", i).cpu()
            if i in adam:
                worst["p"] = max(worst["p"], T.adam_close(p, rep32.p[str(i)].detach(), LR, f"call {call} param {i}"))
                m64, v64 = rep64.moments(str(i))
                em, ev = R.rel_err(tb.seg("m", i).cpu(), m64), R.rel_err(tb.seg("v", i).cpu(), v64)
                worst["m"], worst["v"] = max(worst["m"], em), max(worst["v"], ev)
                assert em <= 1e-5 and ev <= 1e-5, (call, i, em, ev)
                assert bool((tb.seg("grad", i) == 0).all()), (call, i)
            else:                                           # in the EMA and nowhere else
                assert torch.equal(p, p0[i]), (call, i)
                assert bool(tb.seg("grad", i).isnan().all()), (call, i)
                assert bool((tb.seg("m", i) == CANARY).all()) and bool((tb.seg("v", i) == CANARY).all()), (call, i)
            if mode == 1:
                assert torch.equal(e, p), (call, i)
            elif mode == 2:
                worst["ema"] = max(worst["ema"], T.adam_close(e, torch.lerp(ema_before[i], p, w), LR, f"call {call} ema {i}"))
                assert not torch.equal(e, ema_before[i]) or i not in adam        # (an untrained entry's EMA is its parameter already)
            else:
                assert torch.equal(e, ema_before[i]), (call, i)
        rep32.reset_params({str(i): tb.seg("p", i).cpu() for i in adam})
    print(f"synthetic table: params {worst['p']:.2f} and lerped ema {worst['ema']:.2f} of the allclose bound; moments rel err "
          f"exp_avg {worst['m']:.2e}, exp_avg_sq {worst['v']:.2e} (bound 1e-5)")


def test_a_non_finite_norm_is_not_hidden():
    """One NaN (then one inf) gradient element: the norm in device memory is NaN (inf), and the step does what torch does --
    every trained parameter NaN after a NaN norm; after an inf norm coef is 0, so inf * 0 = NaN at that element only."""
    for bad in (NAN, float("inf")):
        tb = Table()
        for i in range(tb.n):
            tb.seg("p", i).copy_(R.uniform((SIZES[i],), 3000 + i))
            for k in ("m", "v", "ema", "grad"):
                tb.seg(k, i).fill_(0.125)
        tb.seg("grad", 5)[17] = bad
        tb.sqnorm()
        got = float(tb.work[PAD].cpu())
        assert math.isnan(got) if math.isnan(bad) else got == float("inf")
        tb.step(1.0, 1, 0, 0.0)
        nan = [bool(tb.seg("p", i).isnan().all()) for i in range(tb.n) if i not in NO_MOMENTS]
        some = bool(tb.seg("p", 5).isnan()[17])
        assert all(nan) if math.isnan(bad) else (some and int(tb.seg("p", 5).isnan().sum()) == 1 and not nan[0])
        tb.outside_is_untouched()


def test_refusals_write_nothing():
    """Null or misaligned pointers, a zero count and a negative max_norm return -1 and write nothing."""
    lib = cabi.lib()
    tb = Table()
    before = tb.snapshot()
    a = (tb.table.data_ptr(), tb.n, tb.n_wg, tb.ptr("grad"), tb.ptr("m"), tb.ptr("v"), tb.ptr("ema"), tb.flat, tb.sumsq_ptr())
    adam = (0.9, 0.99, 1e-8, 1e-3, 0.1)

    def step(a, max_norm=1.0, mode=1, w=0.5):
        return lib.ld_dn_opt_step(*a, max_norm, *adam, mode, w, st())

    def swap(i, v):
        return a[:i] + (v,) + a[i + 1:]
    for i in (0, 3, 4, 5, 6, 8):
        assert step(swap(i, None)) == -1 and b"null" in lib.ld_last_error(), i
        assert step(swap(i, a[i] + 4)) == -1 and b"aligned" in lib.ld_last_error(), i
    assert step(swap(1, 0)) == -1 and step(swap(2, 0)) == -1 and step(swap(7, 0)) == -1 and step(swap(7, tb.flat + 2)) == -1
    assert step(a, max_norm=-1.0) == -1 and b"max_norm" in lib.ld_last_error()
    assert step(a, mode=3) == -1 and step(a, mode=2, w=1.5) == -1
    s = (tb.table.data_ptr(), tb.n, tb.n_wg, tb.ptr("grad"), tb.flat, tb.sumsq_ptr() + 8, tb.sumsq_ptr())
    for i in (0, 3, 5, 6):
        bad = s[:i] + (None,) + s[i + 1:]
        assert lib.ld_dn_opt_sqnorm(*bad, st()) == -1 and b"null" in lib.ld_last_error(), i
        bad = s[:i] + (s[i] + 4,) + s[i + 1:]
        assert lib.ld_dn_opt_sqnorm(*bad, st()) == -1 and b"aligned" in lib.ld_last_error(), i
    assert lib.ld_dn_opt_sqnorm(*(s[:1] + (0,) + s[2:]), st()) == -1
    torch.cuda.synchronize()
    after = tb.snapshot()
    for k in before:
        assert torch.equal(before[k], after[k]), k


# ------------------------------------------------------------------------------------------------ 2. the trainer
def make_diffusion(data, sd=None, image_size=28, timesteps=TIMESTEPS, objective="pred_v", seed=0):
    inf = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **R.KWARGS[data])
    inf.load_state_dict(R.state(data, seed) if sd is None else sd)
    return ldh.GaussianDiffusion(dict(OPTS, data=data), inf, image_size=image_size, timesteps=timesteps, objective=objective).to(DEV)


def make_trainer(data, **kw):
    args = dict(train_lr=LR, ema_update_every=T.EMA_KW["update_every"], ema_update_after_step=T.EMA_KW["update_after_step"])
    args.update(kw)
    tr = ldh.DenoiserTrainer(make_diffusion(data), **args)
    tr.online_model.debug_fill = NAN
    return tr


def dev_batch(case, step, j):
    return tuple(v.to(DEV) for v in T.batch(case, step, j, TIMESTEPS))


def train_step(tr, case, step, n_batches=2):
    """``DenoiserTrainer.train_step`` with explicit ``t`` and noise (what ``train_step`` does, batch by batch)."""
    total = None
    for j in range(n_batches):
        hr, lr, t, noise = dev_batch(case, step, j)
        value = tr.accumulate(hr, lr, scale=1.0 / n_batches, t=t, noise=noise)
        total = value if total is None else total + value
    return total


def cpu_state(tr):
    p = {k: v.detach().cpu() for k, v in tr.online_model.named_parameters()}
    ema = {k: v.cpu() for k, v in tr.ema_state_dict().items()}
    mom = {k: (m.cpu(), v.cpu()) for k, (m, v) in tr.moments().items()}
    return p, ema, mom


@pytest.mark.parametrize("case", R.CASES)
def test_steps_given_the_same_gradients(case):
    """Eight ``train_step``s of two batches (data, t and noise differ, all explicit; lr 1e-3; EMA every 2 calls after call 2):
    the six the EMA needs for copy, skip, copy, skip, first-use copy + lerp, skip, and two more so that a lerp of an
    initialised EMA (call 6, decay 1 - 5^(-2/3)) and the skip behind it occur.  Before each ``apply()`` the accumulated
    ``.grad``s go to the CPU replicas (clip, Adam, the literal EMA rule); parameters, moments and EMA step by step as in the
    kernel test, the replica's parameters and EMA reset to the kernel's after each comparison; the mode and decay the launch
    was given are the rule's, and after the true lerp the EMA is neither the online weights nor the EMA before it;
    ``conv_fusion.mlp.1.*`` keep their values, have no ``.grad``, and their EMA equals them.  MI355X (mri / mnist / mvtec): parameters and EMA 0.47 / 0.46 / 0.47 of
    the allclose bound, exp_avg 4.8e-7 / 1.7e-6 / 3.0e-7, exp_avg_sq 3.5e-7 / 3.5e-7 / 3.7e-7 (bound 1e-5)."""
    data = case[0]
    tr = make_trainer(data)
    sd = R.state(data)
    rep32 = T.Replica(sd, LR, 1.0, F32, T.EMA_KW)
    rep64 = T.Replica(sd, LR, 1.0, F64, None)
    worst = dict(p=0.0, m=0.0, v=0.0, ema=0.0)
    seen, sent = [], []
    ema_prev = {k: v.clone() for k, v in sd.items()}
    for step in range(8):
        train_step(tr, case, step)
        grads = {}
        for k, p in tr.online_model.named_parameters():
            if k in T.NO_GRAD:
                assert p.grad is None or not bool(p.grad.any()), k
            else:
                grads[k] = p.grad.detach().cpu().clone()
        tr.apply()
        sent.append(tr.last_ema)
        seen.append(rep32.step(grads))
        rep64.step(grads)
        p, ema, mom = cpu_state(tr)
        for k in sd:
            if k in T.NO_GRAD:
                assert torch.equal(p[k], sd[k]) and torch.equal(ema[k], sd[k]) and k not in mom, k
                continue
            worst["p"] = max(worst["p"], T.adam_close(p[k], rep32.p[k].detach(), LR, f"{case} step {step} {k}"))
            worst["ema"] = max(worst["ema"], T.adam_close(ema[k], rep32.ema[k], LR, f"{case} step {step} ema {k}"))
            m64, v64 = rep64.moments(k)
            em, ev = R.rel_err(mom[k][0], m64), R.rel_err(mom[k][1], v64)
            worst["m"], worst["v"] = max(worst["m"], em), max(worst["v"], ev)
            assert em <= 1e-5 and ev <= 1e-5, (step, k, em, ev)
            assert not bool(tr.online_model.get_parameter(k).grad.any()), k
            if step == 6:                                    # the true lerp
                assert not torch.equal(ema[k], p[k]) and not torch.equal(ema[k], ema_prev[k]), k
            elif sent[-1][0] == 1:
                assert torch.equal(ema[k], p[k]), (step, k)
            else:
                assert torch.equal(ema[k], ema_prev[k]), (step, k)
        assert abs(tr.check_finite() - rep64.norm) <= 1e-5 * rep64.norm
        rep32.reset_params({k: p[k] for k in grads}, {k: ema[k] for k in grads})
        ema_prev = ema
    assert seen == ["copy", "skip", "copy", "skip", "lerp", "skip", "lerp", "skip"]
    assert [m for m, _ in sent] == [1, 0, 1, 0, 1, 0, 2, 0] and sent[6][1] == pytest.approx(1.0 - 5.0 ** (-2.0 / 3.0), rel=1e-12)
    assert (tr.step, tr.ema_step, tr.ema_initted) == (8, 8, True)
    print(f"{case}: eight steps: params {worst['p']:.2f} and ema {worst['ema']:.2f} of the allclose bound; moments rel err exp_avg "
          f"{worst['m']:.2e}, exp_avg_sq {worst['v']:.2e} (bound 1e-5); last norm {rep64.norm:.3f}")


@functools.lru_cache(maxsize=None)
def mnist_yardsticks(steps):
    case = R.CASES[1]
    gd = make_diffusion("mnist")
    schedule = tuple(getattr(gd, n).cpu() for n in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "loss_weight"))
    args = (case, R.state("mnist"), schedule, "pred_v", LR, steps, 2, TIMESTEPS)
    return T.yardstick_steps(*args, F32)[0], T.yardstick_steps(*args, F64)[0]


def test_losses_follow_the_fp64_yardstick():
    """The summed losses ``train_step`` returns at the mnist case: the first three within max(1e-5, 4 d) of the fp64 CPU
    yardstick's (unet_forward + loss, clip, Adam), d = the fp32 yardstick's distance; steps 4 to 6 are printed, not asserted
    (Adam's first updates are close to lr sign(g), so elements with tiny gradients make two fp32 trajectories part).
    MI355X: 2.16601372 2.03211999 0.97347569, 1.27e-6 of the fp64 sequence (fp32 torch 4.2e-7, bound 1e-5); steps 4 to 6: HIP
    2.6e-6, 1.5e-5, 6.5e-5, fp32 torch 1.2e-6, 5.1e-6, 1.9e-5."""
    case = R.CASES[1]
    l32, l64 = mnist_yardsticks(6)
    tr = make_trainer("mnist")
    got = []
    for step in range(6):
        got.append(float(train_step(tr, case, step)))
        tr.apply()
    print("trainer losses: HIP " + " ".join(f"{v:.8f}" for v in got) + "; fp32 torch " + " ".join(f"{v:.8f}" for v in l32) +
          "; fp64 " + " ".join(f"{v:.8f}" for v in l64))
    for i in range(3, 6):
        print(f"step {i + 1}: HIP {abs(got[i] - l64[i]) / abs(l64[i]):.2e}, fp32 torch {abs(l32[i] - l64[i]) / abs(l64[i]):.2e} "
              "of the fp64 loss (not asserted)")
    R.reduction_bound(torch.tensor(got[:3], dtype=F64), torch.tensor(l64[:3], dtype=F64), torch.tensor(l32[:3], dtype=F64),
                      "trainer loss sequence, steps 1 to 3")


def forward_bound(got, ref, what):
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: out err {err:.3e} (ref max {scale:.3e}, bound {2e-4 * max(1.0, scale):.1e})")
    assert got.shape == ref.shape and err < 2e-4 * max(1.0, scale)


def fresh(data, sd):
    net = ldh.TrainableUnet(dim=32, init_dim=32, **R.KWARGS[data])
    net.load_state_dict(sd)
    net = net.to(DEV)
    net.debug_fill = NAN
    return net


def test_after_apply_the_modules_see_the_new_weights():
    """After ``apply()`` the online forward equals, bit for bit, a fresh ``TrainableUnet`` loaded with its ``state_dict`` and
    differs from the forward before the step; after ``sync_ema()`` ``diffusion.model`` agrees, on test_hip_unet.py's mnist28
    inputs, with a ``TrainableUnet`` loaded with ``ema_state_dict()`` under the forward bound."""
    case = R.CASES[1]
    tr = make_trainer("mnist")
    _, _, cond, time, _ = R.inputs(case)
    x = R.uniform((2, 1, 12, 12), 77)
    dev = [x.to(DEV), cond.to(DEV), time.to(DEV)]
    with torch.no_grad():
        before = tr.online_model(*dev)
    for step in range(2):
        train_step(tr, case, step)
        tr.apply()
        with torch.no_grad():
            after = tr.online_model(*dev)
            want = fresh("mnist", {k: v.detach().cpu() for k, v in tr.online_model.state_dict().items()})(*dev)
        assert torch.equal(after, want) and not torch.equal(after, before), step
        before = after
    big = [torch.from_numpy(rng.randn((4, 1, 28, 28), 1, 100)).to(DEV),
           torch.from_numpy(rng.uniform((4, 1, 28, 28), 1, 101, 0.0, 2.0)).to(DEV), torch.tensor([0, 7, 50, 99], device=DEV)]
    stale = tr.diffusion.model(*big).cpu()
    tr.sync_ema()
    ema = tr.ema_state_dict()
    assert torch.equal(ema["init_conv.weight"], tr.online_model.init_conv.weight) is False      # (call 1 was a skip)
    with torch.no_grad():
        mine = fresh("mnist", {k: v.cpu() for k, v in ema.items()})(*big).cpu()
    got = tr.diffusion.model(*big).cpu()
    forward_bound(got, mine, "diffusion.model after sync_ema vs TrainableUnet with the EMA weights")
    assert not torch.equal(got, stale)


def test_drawn_t_and_noise_are_the_diffusions():
    """``accumulate`` without ``t`` and ``noise`` draws what ``GaussianDiffusion.forward`` and ``p_losses`` draw from the same
    seeds (offset noise included): the same ``t``, and the loss of ``diffusion.p_losses`` on the online weights within the
    forward bound."""
    case = R.CASES[1]
    hr, lr, _, _ = T.batch(case, 0, 0, TIMESTEPS)
    tr = make_trainer("mnist")
    tr.diffusion.offset_noise_strength = 0.1
    torch.manual_seed(123)
    want_t = torch.randint(0, TIMESTEPS, (hr.shape[0],)).long()
    seen = {}

    def record(mod, args):
        seen["t"] = args[0].detach().cpu()
    hook = tr.online_model.time_mlp.register_forward_pre_hook(record)
    torch.manual_seed(123)
    value = tr.accumulate(hr.to(DEV), lr.to(DEV))
    hook.remove()
    assert torch.equal(seen["t"], want_t) and tr.diffusion._train_draw == 1           # (two draws: noise, offset noise)
    other = make_diffusion("mnist")                                  # the same seeds, the same (initial) weights
    other.offset_noise_strength = 0.1
    want = other.p_losses(hr.to(DEV), lr.to(DEV), want_t)
    err = abs(float(value) - float(want))
    print(f"drawn t {want_t.tolist()}: loss {float(value):.8f} vs p_losses {float(want):.8f} (err {err:.2e})")
    assert err < 2e-4 * max(1.0, abs(float(want)))


def test_save_load_and_three_more_steps(tmp_path):
    """``save`` after four steps, ``load`` into a second trainer (other weights), three more steps on both (a copy-free lerp
    among them): parameters, moments, EMA and counters bit-equal; ``load_reference_checkpoint`` into another diffusion samples
    with the EMA weights."""
    case = R.CASES[1]
    a = make_trainer("mnist")
    for step in range(4):
        train_step(a, case, step)
        a.apply()
    path = str(tmp_path / "model-best100.pt")
    a.save(path)
    b = ldh.DenoiserTrainer(make_diffusion("mnist", seed=5), train_lr=LR, ema_update_every=2, ema_update_after_step=2)
    b.online_model.debug_fill = NAN
    info = b.load(path)
    assert info["source"] == "ema" and (b.step, b.ema_step, b.ema_initted) == (4, 4, False) == (a.step, a.ema_step, a.ema_initted)
    for step in range(4, 7):
        for tr in (a, b):
            train_step(tr, case, step)
            tr.apply()
    sa, sb = cpu_state(a), cpu_state(b)
    for k in sa[0]:
        assert torch.equal(sa[0][k], sb[0][k]) and torch.equal(sa[1][k], sb[1][k]), k
        if k not in T.NO_GRAD:
            assert torch.equal(sa[2][k][0], sb[2][k][0]) and torch.equal(sa[2][k][1], sb[2][k][1]), k
        assert not torch.equal(sa[0][k], sa[1][k]) or k in T.NO_GRAD, k        # (call 6 lerped: the EMA is not the online copy)
    assert (b.step, b.ema_step, b.ema_initted) == (7, 7, True) == (a.step, a.ema_step, a.ema_initted)
    data = torch.load(path, map_location="cpu", weights_only=True)
    assert float(data["opt"]["state"][0]["step"]) == 4.0 and len(data["opt"]["state"]) == len(sa[0]) - 2
    other = make_diffusion("mnist", seed=6, image_size=12, timesteps=4, objective="pred_x0")
    with pytest.raises(RuntimeError):
        checkpoint.load_reference_checkpoint(path, other)                 # (250 timesteps do not fit 4)
    other = make_diffusion("mnist", seed=6, image_size=12)
    info = checkpoint.load_reference_checkpoint(path, other)
    assert info["source"] == "ema" and info["step"] == 4
    assert torch.equal(other.model.state_dict()["init_conv.weight"].cpu(), data["ema"]["ema_model.model.init_conv.weight"])
    assert not torch.equal(data["ema"]["ema_model.model.init_conv.weight"], data["model"]["model.init_conv.weight"])
    # ... and samples with them: the bits of a diffusion built on the file's EMA weights, not those of its online weights
    _, lr, _, _ = T.batch(case, 0, 0, TIMESTEPS)

    def sample_with(part, prefix):
        sd = {k[len(prefix):]: v for k, v in data[part].items() if k.startswith(prefix)}
        gd = make_diffusion("mnist", sd=sd, image_size=12)
        return gd.sample(lr.to(DEV), None, batch_size=lr.shape[0], min_max_val=(0.0, 1.0)).cpu()
    got = other.sample(lr.to(DEV), None, batch_size=lr.shape[0], min_max_val=(0.0, 1.0)).cpu()
    assert bool(got.isfinite().all()) and torch.equal(got, sample_with("ema", "ema_model.model."))
    assert not torch.equal(got, sample_with("model", "model."))


def test_evaluate_leaves_the_training_state_alone():
    """``evaluate`` on one mnist batch with 4 timesteps returns a finite number and leaves the online weights and the moments
    untouched, bit for bit."""
    case = R.CASES[1]
    tr = ldh.DenoiserTrainer(make_diffusion("mnist", image_size=12, timesteps=4, objective="pred_x0"), train_lr=LR,
                             ema_update_every=2, ema_update_after_step=2)
    tr.online_model.debug_fill = NAN
    hr, lr, _, noise = T.batch(case, 0, 0, 4)
    t = torch.tensor([1, 3])
    tr.accumulate(hr.to(DEV), lr.to(DEV), t=t.to(DEV), noise=noise.to(DEV))
    tr.apply()
    before = cpu_state(tr)
    ls = tr.evaluate([(hr, lr)], (0.0, 1.0))
    print(f"evaluate: mse {ls:.6f}")
    assert isinstance(ls, float) and math.isfinite(ls)
    after = cpu_state(tr)
    for k in before[0]:
        assert torch.equal(before[0][k], after[0][k]) and torch.equal(before[1][k], after[1][k]), k
        if k not in T.NO_GRAD:
            assert torch.equal(before[2][k][0], after[2][k][0]) and torch.equal(before[2][k][1], after[2][k][1]), k


def test_a_step_does_not_synchronise():
    """After a warm-up step, ``accumulate`` and ``apply`` run under ``set_sync_debug_mode('error')`` (first: the mode is live
    on this build, a lone ``.item()`` under it raises); ``check_finite`` is the one call that reads the norm back."""
    case = R.CASES[1]
    tr = make_trainer("mnist")
    hr, lr, t, noise = dev_batch(case, 0, 0)
    tr.accumulate(hr, lr, t=t, noise=noise)
    tr.apply()
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        with pytest.raises(RuntimeError):
            probe.item()
        value = tr.accumulate(hr, lr, scale=0.5, t=t, noise=noise)       # raises if anything synchronises
        drawn = tr.accumulate(hr, lr, scale=0.5)                          # t and noise drawn by the trainer
        tr.apply()
        with pytest.raises(RuntimeError):
            tr.check_finite()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert math.isfinite(float(value)) and math.isfinite(float(drawn)) and tr.check_finite() > 0.0 and tr.step == 2
