"""GPU tests of the sixth slice of the denoiser's backward pass: the time MLP kernels and ``ld_dn_join`` of csrc/unet_grad.hip one
by one, then ``TimeMLP`` and ``TrainableUnet`` as wholes -- the forward against the CPU oracle, the real reference's recorded
outputs and the inference ``Unet``; every parameter's gradient against torch.autograd in fp64; plain SGD and Adam on the
training loss.

Yardstick: torch.autograd on the CPU through tests/unet_grad_ref.py's restatement (equal to oracle.unet_ref.unet_forward bit
for bit in fp32: test_unet_grad.py).  Element-wise results are held to RTOL["fp32"] of fp32 torch, everything behind a sum to
max(1e-5, 4 d) of the fp64 value, d = fp32 eager torch's own distance to it (resblock_ref.reduction_bound), the forward to
test_hip_unet.py's 2e-4 max(1, scale).  The condition images are the ones for which no ReLU or pool tie of the encoder lies
within the margin (condenc_ref.ENCODER_KEYS) and the rest of the net is smooth, so no element is excluded anywhere.  Every
buffer handed to a kernel is filled with NaN first, padding included, and every module runs with ``debug_fill = NaN``.  Every
test prints HIP's and torch's distances (docs/findings.md, 127)."""
import functools

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import rng

from hip_helpers import DEV, NAN, RTOL, nans, padded, st
import resblock_ref
import unet_grad_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
GOLDEN_CASES = {"mnist28": ("mnist", 4, 28), "mri64": ("mri", 1, 64), "mvtec32": ("mvtec", 2, 32)}     # test_hip_unet.CASES


# ------------------------------------------------------------------------------------------------ 1. the time MLP kernels
TIME_CASES = [(1, 32), (3, 32), (5, 64), (130, 32)]


def time_vectors(B):
    """Times that include 0 and 999: B = 1 holds one of them per run."""
    if B == 1:
        return [torch.tensor([0]), torch.tensor([999])]
    t = (torch.arange(B) * 997 + 13) % 1000
    t[0], t[-1] = 0, 999
    return [t]


@functools.lru_cache(maxsize=None)
def time_case(B, dim, which):
    """Weights, times, dtemb and the two references of one case (computed once, never changed)."""
    T = 4 * dim
    sd = {"1.weight": R.uniform((T, dim), 700 + dim) / dim ** 0.5, "1.bias": R.uniform((T,), 701 + dim) / dim ** 0.5,
          "3.weight": R.uniform((T, T), 702 + dim) / T ** 0.5, "3.bias": R.uniform((T,), 703 + dim) / T ** 0.5}
    time = time_vectors(B)[which]
    dtemb = R.uniform((B, T), 704 + B) / B
    return sd, time, dtemb, R.time_mlp_yardstick(sd, time, dim, dtemb, F32), R.time_mlp_yardstick(sd, time, dim, dtemb, F64)


def hip_time_mlp(sd, time, dtemb, dim):
    lib = cabi.lib()
    B, T = time.shape[0], 4 * dim
    w = {k: v.to(DEV) for k, v in sd.items()}
    times, freqs = time.to(DEV, F32), R.freqs(dim).to(DEV)
    r = dict(emb=nans(B, dim), h1=nans(B, T), temb=nans(B, T))
    cabi.check(lib.ld_dn_time_mlp_forward(times.data_ptr(), freqs.data_ptr(), w["1.weight"].data_ptr(), w["1.bias"].data_ptr(),
                                          w["3.weight"].data_ptr(), w["3.bias"].data_ptr(), r["emb"].data_ptr(), r["h1"].data_ptr(),
                                          r["temb"].data_ptr(), B, dim, T, st()), "dn_time_mlp_forward")
    nbytes = int(lib.ld_dn_time_mlp_work_bytes(B, dim, T))
    assert nbytes == 2 * B * T * 4
    work = nans(nbytes // 4)
    r.update({"1.weight": nans(T, dim), "1.bias": nans(T), "3.weight": nans(T, T), "3.bias": nans(T)})
    d = dtemb.to(DEV)
    cabi.check(lib.ld_dn_time_mlp_backward(d.data_ptr(), r["emb"].data_ptr(), r["h1"].data_ptr(), w["3.weight"].data_ptr(),
                                           work.data_ptr(), r["1.weight"].data_ptr(), r["1.bias"].data_ptr(),
                                           r["3.weight"].data_ptr(), r["3.bias"].data_ptr(), B, dim, T, st()), "dn_time_mlp_backward")
    return r


@pytest.mark.parametrize("B,dim", TIME_CASES)
def test_time_mlp_kernels_and_module(B, dim):
    """ld_dn_time_mlp_forward / ld_dn_time_mlp_backward at one sample, a few, and more samples (130) than a workgroup has
    waves or a wave has lanes, at dim 32 and 64, times 0 and 999 among them: emb, h1 and temb within RTOL of fp32 torch given
    the same frequency table, the four parameter gradients under the reduction bound, a second call the same bits; ``TimeMLP``
    gives the kernels' bits under ``backward`` and under ``autograd.grad``, from int64, int32 and float32 times.  MI355X: see
    docs/findings.md 127."""
    for which in range(len(time_vectors(B))):
        sd, time, dtemb, (e32, h32, t32, g32), (e64, h64, t64, g64) = time_case(B, dim, which)
        assert 0 in time.tolist() or 999 in time.tolist()
        r = hip_time_mlp(sd, time, dtemb, dim)
        tag = f"time MLP B{B} dim{dim} t{time.tolist()[:3]}"
        for k, want32, want64 in (("emb", e32, e64), ("h1", h32, h64), ("temb", t32, t64)):
            resblock_ref.elementwise_bound(r[k].cpu(), want32, want64, f"{tag} {k}", rtol=RTOL["fp32"])
        for k in g64:
            R.reduction_bound(r[k].cpu(), g64[k], g32[k], f"{tag} d {k}")
        again = hip_time_mlp(sd, time, dtemb, dim)
        for k in r:
            assert torch.equal(r[k], again[k]), k
        mlp = ldh.TimeMLP(dim)
        mlp.load_state_dict(sd)
        mlp = mlp.to(DEV)
        mlp.debug_fill = NAN
        for tt in (time, time.to(torch.int32), time.to(F32)):
            mlp.zero_grad(set_to_none=True)
            out = mlp(tt.to(DEV))
            assert torch.equal(out, r["temb"])
            out.backward(dtemb.to(DEV))
            for k, p in mlp.named_parameters():
                assert torch.equal(p.grad, r[k]), k
        grads = torch.autograd.grad(mlp(time.to(DEV)), list(mlp.parameters()), grad_outputs=dtemb.to(DEV))
        for (k, _), g in zip(mlp.named_parameters(), grads):
            assert torch.equal(g, r[k]), k
        with torch.no_grad():
            quiet = mlp(time.to(DEV))
        assert not quiet.requires_grad and torch.equal(quiet, r["temb"])


# ------------------------------------------------------------------------------------------------ 2. the glue kernel
@pytest.mark.parametrize("ca,lda,cb,ldb,ldo", [(32, 64, 32, 64, 64), (64, 64, 32, 64, 128), (256, 256, 256, 256, 512),
                                               (32, 64, None, None, 64)])
def test_join_is_bit_equal_to_cat_and_add(ca, lda, cb, ldb, ldo):
    """ld_dn_join at B = 2, 5 x 3: bit-equal to torch.cat (``a2`` null) or to ``+`` (``b`` null), the output's padding zero,
    the sources' padding (NaN here) never read; 96 real channels leave 32 zero columns.  MI355X: bit-equal."""
    lib = cabi.lib()
    B, H, W = 2, 5, 3
    a = R.uniform((B, ca, H, W), 800 + ca)
    ap = padded(a, lda)
    out = nans(B, H, W, ldo)
    if cb is None:
        a2 = R.uniform((B, ca, H, W), 801 + ca)
        a2p = padded(a2, lda)
        cabi.check(lib.ld_dn_join(ap.data_ptr(), a2p.data_ptr(), None, out.data_ptr(), B, H, W, ca, lda, 0, 0, ldo, st()), "dn_join")
        want, real = a + a2, ca
    else:
        b = R.uniform((B, cb, H, W), 802 + cb)
        bp = padded(b, ldb)
        cabi.check(lib.ld_dn_join(ap.data_ptr(), None, bp.data_ptr(), out.data_ptr(), B, H, W, ca, lda, cb, ldb, ldo, st()),
                   "dn_join")
        want, real = torch.cat((a, b), dim=1), ca + cb
    got = out.cpu()
    assert torch.equal(got[..., :real].permute(0, 3, 1, 2), want)
    assert bool((got[..., real:] == 0).all())
    print(f"join ca{ca}/{lda} cb{cb}/{ldb} -> {ldo}: bit-equal, {ldo - real} zero columns")


# ------------------------------------------------------------------------------------------------ 3. the forward
def build(data, sd=None):
    net = ldh.TrainableUnet(dim=32, init_dim=32, **R.KWARGS[data])
    net.load_state_dict(R.state(data) if sd is None else sd)
    net = net.to(DEV)
    net.debug_fill = NAN
    return net


@functools.lru_cache(maxsize=None)
def case_refs(case):
    """Inputs and the two yardsticks of one small case (computed once, never changed)."""
    sd, x, cond, time, dout = R.inputs(case)
    cfg = R.CONFIGS[case[0]]
    return sd, x, cond, time, dout, R.yardstick(cfg, sd, x, cond, time, dout, F32), R.yardstick(cfg, sd, x, cond, time, dout, F64)


def forward_bound(got, ref, what):
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: out err {err:.3e} (ref max {scale:.3e}, bound {2e-4 * max(1.0, scale):.1e})")
    assert got.shape == ref.shape and err < 2e-4 * max(1.0, scale)
    return err


@pytest.mark.parametrize("case", R.CASES)
def test_forward_against_the_oracle(case):
    """``TrainableUnet`` at the three small cases against the fp32 CPU oracle under test_hip_unet.py's fp32 bound; a grad-mode
    and a no_grad forward give the same bits.  MI355X: see docs/findings.md 127."""
    sd, x, cond, time, _, (o32, _), (o64, _) = case_refs(case)
    net = build(case[0])
    with torch.no_grad():
        out = net(x.to(DEV), cond.to(DEV), time.to(DEV))
    assert out.is_contiguous() and not out.requires_grad
    forward_bound(out.cpu(), o32, f"{case} vs the fp32 oracle")
    print(f"{case}: to fp64: HIP {R.rel_err(out.cpu(), o64):.2e}, fp32 torch {R.rel_err(o32, o64):.2e}")
    loud = net(x.to(DEV), cond.to(DEV), time.to(DEV))
    assert loud.requires_grad and torch.equal(loud.detach(), out)


@pytest.mark.parametrize("tag", list(GOLDEN_CASES))
def test_forward_against_the_references_recorded_outputs(golden, tag):
    """The three ``g2_unet_forward`` cases (mnist 4 x 28^2, mri 1 x 64^2, mvtec 2 x 32^2, every recorded timestep): the real
    reference's outputs under the same bound, and ``ldh.Unet(compute_dtype='fp32')`` after ``load_state_dict`` in both
    directions (the sizes test_hip_unet.py runs the inference net at).  MI355X: see docs/findings.md 127."""
    data, B, H = GOLDEN_CASES[tag]
    g = golden("g2_unet_forward")
    net = build(data)
    cfg = net.cfg
    x = torch.from_numpy(rng.randn((B, cfg.channels, H, H), 1, 100)).to(DEV)
    cond = torch.from_numpy(rng.uniform((B, cfg.cond_in_channels, H, H), 1, 101, 0.0, 2.0)).to(DEV)
    steps = [int(k.split("_t")[1].split("_")[0]) for k in g.files if k.startswith(tag) and k.endswith("_out")]
    assert steps
    for t in steps:
        with torch.no_grad():
            y = net(x, cond, torch.full((B,), t, dtype=torch.long, device=DEV)).cpu()
        forward_bound(y, torch.from_numpy(g[f"{tag}_t{t}_out"]), f"{tag} t={t} vs the reference's recorded output")
    tv = torch.full((B,), steps[-1], dtype=torch.long, device=DEV)
    inf = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **R.KWARGS[data])
    inf.load_state_dict(net.state_dict())
    forward_bound(y, inf.to(DEV)(x, cond, tv).cpu(), f"{tag} vs ldh.Unet loaded from it")
    back = build(data, inf.state_dict())
    with torch.no_grad():
        assert torch.equal(back(x, cond, tv).cpu(), y)


# ------------------------------------------------------------------------------------------------ 4. the gradients
def hip_forward_backward(net, x, cond, time, dout, zero=True):
    if zero:
        net.zero_grad(set_to_none=True)
    out = net(x.to(DEV), cond.to(DEV), time.to(DEV))
    out.backward(dout.to(DEV))
    return out.detach(), {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}


@pytest.mark.parametrize("case", R.CASES)
def test_every_parameter_gradient(case):
    """Every parameter's gradient of sum(out * dout) at the three small cases under max(1e-5, 4 d); ``conv_fusion.mlp.1.*`` are
    not used (the reference calls conv_fusion without a time embedding) and keep ``.grad is None``; a second forward + backward
    gives identical bits; a second ``backward`` without ``zero_grad`` doubles ``.grad``.  MI355X, largest rel err to fp64, HIP /
    fp32 eager torch: mri 9.3e-6 / 9.3e-6 and mvtec 7.4e-6 / 7.4e-6 (both at time_mlp.1.weight, bounds 3.7e-5 and 3.0e-5), mnist
    5.8e-6 / 3.1e-6; no gradient closer to its bound than 0.67 of it."""
    sd, x, cond, time, dout, (o32, g32), (o64, g64) = case_refs(case)
    net = build(case[0])
    out, grads = hip_forward_backward(net, x, cond, time, dout)
    forward_bound(out.cpu(), o32, f"{case} out")
    assert list(grads) == list(g64)
    unused = [k for k, v in g64.items() if v is None]
    assert unused == ["conv_fusion.mlp.1.weight", "conv_fusion.mlp.1.bias"]
    worst = (0.0, 0.0, "")
    for k in g64:
        if g64[k] is None:
            assert grads[k] is None, k
            continue
        assert grads[k] is not None and grads[k].shape == g64[k].shape, k
        e, d = R.reduction_bound(grads[k].cpu(), g64[k], g32[k], f"{case} d {k}")
        worst = max(worst, (e, d, k))
    print(f"{case}: largest HIP rel err {worst[0]:.2e} (fp32 torch there {worst[1]:.2e}) at {worst[2]}; largest fp32 torch "
          f"{max(R.rel_err(g32[k], g64[k]) for k in g64 if g64[k] is not None):.2e}")
    out2, grads2 = hip_forward_backward(net, x, cond, time, dout)
    assert torch.equal(out, out2)
    for k in grads:
        assert (grads[k] is None and grads2[k] is None) or torch.equal(grads[k], grads2[k]), k
    _, grads3 = hip_forward_backward(net, x, cond, time, dout, zero=False)
    for k in grads:
        assert (grads[k] is None and grads3[k] is None) or torch.equal(grads3[k], 2 * grads[k]), k


# ------------------------------------------------------------------------------------------------ 5. training
@pytest.fixture(scope="module")
def training():
    """The mnist case as a training batch: x0, noise and times, x_t = q_sample on the CPU, the diffusion's schedule."""
    case = R.CASES[1]
    data, B, H, W = case
    assert data == "mnist"
    sd, _, cond, _, _ = R.inputs(case)
    inf = ldh.Unet(dim=32, init_dim=32, **R.KWARGS[data])
    inf.load_state_dict(sd)
    opts = dict(branch_out=False, start_intermediate=False, start_timestep=2, data="mnist", mask_x=False, ood_AD=False,
                ood_confidence=False, classifier=False, use_gt=False)
    gd = ldh.GaussianDiffusion(opts, inf, image_size=28, timesteps=250, objective="pred_v").to(DEV)
    schedule = tuple(getattr(gd, n).cpu() for n in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "loss_weight"))
    time = torch.tensor([3, 117])
    x0, noise = R.uniform((B, 1, H, W), 901), torch.from_numpy(rng.randn((B, 1, H, W), 7, 902))
    x = (schedule[0][time][:, None, None, None] * x0 + schedule[1][time][:, None, None, None] * noise).contiguous()
    return dict(gd=gd, schedule=schedule, sd=sd, cfg=R.CONFIGS[data], x=x, cond=cond, time=time, x0=x0, noise=noise, data=data)


def hip_step(tr, net, opt):
    """One training step on the fixed batch: the loss of the forward's output (fp64 on the CPU) and the optimiser's step."""
    dev = [tr[k].to(DEV) for k in ("x", "cond", "time", "x0", "noise")]
    opt.zero_grad()
    out = net(*dev[:3])
    value = float(R.loss(out.detach().cpu(), tr["x0"], tr["noise"], tr["time"], *tr["schedule"], "pred_v", F64))
    out.backward(tr["gd"].p_losses_grad(out, dev[3], dev[4], dev[2]))
    opt.step()
    return value


def test_three_sgd_steps_follow_the_fp64_losses(training):
    """Three plain SGD steps (lr 1e-3, at which the fp64 loss falls at every step) at the mnist case on a fixed batch, the loss ``GaussianDiffusion.p_losses_grad`` fed
    into ``out.backward``: the loss sequence within max(1e-5, 4 d) of the fp64 CPU sequence, d = fp32 eager torch's distance.
    MI355X: 1.64297740 1.39931932 1.14078828, 8.5e-8 of the fp64 sequence (fp32 torch 1.8e-7, bound 1e-5)."""
    tr = training
    lr, steps = 1e-3, 3
    args = (tr["cfg"], tr["sd"], tr["x"], tr["cond"], tr["time"], tr["x0"], tr["noise"], tr["schedule"], "pred_v", lr, steps)
    l64, _ = R.sgd_losses(*args, F64)
    l32, _ = R.sgd_losses(*args, F32)
    net = build(tr["data"])
    opt = torch.optim.SGD(net.parameters(), lr=lr)
    got = [hip_step(tr, net, opt) for _ in range(steps)]
    print("sgd losses: HIP " + " ".join(f"{v:.8f}" for v in got) + "; fp32 torch " + " ".join(f"{v:.8f}" for v in l32) +
          "; fp64 " + " ".join(f"{v:.8f}" for v in l64))
    assert l64[0] > l64[1] > l64[2]
    R.reduction_bound(torch.tensor(got, dtype=F64), torch.tensor(l64, dtype=F64), torch.tensor(l32, dtype=F64), "sgd loss sequence")


def test_an_adam_step_moves_the_packed_weights(training):
    """One ``torch.optim.Adam`` step: the next forward equals, bit for bit, that of a fresh ``TrainableUnet`` loaded with the
    stepped ``state_dict`` (the packed-weight caches follow ``_version``), differs from the forward before the step, and the
    stepped weights in ``ldh.Unet`` agree under the forward bound (at 4 x 28^2, a size the inference net is tested at)."""
    tr = training
    net = build(tr["data"])
    dev = [tr[k].to(DEV) for k in ("x", "cond", "time")]
    with torch.no_grad():
        before = net(*dev)
    hip_step(tr, net, torch.optim.Adam(net.parameters(), lr=1e-3))
    with torch.no_grad():
        after = net(*dev)
        fresh = build(tr["data"], {k: v.detach().cpu() for k, v in net.state_dict().items()})(*dev)
    assert not torch.equal(after, before)
    assert torch.equal(after, fresh)
    inf = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **R.KWARGS[tr["data"]])
    inf.load_state_dict(net.state_dict())
    big = [torch.from_numpy(rng.randn((4, 1, 28, 28), 1, 100)).to(DEV),                 # (test_hip_unet.py's mnist28 inputs)
           torch.from_numpy(rng.uniform((4, 1, 28, 28), 1, 101, 0.0, 2.0)).to(DEV), torch.tensor([0, 7, 50, 99], device=DEV)]
    with torch.no_grad():
        mine = net(*big)
    forward_bound(mine.cpu(), inf.to(DEV)(*big).cpu(), "after Adam vs ldh.Unet with the stepped weights")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_with_device_pointers():
    """Null or misaligned pointers and bad sizes return -1 and write nothing; the modules refuse what they cannot run."""
    lib = cabi.lib()
    buf = torch.zeros(8192, device=DEV)
    p, N = buf.data_ptr(), None
    assert lib.ld_dn_time_mlp_forward(p, p, p, p, p, p, p, p, N, 2, 32, 128, st()) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_time_mlp_forward(p, p, p, p, p, p, p, p, p, 2, 31, 128, st()) == -1
    assert lib.ld_dn_time_mlp_backward(p, p, p, p, p, p, p, p, p + 2, 2, 32, 128, st()) == -1 and b"aligned" in lib.ld_last_error()
    assert lib.ld_dn_join(p, N, p, p + 4, 2, 5, 3, 32, 64, 32, 64, 64, st()) == -1 and b"aligned" in lib.ld_last_error()
    assert lib.ld_dn_join(p, N, p, p + 16, 2, 5, 3, 48, 64, 32, 64, 128, st()) == -1
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
    net = ldh.TrainableUnet(dim=32, **R.KWARGS["mri"])
    with pytest.raises(ValueError, match="parameter"):
        net(torch.zeros(1, 1, 8, 8, device=DEV), torch.zeros(1, 1, 8, 8, device=DEV), torch.zeros(1, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError, match="divisible by 8"):
        net.to(DEV)(torch.zeros(1, 1, 12, 8, device=DEV), torch.zeros(1, 1, 12, 8, device=DEV),
                    torch.zeros(1, dtype=torch.long, device=DEV))
