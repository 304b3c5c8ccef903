"""The MNIST digit classifier and its training step on the GPU (csrc/mnistcls.hip) against golden G20 (the reference's own
SimpleCNN in fp64, and its fp32 spread in four arithmetic orders) and against the fp64 restatement of tests/mnistcls_ref.py.
Reads only tests/golden/.

Tolerances.  Whole-net quantities are held to 4 x the reference's own fp32-to-fp64 spread on the same inputs (G20's
``logit_spread``, ``grad_spread``, ``loss_spread``), the multiple G19's tests use.  Single kernels on small shapes are held to
hip_helpers.RTOL['fp32'] (2e-5 of the reference's largest value), the suite's fp32 bound; the pooling backward only routes
values and must be exact.  The gradients of the biases and of fc2 do not depend on which of two equal maxima a pooling
window routes to (a bias gradient is the sum over the window either way), so they are compared element by element with the
same 2e-5; the convolution and fc1 weights are compared in relative L2 only."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import localdiffusion_hallucination_amd as ldh                              # noqa: E402
from localdiffusion_hallucination_amd import _cabi as cabi                  # noqa: E402
from localdiffusion_hallucination_amd import checkpoint, evalio, rng, weights   # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hip_helpers import DEV, RTOL, rel_err, st                              # noqa: E402
import mnistcls_ref                                                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = RTOL["fp32"]
SMALL = ("conv1.bias", "conv2.bias", "fc1.bias", "fc2.weight", "fc2.bias")


def rnd(shape, key, lo=-1.0, hi=1.0):
    return torch.from_numpy(rng.uniform(shape, 2020, key, lo, hi))


def g20():
    g = np.load(os.path.join(GOLD, "g20_mnistcls.npz"))
    grads = np.load(os.path.join(GOLD, "g20_mnistcls_grads.npz"))
    d = np.load(os.path.join(GOLD, "g20_mnist_digits.npz"))
    sd = weights.procedural_mnistcls_state_dict(int(g["seed"]))
    x, y = mnistcls_ref.images_of(d["images"]), torch.from_numpy(d["labels"].astype(np.int64))
    return g, grads, sd, x, y


def g20_net(sd):
    net = ldh.MnistClassifier()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net.to(DEV)


# ------------------------------------------------------------------------------------------------ forward
def test_forward_logits_against_the_fp64_reference():
    """The golden batch against G20's fp64 logits, then B = 1, 3, 64, 200 against the restatement in fp64 run here: within
    4 x logit_spread.  The spreads and what has been measured: docs/findings.md 120."""
    g, _, sd, x, y = g20()
    net = g20_net(sd)
    bound = 4.0 * float(g["logit_spread"])
    z = net(x[:64].to(DEV))
    assert z.shape == (64, 10) and z.dtype == torch.float32 and z.is_cuda
    e = float((z.cpu().double() - torch.from_numpy(g["logits_init"])).abs().max())
    print(f"golden batch: HIP to fp64 {e:.3e} (logit_spread {float(g['logit_spread']):.3e}, bound {bound:.3e})")
    assert e <= bound
    params = mnistcls_ref.params_of(sd, torch.float64)
    for B in (1, 3, 64, 200):
        xb = x[100:100 + B]
        z64 = mnistcls_ref.forward(params, xb.double()).detach()
        e = float((net(xb.to(DEV)).cpu().double() - z64).abs().max())
        print(f"B = {B}: HIP to fp64 {e:.3e}")
        assert e <= bound, (B, e)


def test_predict_is_the_lowest_index_argmax_on_the_device():
    g, _, sd, x, y = g20()
    net = g20_net(sd)
    labels, logits = net.predict(x[:200].to(DEV))
    assert labels.is_cuda and logits.is_cuda and labels.dtype == torch.int64 and labels.shape == (200,)
    assert torch.equal(labels, logits.argmax(1)) and torch.equal(logits, net(x[:200].to(DEV)))
    # equal logits: fc2 zeroed leaves every logit at its bias; two equal largest biases -> the lower index
    net.fc2.weight.zero_()
    net.fc2.bias.copy_(torch.tensor([0.0, 1.0, 0.5, 3.0, 3.0, -1.0, 3.0, 0.0, 0.0, 0.0]))
    net.invalidate()
    labels, logits = net.predict(x[:5].to(DEV))
    assert labels.tolist() == [3] * 5 and torch.equal(logits[0].cpu(), net.fc2.bias.cpu())


# ------------------------------------------------------------------------------------------------ single kernels
def nhwc_pad(t, cs):
    """NCHW (cpu) -> NHWC on the device with the channels at a stride of cs (the rest zero)."""
    B, C_, H, W = t.shape
    out = torch.zeros((B, H, W, cs), device=DEV)
    out[..., :C_] = t.permute(0, 2, 3, 1).to(DEV)
    return out


@pytest.mark.parametrize("B", [1, 3])
def test_conv1_relu_pool_forward_and_its_weight_gradient(B):
    lib = cabi.lib()
    x = rnd((B, 1, 28, 28), 1, 0.0, 2.0)
    x[:, :, :6] = 0.0                                          # background rows: windows of equal values (the bias)
    w, b = rnd((32, 1, 3, 3), 2) / 3.0, rnd((32,), 3) / 3.0
    dp = rnd((B, 32, 14, 14), 4)
    x64, w64, b64 = x.double(), w.double().requires_grad_(True), b.double().requires_grad_(True)
    out64 = F.max_pool2d(F.relu(F.conv2d(x64, w64, b64, padding=1)), 2)
    gw64, gb64 = torch.autograd.grad(out64, (w64, b64), dp.double())
    xd, wd, bd = x.to(DEV), w.to(DEV).contiguous(), b.to(DEV)
    p1 = torch.zeros((B, 14, 14, 64), device=DEV)
    idx = torch.empty((B, 14, 14, 32), dtype=torch.uint8, device=DEV)
    cabi.check(lib.ld_mc_conv1(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), p1.data_ptr(), idx.data_ptr(), B, st()), "mc_conv1")
    assert rel_err(p1[..., :32].permute(0, 3, 1, 2).cpu().double(), out64.detach()) <= TOL
    assert float(p1[..., 32:].abs().max()) == 0.0 and int(idx.max()) <= 3
    # a window of the background: four equal values, position 0
    assert int(idx[0, 1, 5].max()) == 0
    work = torch.empty(int(lib.ld_mc_conv1_wgrad_work_floats(B)), device=DEV)
    gw, gb = torch.empty(32 * 9, device=DEV), torch.empty(32, device=DEV)
    dpd = nhwc_pad(dp, 64)
    cabi.check(lib.ld_mc_conv1_wgrad(xd.data_ptr(), p1.data_ptr(), dpd.data_ptr(), idx.data_ptr(), work.data_ptr(), gw.data_ptr(),
                                     gb.data_ptr(), B, st()), "mc_conv1_wgrad")
    e_w, e_b = rel_err(gw.cpu().double().view_as(gw64), gw64), rel_err(gb.cpu().double(), gb64)
    print(f"conv1 B={B}: dW {e_w:.2e} db {e_b:.2e}")
    assert e_w <= TOL and e_b <= TOL


@pytest.mark.parametrize("B,H,C_", [(2, 7, 64), (1, 3, 8)])
def test_pool_and_its_backward_route_to_the_first_maximum_exactly(B, H, C_):
    lib = cabi.lib()
    pre = rnd((B, C_, 2 * H, 2 * H), 5)
    pre[0, :, 0:2, 0:2] = 0.75                                 # four equal positive values -> position 0
    pre[0, :, 0, 2], pre[0, :, 1, 3], pre[0, :, 0, 3], pre[0, :, 1, 2] = -1.0, 0.9, 0.9, 0.1    # (0, 1) and (1, 1) tie -> 1
    pre[0, :, 2:4, 0:2] = -0.5                                 # all below zero: ReLU's gradient is 0 everywhere
    pre[0, :, 2, 2], pre[0, :, 2, 3], pre[0, :, 3, 2], pre[0, :, 3, 3] = 0.2, 0.1, 0.2, 0.2     # (0, 0) wins over the later 0.2s
    pre64 = pre.double().requires_grad_(True)
    out64 = F.max_pool2d(F.relu(pre64), 2)
    dp = rnd((B, C_, H, H), 6)
    (g64,) = torch.autograd.grad(out64, pre64, dp.double())
    a = nhwc_pad(F.relu(pre), C_)
    out = torch.empty((B, H, H, C_), device=DEV)
    idx = torch.empty((B, H, H, C_), dtype=torch.uint8, device=DEV)
    cabi.check(lib.ld_mc_pool(a.data_ptr(), out.data_ptr(), idx.data_ptr(), B, H, H, C_, st()), "mc_pool")
    assert torch.equal(out.permute(0, 3, 1, 2).cpu(), out64.detach().float())
    assert idx[0, 0, 0].tolist() == [0] * C_ and idx[0, 0, 1].tolist() == [1] * C_ and idx[0, 1, 1].tolist() == [0] * C_
    dx = torch.full((B, 2 * H, 2 * H, C_), 7.0, device=DEV)
    cabi.check(lib.ld_mc_pool_backward(nhwc_pad(dp, C_).data_ptr(), out.data_ptr(), idx.data_ptr(), dx.data_ptr(), B, H, H, C_,
                                       st()), "mc_pool_backward")
    got = dx.permute(0, 3, 1, 2).cpu()
    assert torch.equal(got, g64.float())                       # routing only: exact
    assert float(got[0, :, 2:4, 0:2].abs().max()) == 0.0 and torch.equal(got[0, :, 0, 0], dp[0, :, 0, 0])


@pytest.mark.parametrize("M,N,K,splits", [(64, 128, 3136, 49), (3, 128, 3136, 49), (5, 70, 45, 2), (130, 64, 33, 1)])
def test_gemm_in_the_three_operand_layouts(M, N, K, splits):
    """fc1's forward (both operands K-contiguous, split over K), its weight gradient (both K-strided) and its data gradient
    (mixed) against fp64."""
    lib = cabi.lib()
    a, b = rnd((M, K), 7), rnd((N, K), 8)
    ref = a.double() @ b.double().t()
    bound = TOL * float(ref.abs().max())

    def run(ad, am, ak, bd, bn, bk, s):
        out = torch.full((s, M, N), 9.0, device=DEV)
        cabi.check(lib.ld_mc_gemm(ad.data_ptr(), bd.data_ptr(), out.data_ptr(), M, N, K, am, ak, bn, bk, N, s, st()), "mc_gemm")
        return out
    out = run(a.to(DEV), K, 1, b.to(DEV), K, 1, splits)
    assert float((out.cpu().double().sum(0) - ref).abs().max()) <= bound
    if splits > 1:                                             # the finish pass adds the slabs in order, + bias, ReLU
        bias = rnd((N,), 9).to(DEV)
        h = torch.empty((M, N), device=DEV)
        cabi.check(lib.ld_mc_fc1_finish(out.data_ptr(), bias.data_ptr(), h.data_ptr(), M, N, splits, st()), "mc_fc1_finish")
        s = out[0].clone()
        for k in range(1, splits):
            s += out[k]
        assert torch.equal(h, torch.relu(s + bias))
    at, bt = a.t().contiguous().to(DEV), b.t().contiguous().to(DEV)
    assert float((run(at, 1, M, bt, 1, N, 1)[0].cpu().double() - ref).abs().max()) <= bound
    assert float((run(a.to(DEV), K, 1, bt, 1, N, 1)[0].cpu().double() - ref).abs().max()) <= bound


@pytest.mark.parametrize("B", [1, 5, 64])
def test_head_loss_and_small_gradients(B):
    lib = cabi.lib()
    pre = rnd((B, 128), 10)
    pre[:, ::7] = 0.0                                          # exact zeros behind the ReLU: gradient 0 there
    w2, b2 = rnd((10, 128), 11) / 4.0, rnd((10,), 12)
    label = torch.from_numpy(rng.uniform((B,), 2020, 13, 0.0, 10.0)).long().clamp(0, 9)
    pre64, w64, b64 = pre.double().requires_grad_(True), w2.double().requires_grad_(True), b2.double().requires_grad_(True)
    z64 = F.linear(F.relu(pre64), w64, b64)
    loss64 = F.cross_entropy(z64, label)
    gpre, gw, gb = torch.autograd.grad(loss64, (pre64, w64, b64))
    h = F.relu(pre).to(DEV)
    f32 = dict(device=DEV)
    logits, pred = torch.empty((B, 10), **f32), torch.empty(B, dtype=torch.int64, device=DEV)
    loss_b, dz, dh = torch.empty(B, **f32), torch.empty((B, 10), **f32), torch.empty((B, 128), **f32)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    w2d, b2d, lab = w2.to(DEV), b2.to(DEV), label.to(DEV)
    cabi.check(lib.ld_mc_head(h.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), lab.data_ptr(), logits.data_ptr(), pred.data_ptr(),
                              loss_b.data_ptr(), dz.data_ptr(), dh.data_ptr(), flag.data_ptr(), B, st()), "mc_head")
    assert rel_err(logits.cpu().double(), z64.detach()) <= TOL and torch.equal(pred, logits.argmax(1)) and int(flag) == 0
    assert rel_err(dh.cpu().double(), gpre) <= TOL
    assert float(dh.cpu()[:, ::7].abs().max()) == 0.0
    gw2, gb2, gb1, loss = torch.empty((10, 128), **f32), torch.empty(10, **f32), torch.empty(128, **f32), torch.empty(1, **f32)
    cabi.check(lib.ld_mc_small_grads(dz.data_ptr(), h.data_ptr(), dh.data_ptr(), loss_b.data_ptr(), gw2.data_ptr(), gb2.data_ptr(),
                                     gb1.data_ptr(), loss.data_ptr(), B, st()), "mc_small_grads")
    assert abs(float(loss) - float(loss64.detach())) <= TOL * abs(float(loss64.detach()))
    assert rel_err(gw2.cpu().double(), gw) <= TOL and rel_err(gb2.cpu().double(), gb) <= TOL
    assert rel_err(gb1.cpu().double(), gpre.sum(0)) <= TOL
    # inference form: no labels, same logits
    logits2 = torch.empty((B, 10), **f32)
    cabi.check(lib.ld_mc_head(h.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), None, logits2.data_ptr(), None, None, None, None,
                              None, B, st()), "mc_head")
    assert torch.equal(logits, logits2)


def test_a_label_outside_0_to_9_indexes_nothing_and_is_reported():
    g, _, sd, x, y = g20()
    net = g20_net(sd)
    tr = ldh.MnistClassifierTrainer(net)
    with pytest.raises(ValueError, match="outside 0..9"):      # host labels: refused before anything is launched
        tr.step(x[:4].to(DEV), torch.tensor([1, 2, 10, 3]))
    bad = y[:8].clone()
    bad[3] = 10
    loss, grads = tr.loss_and_grads(x[:8].to(DEV), bad.to(DEV))
    assert torch.isnan(loss) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    with pytest.raises(ValueError, match="outside 0..9"):
        tr.check_labels()
    tr.check_labels()                                          # the flag was cleared
    loss, _ = tr.loss_and_grads(x[:8].to(DEV), y[:8].to(DEV))
    assert bool(torch.isfinite(loss))


# ------------------------------------------------------------------------------------------------ whole net
def test_whole_net_gradients_on_the_three_golden_batches():
    """Loss and all eight gradients at the initial weights.  The biases and fc2 element by element against G20 (2e-5 of the
    tensor's largest value); every parameter within 4 x grad_spread in relative L2 (the full fp64 gradient of fc1.weight,
    which G20 holds only in summary, comes from the restatement run here, which tests/test_mnistcls.py ties to G20).
    The spreads and what has been measured: docs/findings.md 120."""
    g, gg, sd, x, y = g20()
    net = g20_net(sd)
    tr = ldh.MnistClassifierTrainer(net)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    loose = 4.0 * float(g["grad_spread"])
    for b in range(3):
        xb, yb = x[64 * b:64 * b + 64], y[64 * b:64 * b + 64]
        loss64, grads64 = mnistcls_ref.loss_and_grads(mnistcls_ref.params_of(sd, torch.float64), xb, yb)
        loss, grads = tr.loss_and_grads(xb.to(DEV), yb.to(DEV))
        assert list(grads.keys()) == list(grads64.keys())
        e_loss = abs(float(loss) - float(g["loss_init"][b]))
        rel = {k: mnistcls_ref.rel_l2(grads[k].cpu(), grads64[k]) for k in grads}
        small = {k: rel_err(grads[k].cpu().double(), torch.from_numpy(gg[f"grad{b}.{k}"])) for k in SMALL}
        print(f"batch {b}: loss error {e_loss:.2e}; relative L2 " + ", ".join(f"{k} {v:.2e}" for k, v in rel.items())
              + f" (bound {loose:.2e}); element-wise " + ", ".join(f"{k} {v:.2e}" for k, v in small.items()))
        for k in grads:
            assert grads[k].shape == grads64[k].shape, k
        assert e_loss <= 4.0 * float(g["loss_spread"]), (b, e_loss)
        assert max(small.values()) <= TOL, (b, small)
        assert max(rel.values()) <= loose, (b, max(rel, key=rel.get), max(rel.values()), loose)
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_adam_step_is_torch_optim_adam_within_two_ulps():
    """One step from the HIP gradients: every parameter within allclose(rtol=2.4e-7, atol=1e-8) -- two ulps of the parameter
    plus 1e-5 of lr, the rule of test_hip_segtrain.py -- of torch.optim.Adam given the same fp32 gradients; and the
    kernel-layout copies that the optimiser's launch keeps are the repacked parameters, bit for bit."""
    g, _, sd, x, y = g20()
    net = g20_net(sd)
    tr = ldh.MnistClassifierTrainer(net)
    xb, yb = x[:64].to(DEV), y[:64].to(DEV)
    _, grads = tr.loss_and_grads(xb, yb)
    theirs1 = [torch.from_numpy(np.asarray(v)).clone().requires_grad_(True) for v in sd.values()]
    opt1 = torch.optim.Adam(theirs1, lr=0.001)
    for p, k in zip(theirs1, sd):
        p.grad = grads[k].cpu().clone()
    opt1.step()
    tr.step(xb, yb)                                            # the same gradients: the kernels are deterministic
    mirrors = {k: v.clone() for k, v in (("w2f", net._packed.w2f), ("w2b", net._packed.w2b), ("wfc1", net._packed.wfc1))}
    for (k, mine), th in zip(net.state_dict().items(), theirs1):
        assert torch.allclose(mine.cpu(), th.detach(), rtol=2.4e-7, atol=1e-8), (k, float((mine.cpu() - th.detach()).abs().max()))
        assert not torch.equal(mine.cpu(), torch.from_numpy(np.asarray(sd[k]))), k
    net._packed.pack()                                         # repack from the parameters: must change nothing
    assert torch.equal(mirrors["w2f"], net._packed.w2f) and torch.equal(mirrors["w2b"], net._packed.w2b)
    assert torch.equal(mirrors["wfc1"], net._packed.wfc1)
    w = net.fc1.weight.view(128, 64, 49).permute(0, 2, 1).reshape(-1)
    assert torch.equal(net._packed.wfc1, w)


def test_48_steps_follow_the_fp64_trajectory():
    """Three epochs over the 1,024 training digits in file order at B = 64.  The 48 losses within 4 x loss_spread of G20's
    fp64 losses, all finite, the last below half the first.  After step 48 the argmax of the test logits equals the fp64
    reference's on every held-out digit whose fp64 top-two gap exceeds 100 x logit_spread; at most 2 % of the 512 are left
    out by that rule.  The spreads and what has been measured: docs/findings.md 120."""
    g, _, sd, x, y = g20()
    net = g20_net(sd)
    tr = ldh.MnistClassifierTrainer(net)
    batches = mnistcls_ref.epoch_batches(x[:1024], y[:1024], 3)
    losses = torch.stack([tr.step(xb.to(DEV), yb.to(DEV)) for xb, yb in batches]).cpu().double().numpy()
    tr.check_labels()
    errs = np.abs(losses - g["loss_steps"])
    bound = 4.0 * float(g["loss_spread"])
    print(f"losses {losses[0]:.5f} -> {losses[-1]:.5f}; distance to the fp64 losses: max {errs.max():.3e} at step "
          f"{int(errs.argmax()) + 1}, step 1 {errs[0]:.3e}, step 48 {errs[-1]:.3e} (loss_spread {float(g['loss_spread']):.3e}, "
          f"bound {bound:.3e})")
    assert tr.t == 48 and np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0]
    assert errs.max() <= bound, (errs.max(), bound)
    z64 = torch.from_numpy(g["test_logits"])
    pred, z = net.predict(x[1024:].to(DEV))
    top2 = z64.topk(2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]) > 100.0 * float(g["logit_spread"])
    left_out = int((~decided).sum())
    e = float((z.cpu().double() - z64).abs().max())
    acc = float((pred.cpu() == y[1024:]).double().mean())
    print(f"test logits after step 48: HIP to fp64 {e:.3e} (logit_spread {float(g['logit_spread']):.3e}); accuracy "
          f"{100 * acc:.1f} % (fp64 {100 * float(g['accuracy']):.1f} %); {left_out} digits left out")
    assert left_out <= 0.02 * 512
    assert torch.equal(pred.cpu()[decided], z64.argmax(1)[decided])


def test_two_runs_from_the_same_state_are_bit_identical():
    g, _, sd, x, y = g20()
    runs = []
    for _ in range(2):
        net = g20_net(sd)
        tr = ldh.MnistClassifierTrainer(net)
        losses = [tr.step(x[64 * b:64 * b + 64].to(DEV), y[64 * b:64 * b + 64].to(DEV)) for b in range(8)]
        runs.append((torch.stack(losses), {k: v.clone() for k, v in net.state_dict().items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
        assert not torch.equal(runs[0][1][k].cpu(), torch.from_numpy(np.asarray(sd[k]))), k


def test_eight_steps_enqueue_without_the_host_waiting():
    """The stream is kept busy by a long queue of matrix products; eight steps are enqueued behind it.  If anything inside a
    step waited for the device, the host would come back only after the products had finished; here the event recorded
    behind them has not yet completed when the host returns from the eighth step."""
    g, _, sd, x, y = g20()
    net = g20_net(sd)
    tr = ldh.MnistClassifierTrainer(net)
    xb, yb = x[:64].to(DEV), y[:64].to(DEV)
    for _ in range(2):                                         # buffers, moments and the allocator's pools exist
        tr.step(xb, yb)
    a = torch.randn(8192, 8192, device=DEV)
    c = torch.empty_like(a)
    torch.mm(a, a, out=c)
    torch.cuda.synchronize()
    busy = torch.cuda.Event()
    for _ in range(60):
        torch.mm(a, a, out=c)
    busy.record()
    losses = [tr.step(xb, yb) for _ in range(8)]
    still_running = not busy.query()
    torch.cuda.synchronize()
    assert still_running, "a step waited for the device"
    assert all(v.is_cuda and v.dim() == 0 for v in losses) and bool(torch.isfinite(torch.stack(losses)).all())


# ------------------------------------------------------------------------------------------------ around it
def test_digit_report_counts_every_image():
    g, _, sd, x, y = g20()
    net = g20_net(sd)
    rep = evalio.digit_report(net, x[:300], y[:300].numpy(), batch_size=128)
    assert rep["confusion"].shape == (10, 10) and int(rep["confusion"].sum()) == 300
    assert rep["pred"].shape == (300,) and rep["pred"].dtype == np.int64
    assert abs(rep["accuracy"] - float(np.trace(rep["confusion"])) / 300.0) < 1e-12
    assert np.array_equal(rep["confusion"].sum(1), np.bincount(y[:300].numpy(), minlength=10))
    assert np.array_equal(rep["pred"], net.predict(x[:300].to(DEV))[0].cpu().numpy())


def test_fit_writes_a_loadable_checkpoint_and_a_csv(tmp_path):
    import csv
    g, _, sd, x, y = g20()
    net = g20_net(sd)
    tr = ldh.MnistClassifierTrainer(net)
    train = [(x[i:i + 64].to(DEV), y[i:i + 64].to(DEV)) for i in range(0, 512, 64)]
    test = [(x[i:i + 128].to(DEV), y[i:i + 128].to(DEV)) for i in range(1024, 1536, 128)]
    out_path, csv_path = str(tmp_path / "best.pth"), str(tmp_path / "loss.csv")
    res = tr.fit(train, test, 2, out_path, csv_path)
    rows = list(csv.reader(open(csv_path)))
    assert rows[0] == ["epoch", "train_loss", "accuracy"] and len(rows) == 3 and tr.t == 16
    counts = [tr.evaluate(xb, yb) for xb, yb in test]
    assert all(c.is_cuda for c, _ in counts)
    acc = 100 * sum(int(c) for c, _ in counts) / sum(n for _, n in counts)
    assert float(rows[2][2]) == acc and res["rows"][1][2] == acc
    assert res["best_acc"] == max(r[2] for r in res["rows"]) and res["best_acc"] > 30.0
    assert float(rows[2][1]) < float(rows[1][1])               # the running mean over all 16 steps fell
    loaded = ldh.MnistClassifier()
    assert checkpoint.load_mnist_classifier(out_path, loaded)["n_tensors"] == 8
    if res["best_epoch"] == 1:                                 # the file is the final state
        for k, v in net.state_dict().items():
            assert torch.equal(v.cpu(), loaded.state_dict()[k]), k
    z = loaded.to(DEV)(x[1024:1088].to(DEV))
    assert z.shape == (64, 10) and bool(torch.isfinite(z).all())
