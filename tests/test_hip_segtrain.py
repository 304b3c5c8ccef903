"""Training the segmentation U-Net on the GPU: every new kernel against the fp32 torch op (element-wise outputs) or the
same quantity in fp64 (long reductions) at every level's shape of a 256^2 net, the whole net's loss / statistics /
gradients at the initial weights against tests/segtrain_ref.py in fp64 on G19's six batches, six Adam steps, and the
module-level behaviour (train-mode forward, determinism, the saved file, tools/train_seg.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import localdiffusion_hallucination_amd as ldh                              # noqa: E402
from localdiffusion_hallucination_amd import _cabi as cabi                  # noqa: E402
from localdiffusion_hallucination_amd import checkpoint, rng, segtrain, weights   # noqa: E402

from hip_helpers import DEV, RTOL, rel_err, st                              # noqa: E402
import segtrain_ref                                                          # noqa: E402
from test_hip_segnet import LEVELS, UPS                                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = RTOL["fp32"]


def rnd(shape, key, lo=-1.0, hi=1.0):
    return torch.from_numpy(rng.uniform(shape, 1919, key, lo, hi))


def to_nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


def to_nchw(x):
    return x.permute(0, 3, 1, 2).contiguous().cpu()


def red_work():
    return torch.empty(segtrain.RED_WORK_BYTES // 8, dtype=torch.float64, device=DEV)


def reduction_bound(got, ref64, torch32, what):
    """Long reductions: rel_err to the fp64 value at most max(1e-5, 4 d), d = the fp32 torch op's own rel_err to it."""
    d = rel_err(torch32.double(), ref64)
    e = rel_err(got.double(), ref64)
    print(f"{what}: HIP rel err {e:.2e}, fp32 torch {d:.2e}, bound {max(1e-5, 4 * d):.2e}")
    assert e <= max(1e-5, 4 * d), (what, e, d)
    return e, d


def pc_conv(src, weight, cin, cout, B, h, ksize, shift=None):
    out = torch.empty((B, h, h, cout), device=DEV)
    ones, zeros = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
    a = cabi.PcConvArgs()
    a.src, a.weight, a.scale, a.shift, a.out = src.data_ptr(), weight.data_ptr(), ones.data_ptr(), \
        (zeros if shift is None else shift).data_ptr(), out.data_ptr()
    a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout, a.ksize, a.stride, a.relu = B, h, h, cin, h, h, cout, ksize, 1, 0
    cabi.check(cabi.lib().ld_pc_conv(C.byref(a), st()), "pc_conv")
    return out


def hip_wgrad(dy, a, B, h, cin, cout, ksize):
    lib = cabi.lib()
    splits = lib.ld_seg_wgrad_splits(B, h, h, cin, cout, ksize)
    assert splits >= 1
    n = cout * ksize * ksize * cin
    work, dw = torch.empty(splits * n, device=DEV), torch.empty(n, device=DEV)
    cabi.check(lib.ld_seg_wgrad(dy.data_ptr(), a.data_ptr(), work.data_ptr(), dw.data_ptr(), B, h, h, cin, cout, ksize, splits,
                                st()), "seg_wgrad")
    return dw, splits


def permute3(w, out_numel, dims, off, strides):
    w = w.to(DEV).contiguous()
    out = torch.zeros(out_numel, device=DEV)
    cabi.check(cabi.lib().ld_seg_permute3(w.data_ptr(), out.data_ptr(), *dims, off, *strides, st()), "seg_permute3")
    return out


# every 3x3 convolution shape of a 256^2 net: (H, Cin, Cout) of LEVELS (first convolution of inc / each Down), the second
# convolution of each DoubleConv, and the first convolution of each Up (Cin = the concatenation)
CONVS = sorted(set(LEVELS) | {(h, co, co) for h, _, co in LEVELS} | {(h, ci, ci // 2) for h, ci in UPS})


@pytest.mark.parametrize("H,cin,cout", CONVS)
def test_weight_gradient_per_level(H, cin, cout):
    """Bound max(1e-5, 4 d), d = torch's fp32 op against fp64 on the same inputs.  Measured on an MI355X over the 13 shapes:
    HIP 2.5e-7 .. 7.6e-7, fp32 torch 6.4e-7 .. 1.7e-6 (1 .. 228 splits)."""
    B = 2 if H <= 64 else 1
    x = F.relu(rnd((B, cin, H, H), 3 * H + cin))                   # a post-ReLU activation, as in the net
    dy = rnd((B, cout, H, H), 3 * H + cin + 1) / (B * H * H)
    ref64 = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 3, 3), dy.double(), padding=1)
    t32 = torch.nn.grad.conv2d_weight(x, (cout, cin, 3, 3), dy, padding=1)
    dw, splits = hip_wgrad(to_nhwc(dy), to_nhwc(x), B, H, cin, cout, 3)
    got = dw.view(cout, 3, 3, cin).permute(0, 3, 1, 2).cpu()
    reduction_bound(got, ref64, t32, f"wgrad 3x3 {H}^2 B={B} {cin}->{cout} ({splits} splits)")


@pytest.mark.parametrize("H,cin,cout", CONVS)
def test_data_gradient_per_level(H, cin, cout):
    """ld_pc_conv on the flipped, transposed weight (ld_seg_permute3) against torch's conv2d input gradient (fp32).
    Bound 2e-5; measured on an MI355X: 1.1e-6 .. 4.3e-6."""
    B = 2 if H <= 64 else 1
    w = rnd((cout, cin, 3, 3), 5 * H + cin) / np.sqrt(cin * 9)
    dy = rnd((B, cout, H, H), 5 * H + cin + 1)
    ref = torch.nn.grad.conv2d_input((B, cin, H, H), w, dy, padding=1)
    wb = permute3(w, cin * 9 * cout, (cout, cin, 9), 8 * cout, (1, 9 * cout, -cout))
    assert torch.equal(wb.view(cin, 3, 3, cout).cpu(), w.flip(2, 3).permute(1, 2, 3, 0))
    got = to_nchw(pc_conv(to_nhwc(dy), wb, cout, cin, B, H, 3))
    e = rel_err(got, ref)
    print(f"dgrad 3x3 {H}^2 {cout}->{cin}: rel err {e:.2e}")
    assert e <= TOL, e


@pytest.mark.parametrize("H,cin", UPS)
def test_conv_transpose_gradients(H, cin):
    """ConvTranspose2d(2, 2) as a 1x1 GEMM to (p1, p2, c) channels: forward with the training-layout weight, weight / bias /
    data gradients from the gradient of the GEMM output.  Measured on an MI355X: weight gradient 2.2e-7 .. 5.4e-7 (fp32 torch
    6.7e-7 .. 1.4e-6), bias gradient 2.6e-8 .. 4.0e-8 (torch 1.6e-6 .. 7.9e-6), data gradient 6.9e-7 .. 1.7e-6 (bound 2e-5)."""
    B, cout, h = (2 if H <= 64 else 1), cin // 2, H // 2
    x = F.relu(rnd((B, cin, h, h), 7 * H)).requires_grad_(True)
    w = (rnd((cin, cout, 2, 2), 7 * H + 1) / np.sqrt(cin)).requires_grad_(True)
    b = (rnd((cout,), 7 * H + 2) / np.sqrt(cin)).requires_grad_(True)
    dup = rnd((B, cout, H, H), 7 * H + 3) / (B * H * H)
    up = F.conv_transpose2d(x, w, b, stride=2)
    gx, gw, gb = torch.autograd.grad(up, (x, w, b), dup)
    x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (x, w, b))
    _, gw64, gb64 = torch.autograd.grad(F.conv_transpose2d(x64, w64, b64, stride=2), (x64, w64, b64), dup.double())
    wf = permute3(w.detach(), 4 * cout * cin, (cin, cout, 4), 0, (1, cin, cout * cin))
    wbk = permute3(w.detach(), 4 * cout * cin, (cin, cout, 4), 0, (4 * cout, 1, cout))
    bias4 = b.detach().repeat(4).to(DEV)
    xd = to_nhwc(x.detach())
    low = pc_conv(xd, wf, cin, 4 * cout, B, h, 1, shift=bias4)
    up_img = low.reshape(B, h, h, 2, 2, cout).permute(0, 5, 1, 3, 2, 4).reshape(B, cout, H, H).cpu()
    assert rel_err(up_img, up.detach()) <= TOL
    dlow = dup.reshape(B, cout, h, 2, h, 2).permute(0, 2, 4, 3, 5, 1).reshape(B, h, h, 4 * cout).contiguous().to(DEV)
    dw, splits = hip_wgrad(dlow, xd, B, h, cin, 4 * cout, 1)
    reduction_bound(dw.view(2, 2, cout, cin).permute(3, 2, 0, 1).cpu(), gw64, gw, f"convT wgrad {H}^2 {cin} ({splits} splits)")
    gbh, work = torch.empty(cout, device=DEV), red_work()
    cabi.check(cabi.lib().ld_seg_colsum(dlow.data_ptr(), work.data_ptr(), gbh.data_ptr(), B * h * h, 4 * cout, 4, st()),
               "seg_colsum")
    reduction_bound(gbh.cpu(), gb64, gb, f"convT bias grad {H}^2")
    e = rel_err(to_nchw(pc_conv(dlow, wbk, 4 * cout, cin, B, h, 1)), gx)
    print(f"convT dgrad {H}^2: rel err {e:.2e}")
    assert e <= TOL, e


def hip_bn_train(y, gamma, beta, rm=None, rv=None):
    M, Cc = y.numel() // y.shape[-1], y.shape[-1]
    stat, out, work = torch.empty(3 * Cc, device=DEV), torch.empty_like(y), red_work()
    cabi.check(cabi.lib().ld_seg_bn_train(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), work.data_ptr(), stat.data_ptr(),
                                          cabi.ptr(rm), cabi.ptr(rv), 0.1, 1e-5, out.data_ptr(), M, Cc, st()), "seg_bn_train")
    return stat.view(3, Cc), out


@pytest.mark.parametrize("H,C_", [(h, co) for h, _, co in LEVELS])
def test_batchnorm_train_forward_and_backward_per_level(H, C_):
    """Measured on an MI355X: mean / variance / dbeta / dgamma 2.4e-8 .. 9.0e-8 against fp64 (fp32 torch 3.5e-8 .. 1.1e-6,
    bound max(1e-5, 4 d)); activation 1.8e-7 .. 2.4e-7 and dY 2.8e-7 against torch's fp32 ops (bound 2e-5)."""
    B = 2 if H <= 64 else 1
    y = (0.3 + 1.5 * rnd((B, C_, H, H), 11 * H)).requires_grad_(True)
    gamma = (1.0 + 0.1 * rnd((C_,), 11 * H + 1)).requires_grad_(True)
    beta = (0.1 * rnd((C_,), 11 * H + 2)).requires_grad_(True)
    rm, rv = 0.2 * rnd((C_,), 11 * H + 3), 0.5 + rnd((C_,), 11 * H + 4, 0.0, 1.0)
    rm_t, rv_t = rm.clone(), rv.clone()
    act = F.relu(F.batch_norm(y, rm_t, rv_t, gamma, beta, training=True, momentum=0.1, eps=1e-5))
    rm_d, rv_d = rm.to(DEV), rv.to(DEV)
    yd, gd, bd = to_nhwc(y.detach()), gamma.detach().to(DEV), beta.detach().to(DEV)
    stat, out = hip_bn_train(yd, gd, bd, rm_d, rv_d)
    e_act = rel_err(to_nchw(out), act.detach())
    assert e_act <= TOL, e_act
    y64 = y.detach().double()
    mean64, var64 = y64.mean(dim=(0, 2, 3)), y64.var(dim=(0, 2, 3), unbiased=False)
    y32 = y.detach()
    reduction_bound(stat[0].cpu(), mean64, y32.mean(dim=(0, 2, 3)), f"BN mean {H}^2 C={C_}")
    reduction_bound(stat[1].cpu(), var64, y32.var(dim=(0, 2, 3), unbiased=False), f"BN var {H}^2 C={C_}")
    assert rel_err(rm_d.cpu(), rm_t) <= TOL and rel_err(rv_d.cpu(), rv_t) <= TOL
    # without running pointers nothing else is touched
    stat2, out2 = hip_bn_train(yd, gd, bd)
    assert torch.equal(stat2, stat) and torch.equal(out2, out)
    # backward: both sides take the ReLU mask from the same saved activation (torch's)
    da = rnd((B, C_, H, H), 11 * H + 5) / (B * H * H)
    gy, gg, gb = torch.autograd.grad(act, (y, gamma, beta), da)
    mask = (act.detach() > 0)
    g64 = da.double() * mask
    xh64 = (y64 - mean64.view(1, -1, 1, 1)) / torch.sqrt(var64.view(1, -1, 1, 1) + 1e-5)
    dgamma, dbeta, dy = torch.empty(C_, device=DEV), torch.empty(C_, device=DEV), torch.empty_like(yd)
    dad, actd, work = to_nhwc(da), to_nhwc(act.detach()), red_work()     # (held: a temporary's memory is reused at once)
    cabi.check(cabi.lib().ld_seg_bn_backward(dad.data_ptr(), actd.data_ptr(), yd.data_ptr(), gd.data_ptr(),
                                             stat.data_ptr(), work.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                             dy.data_ptr(), B * H * H, C_, st()), "seg_bn_backward")
    reduction_bound(dbeta.cpu(), g64.sum(dim=(0, 2, 3)), gb, f"BN dbeta {H}^2 C={C_}")
    reduction_bound(dgamma.cpu(), (g64 * xh64).sum(dim=(0, 2, 3)), gg, f"BN dgamma {H}^2 C={C_}")
    e_dy = rel_err(to_nchw(dy), gy)
    print(f"BN {H}^2 C={C_}: act rel err {e_act:.2e}, dY rel err {e_dy:.2e}")
    assert e_dy <= TOL, e_dy
    # in place (dy = da), as the trainer calls it
    cabi.check(cabi.lib().ld_seg_bn_backward(dad.data_ptr(), actd.data_ptr(), yd.data_ptr(), gd.data_ptr(),
                                             stat.data_ptr(), work.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                             dad.data_ptr(), B * H * H, C_, st()), "seg_bn_backward")
    assert torch.equal(dad, dy)


@pytest.mark.parametrize("H,C_", [(h // 2, co) for h, _, co in LEVELS[:4]])
def test_max_pool_and_its_backward_with_the_skip_gradient(H, C_):
    """Post-ReLU input: about one window in sixteen is all zeros (the tie rule: first maximum in row-major order), the rest
    hold distinct values.  Exact in fp32 on both sides, so the comparison is bitwise."""
    B = 2 if H <= 32 else 1
    x = F.relu(rnd((B, C_, 2 * H, 2 * H), 13 * H)).requires_grad_(True)
    win = x.detach().reshape(B, C_, H, 2, H, 2)
    assert int((win.amax(dim=(3, 5)) == 0).sum()) > 0
    pooled = F.max_pool2d(x, 2)
    dp, dskip = rnd((B, C_, H, H), 13 * H + 1), rnd((B, C_, 2 * H, 2 * H), 13 * H + 2)
    (gx,) = torch.autograd.grad(pooled, x, dp)
    lib = cabi.lib()
    xd, out = to_nhwc(x.detach()), torch.empty((B, H, H, C_), device=DEV)
    cabi.check(lib.ld_seg_pool(xd.data_ptr(), out.data_ptr(), B, H, H, C_, st()), "seg_pool")
    assert torch.equal(to_nchw(out), pooled.detach())
    dx, dpd, dskipd = torch.empty_like(xd), to_nhwc(dp), to_nhwc(dskip)
    cabi.check(lib.ld_seg_pool_backward(xd.data_ptr(), dpd.data_ptr(), None, dx.data_ptr(), B, H, H, C_, st()),
               "seg_pool_backward")
    assert torch.equal(to_nchw(dx), gx)
    cabi.check(lib.ld_seg_pool_backward(xd.data_ptr(), dpd.data_ptr(), dskipd.data_ptr(), dx.data_ptr(), B, H, H,
                                        C_, st()), "seg_pool_backward")
    assert torch.equal(to_nchw(dx), dskip + gx)


@pytest.mark.parametrize("H,cin", UPS)
def test_concat_with_depth_to_space_and_its_split(H, cin):
    B, c, h = 1, cin // 2, H // 2
    skip, low = rnd((B, H, H, c), 17 * H).to(DEV), rnd((B, h, h, 4 * c), 17 * H + 1).to(DEV)
    cat = torch.empty((B, H, H, 2 * c), device=DEV)
    lib = cabi.lib()
    cabi.check(lib.ld_seg_cat_d2s(skip.data_ptr(), low.data_ptr(), cat.data_ptr(), B, H, H, c, c, st()), "seg_cat_d2s")
    up = low.reshape(B, h, h, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(B, H, H, c)
    assert torch.equal(cat, torch.cat([skip, up], dim=3))           # the skip first (unet_model.py:201)
    dskip, dlow = torch.empty_like(skip), torch.empty_like(low)
    cabi.check(lib.ld_seg_cat_d2s_backward(cat.data_ptr(), dskip.data_ptr(), dlow.data_ptr(), B, H, H, c, c, st()),
               "seg_cat_d2s_backward")
    assert torch.equal(dskip, skip) and torch.equal(dlow, low)


@pytest.mark.parametrize("B,H", [(2, 256), (4, 32)])
def test_loss_and_head_backward(B, H):
    """Measured on an MI355X: loss terms 9e-9 / 3e-8 against fp64 (fp32 torch the same), dz 2.0e-7 / 9.8e-8 (bound 2e-5),
    head dW 4.2e-8 / 3.6e-8 and db 1.9e-8 / 2.9e-8 (fp32 torch 1.7e-7 .. 1.5e-6)."""
    M = B * H * H
    z = (3.0 * rnd((B, 1, H, H), 19 * H)).requires_grad_(True)
    t = (rnd((B, 1, H, H), 19 * H + 1, 0.0, 1.0) < 0.03).float()
    bce, dice = segtrain_ref.loss_terms(z, t)
    (gz,) = torch.autograd.grad(bce + dice, z)
    bce64, dice64 = segtrain_ref.loss_terms(z.detach().double(), t.double())
    out, dz = torch.empty(3, device=DEV), torch.empty(M, device=DEV)
    zd, td, work = z.detach().to(DEV), t.to(DEV), red_work()
    lib = cabi.lib()
    cabi.check(lib.ld_seg_loss(zd.data_ptr(), td.data_ptr(), work.data_ptr(), out.data_ptr(), dz.data_ptr(), M, 10.0, 1e-5,
                               st()), "seg_loss")
    ref64 = torch.stack([bce64 + dice64, bce64, dice64])
    reduction_bound(out.cpu(), ref64, torch.stack([bce + dice, bce, dice]).detach(), f"loss terms B={B} {H}^2")
    e = rel_err(dz.cpu().view_as(gz), gz)
    print(f"dz B={B} {H}^2: rel err {e:.2e}")
    assert e <= TOL, e
    out2 = torch.empty(3, device=DEV)                              # evaluation: no dz
    cabi.check(lib.ld_seg_loss(zd.data_ptr(), td.data_ptr(), work.data_ptr(), out2.data_ptr(), None, M, 10.0, 1e-5, st()),
               "seg_loss")
    assert torch.equal(out, out2)
    # the head: dW, db (long reductions), dX (element-wise)
    x = F.relu(rnd((B, 64, H, H), 19 * H + 2)).requires_grad_(True)
    w, b = (rnd((1, 64, 1, 1), 19 * H + 3) / 8.0).requires_grad_(True), torch.tensor([-0.4], requires_grad=True)
    gx, gw, gb = torch.autograd.grad(F.conv2d(x, w, b), (x, w, b), gz)
    x64, w64, b64 = (v.detach().double().requires_grad_(True) for v in (x, w, b))
    _, gw64, gb64 = torch.autograd.grad(F.conv2d(x64, w64, b64), (x64, w64, b64), gz.double())
    dw, db, dx = torch.empty(64, device=DEV), torch.empty(1, device=DEV), torch.empty((B, H, H, 64), device=DEV)
    gzd, xd, wd = gz.reshape(-1).to(DEV), to_nhwc(x.detach()), w.detach().reshape(-1).to(DEV)
    cabi.check(lib.ld_seg_head_backward(gzd.data_ptr(), xd.data_ptr(), wd.data_ptr(),
                                        work.data_ptr(), dw.data_ptr(), db.data_ptr(), dx.data_ptr(), M, 64, st()),
               "seg_head_backward")
    reduction_bound(dw.cpu().view_as(gw64), gw64, gw, f"head dW B={B} {H}^2")
    reduction_bound(db.cpu(), gb64, gb, f"head db B={B} {H}^2")
    assert rel_err(to_nchw(dx), gx) <= TOL


def adam_call(entries, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """One ld_seg_adam call at step t over (param, grad, m, v, dims, grad strides, mirrors) entries."""
    arr = (cabi.SegAdamTensor * len(entries))()
    for a, (p, g, m, v, dims, gs, mirrors) in zip(arr, entries):
        a.param, a.grad, a.m, a.v = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
        (a.d0, a.d1, a.d2), (a.gs0, a.gs1, a.gs2) = dims, gs
        for k, (buf, off, s0, s1, s2) in enumerate(mirrors):
            if k == 0:
                a.mirror0, a.m0_off, a.m0_s0, a.m0_s1, a.m0_s2 = buf.data_ptr(), off, s0, s1, s2
            else:
                a.mirror1, a.m1_off, a.m1_s0, a.m1_s1, a.m1_s2 = buf.data_ptr(), off, s0, s1, s2
    cabi.check(cabi.lib().ld_seg_adam(arr, len(entries), b1, b2, eps, lr / (1.0 - b1 ** t), float(np.sqrt(1.0 - b2 ** t)), st()),
               "seg_adam")


def test_adam_three_steps_against_torch_optim():
    """allclose(rtol=2.4e-7, atol=1e-8): two ulps of the parameter plus 1e-5 of lr.  One call over two tensors: one in a
    convolution's layouts (parameter OIHW, gradient OHWI) with two mirrors -- OHWI with the input channels padded from 5 to
    8 (pre-zeroed) and the data gradient's flipped, transposed layout (negative stride, offset 8 co) -- and one flat.  The
    mirrors are bitwise what ld_seg_permute3 makes of the updated parameter."""
    co, ci, cp = 8, 5, 8
    p_conv, p_flat = rnd((co, ci, 3, 3), 23), rnd((300,), 24)
    theirs = [p_conv.clone().requires_grad_(True), p_flat.clone().requires_grad_(True)]
    opt = torch.optim.Adam(theirs, lr=1e-3)
    mine = [p_conv.to(DEV), p_flat.to(DEV)]
    mom = [(torch.zeros_like(p), torch.zeros_like(p)) for p in mine]
    wf, wb = torch.zeros(co * 9 * cp, device=DEV), torch.zeros(ci * 9 * co, device=DEV)
    mirrors = ((wf, 0, 9 * cp, 1, cp), (wb, 8 * co, 1, 9 * co, -co))
    for t in range(1, 4):
        grads = [rnd((co, ci, 3, 3), 30 + t) * 10.0 ** (-t), rnd((300,), 40 + t)]
        for p, g in zip(theirs, grads):
            p.grad = g.clone()
        opt.step()
        g_ohwi = grads[0].permute(0, 2, 3, 1).contiguous().to(DEV)
        g_flat = grads[1].to(DEV)
        adam_call([(mine[0], g_ohwi, *mom[0], (co, ci, 9), (9 * ci, 1, ci), mirrors),
                   (mine[1], g_flat, *mom[1], (1, 1, 300), (0, 0, 1), ())], t)
    for m, th in zip(mine, theirs):
        assert torch.allclose(m.cpu(), th.detach(), rtol=2.4e-7, atol=1e-8), float((m.cpu() - th.detach()).abs().max())
        assert not torch.equal(m.cpu(), p_conv if m.dim() == 4 else p_flat)
    for buf, off, *strides in mirrors:
        assert torch.equal(buf, permute3(mine[0], buf.numel(), (co, ci, 9), off, strides))
    assert torch.equal(wf.view(co, 9, cp)[:, :, :ci].cpu(), mine[0].cpu().permute(0, 2, 3, 1).reshape(co, 9, ci))
    assert not wf.view(co, 9, cp)[:, :, ci:].any()                 # the padded lanes are still zero


def test_adam_groups_are_the_same_update_as_one_tensor_per_call():
    """LD_SEG_ADAM_GROUP + 1 tensors in one call (two launches; sizes across the 256-thread block edges, one [3][5][7] with
    a permuted gradient) against clones updated one tensor per call: the arithmetic is per element, so bitwise."""
    sizes = [1, 255, 256, 257, (3, 5, 7)] + [2 + 37 * k for k in range(cabi.SEG_ADAM_GROUP - 4)]
    assert len(sizes) == cabi.SEG_ADAM_GROUP + 1

    def entries():
        out = []
        for k, n in enumerate(sizes):
            dims = n if isinstance(n, tuple) else (1, 1, n)
            numel = dims[0] * dims[1] * dims[2]
            g = rnd((numel,), 500 + k).to(DEV)
            gs = (1, 21, 3) if isinstance(n, tuple) else (0, 0, 1)      # [3][5][7] read from a [5][7][3] buffer
            out.append((rnd((numel,), 400 + k).to(DEV), g, torch.zeros(numel, device=DEV), torch.zeros(numel, device=DEV), dims,
                        gs, ()))
        return out
    together, apart = entries(), entries()
    for t in (1, 2):
        adam_call(together, t)
        for e in apart:
            adam_call([e], t)
    for k, (a, b) in enumerate(zip(together, apart)):
        for x, y, what in zip(a[:4], b[:4], ("param", "grad", "m", "v")):
            assert torch.equal(x, y), (k, what)
        assert not torch.equal(a[0].cpu(), rnd((a[0].numel(),), 400 + k))
    # the permuted gradient was read through its strides: the first step's m is (1 - beta1) g
    g357 = together[4][1].view(5, 7, 3).permute(2, 0, 1).reshape(-1)
    m1 = torch.zeros_like(g357)
    adam_call([(together[4][0].clone(), together[4][1], m1, torch.zeros_like(g357), (3, 5, 7), (1, 21, 3), ())], 1)
    assert torch.equal(m1, g357 * float(np.float32(1.0 - 0.9)))


# ------------------------------------------------------------------------------------------------ whole net
def g19():
    g = np.load(os.path.join(GOLD, "g19_segtrain.npz"))
    sd = weights.procedural_seg_state_dict(int(g["seed"]))
    batches = [(torch.from_numpy(g["x"][b]), torch.from_numpy(g["target"][b].astype(np.float32))) for b in range(g["x"].shape[0])]
    return g, sd, batches


def g19_net(sd):
    net = ldh.SegUNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net.to(DEV).train()


def test_whole_net_loss_statistics_and_gradients_at_the_initial_weights():
    """HIP loss_and_grads on G19's six batches against the restatement in fp64 run here.
    Continuous quantities on all six: loss within 1e-5 |loss|, batch statistics within relative 1e-5, the head's two
    gradients within relative L2 1e-5.  Loose tier: all 64 parameters within 4 x grad_spread (relative L2) on all six.
    Tight tier: on at least two batches at least 32 parameters within 1e-4 (a ReLU sign flip may excuse some batches,
    a systematic error moves all of them).
    Measured on an MI355X (batches 0..5): loss 2.3e-8, 7e-9, 3.7e-8, 1.6e-8, 1.2e-8, 2.2e-8; statistics 2.1e-6 .. 2.7e-6;
    head gradients 2.6e-7 .. 3.5e-7 / 1.1e-8 .. 8.8e-8; worst parameter 6.8e-5, 5.5e-6, 5.6e-3, 2.4e-3, 1.2e-2, 5.7e-6
    (loose bound 4 x 1.797e-2 = 7.2e-2); parameters within 1e-4: 64, 64, 7, 5, 6, 64 (finding 119)."""
    g, sd, batches = g19()
    net = g19_net(sd)
    tr = ldh.SegTrainer(net)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    loose = 4.0 * float(g["grad_spread"])
    clean = []
    for b, (x, t) in enumerate(batches):
        params, buffers = segtrain_ref.params_of(sd, torch.float64)
        stats = {}
        loss64, grads64 = segtrain_ref.loss_and_grads(params, buffers, x, t, update_running=False, stats=stats)
        loss, grads = tr.loss_and_grads(x.to(DEV), t.to(DEV))
        e_loss = abs(float(loss) - float(loss64)) / abs(float(loss64))
        assert list(grads.keys()) == list(grads64.keys())
        rel = {k: segtrain_ref.rel_l2(grads[k].cpu(), grads64[k]) for k in grads}
        for k in grads:
            assert grads[k].shape == grads64[k].shape, k
        plan = net._train.plans[(4, 32, 32)]
        e_stat = 0.0
        for i, dc in enumerate(("inc.", "down1.maxpool_conv.1.", "down2.maxpool_conv.1.", "down3.maxpool_conv.1.",
                                "down4.maxpool_conv.1.", "up1.conv.", "up2.conv.", "up3.conv.", "up4.conv.")):
            for j, sk in ((1, "stat1"), (4, "stat2")):
                s = plan["blocks"][i][sk].view(3, -1).cpu().double()
                e_stat = max(e_stat, rel_err(s[0], stats[f"{dc}double_conv.{j}.mean"]),
                             rel_err(s[1], stats[f"{dc}double_conv.{j}.var"]))
        n_clean = sum(r <= 1e-4 for r in rel.values())
        clean.append(n_clean)
        print(f"batch {b}: loss rel err {e_loss:.2e}, statistics {e_stat:.2e}, head grads {rel['outc.conv.weight']:.2e} / "
              f"{rel['outc.conv.bias']:.2e}, worst parameter {max(rel.values()):.2e} (loose bound {loose:.2e}), "
              f"{n_clean} of 64 within 1e-4")
        assert e_loss <= 1e-5 and e_stat <= 1e-5, (b, e_loss, e_stat)
        assert rel["outc.conv.weight"] <= 1e-5 and rel["outc.conv.bias"] <= 1e-5, (b, rel["outc.conv.weight"], rel["outc.conv.bias"])
        assert max(rel.values()) <= loose, (b, max(rel, key=rel.get), max(rel.values()), loose)
    assert sum(c >= 32 for c in clean) >= 2, clean
    for k, v in net.state_dict().items():                          # neither parameters nor running statistics moved
        assert torch.equal(v, before[k]), k


def test_six_adam_steps_follow_the_fp64_run():
    """Losses within 4 x loss_spread of G19's fp64 losses, the last below 0.8 of the first, all finite; the running
    statistics after the first step within relative 1e-5.
    Measured on an MI355X: losses 1.86250, 1.55881, 1.41221, 1.41616, 1.36054, 1.28159; distance to the fp64 losses 4e-8,
    6e-8, 2e-7, 1e-6, 2.2e-5, 2.6e-5 (bound 4 x 4.68e-5 = 1.9e-4); running statistics 1.1e-6."""
    g, sd, batches = g19()
    net = g19_net(sd)
    tr = ldh.SegTrainer(net)
    bound = 4.0 * float(g["loss_spread"])
    losses = []
    for b, (x, t) in enumerate(batches):
        loss = tr.step(x.to(DEV), t.to(DEV))
        assert loss.is_cuda and loss.dim() == 0
        losses.append(loss)
        if b == 0:
            e = 0.0
            for k, v in net.state_dict().items():
                if "running_" in k:
                    e = max(e, rel_err(v.cpu().double(), torch.from_numpy(g["step1." + k])))
                elif k.endswith("num_batches_tracked"):
                    assert int(v) == 1
            print(f"running statistics after the first step: worst rel err {e:.2e}")
            assert e <= 1e-5, e
    losses = [float(l) for l in losses]
    errs = [abs(a - float(r)) for a, r in zip(losses, g["loss_steps"])]
    print(f"six steps: losses {['%.5f' % l for l in losses]}, |err| to fp64 {['%.1e' % e for e in errs]} (bound {bound:.1e})")
    assert all(np.isfinite(losses)) and max(errs) <= bound and losses[-1] < 0.8 * losses[0]
    assert tr.t == 6 and int(net.inc.double_conv[1].num_batches_tracked) == 6


def packed_copies(state):
    out = {}
    for i, pair in enumerate(state.convs):
        for j, cv in enumerate(pair):
            out[f"conv {i}.{j} wf"] = cv.wf
            if cv.wb is not None:
                out[f"conv {i}.{j} wb"] = cv.wb
    for i, u in enumerate(state.ups):
        out.update({f"up {i} {k}": u[k] for k in ("wf", "wb", "bias4")})
    return out


def assert_packed_weights_are_current(net):
    """Every kernel-layout copy equals a repack from the parameters, bit for bit; inc's padded lanes are zero."""
    state = net._train
    kept = {k: v.clone() for k, v in packed_copies(state).items()}
    assert len(kept) == 18 + 17 + 4 * 3
    state.pack()
    for k, v in packed_copies(state).items():
        assert torch.equal(v, kept[k]), k
    inc = state.convs[0][0]
    assert inc.cin_k == 64 and not inc.wf.view(inc.cout, 9, 64)[:, :, inc.cin:].any()
    assert torch.equal(inc.wf.view(inc.cout, 9, 64)[:, :, :inc.cin],
                       inc.conv.weight.detach().permute(0, 2, 3, 1).reshape(inc.cout, 9, inc.cin))


def test_steps_keep_the_packed_weights_current():
    """No repack follows a step: after two of them every wf / wb / bias4 is what pack() makes of the parameters, and a fresh
    module loaded from state_dict() (packed at construction) gives the same train-mode logits."""
    g, sd, batches = g19()
    x, t = batches[0][0].to(DEV), batches[0][1].to(DEV)
    net = g19_net(sd)
    tr = ldh.SegTrainer(net)
    tr.step(x, t)
    tr.step(x, t)
    fresh = ldh.SegUNet()
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    logits = net(x)
    assert torch.equal(fresh.to(DEV).train()(x), logits)
    assert_packed_weights_are_current(net)


def test_train_mode_forward_equals_the_trainers_forward():
    g, sd, batches = g19()
    x, t = batches[0][0].to(DEV), batches[0][1].to(DEV)
    net = g19_net(sd)
    logits = net(x)
    assert logits.shape == (4, 1, 32, 32) and int(net.up2.conv.double_conv[4].num_batches_tracked) == 1
    net2 = g19_net(sd)
    tr = ldh.SegTrainer(net2)
    tr.loss_and_grads(x, t)
    assert torch.equal(net2._train.plans[(4, 32, 32)]["logits"], logits)
    assert int(net2.up2.conv.double_conv[4].num_batches_tracked) == 0
    rm = net.inc.double_conv[1].running_mean
    assert not torch.equal(rm, net2.inc.double_conv[1].running_mean)
    # eval mode afterwards: the running statistics just updated are used (cache invalidated), and differ from train mode
    ev = net.eval()(x)
    assert torch.isfinite(ev).all() and not torch.equal(ev, logits)
    with pytest.raises(ValueError, match="two values"):
        net.train()(x[:1, :, :16, :16])


def test_step_is_deterministic():
    g, sd, batches = g19()
    x, t = batches[1][0].to(DEV), batches[1][1].to(DEV)
    runs = []
    for _ in range(2):
        net = g19_net(sd)
        tr = ldh.SegTrainer(net)
        loss0, grads = tr.loss_and_grads(x, t)
        loss = tr.step(x, t)
        runs.append((loss0, loss, grads, {k: v.clone() for k, v in net.state_dict().items()}))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], a[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def test_trained_net_in_eval_mode_and_the_saved_file(tmp_path):
    g, sd, batches = g19()
    net = g19_net(sd)
    x = batches[0][0].to(DEV)
    untrained = net.eval()(x)
    tr = ldh.SegTrainer(net)
    dev_batches = [(a.to(DEV), b.to(DEV)) for a, b in batches]
    out = str(tmp_path / "best_dice.pth")
    res = tr.fit(dev_batches[:4], dev_batches[4:], epochs=1, out_path=out, log=str(tmp_path))
    # dice = (2 sum p t + eps) / (sum p + sum t + eps) > 0 = the initial best: the first epoch always writes the file
    assert res["best_epoch"] == 0 and 0.0 < res["best_dice"] <= 1.0 and len(res["val"]) == 1 and os.path.exists(out)
    dice, bce = tr.evaluate(*dev_batches[4])
    logits = net.eval()(dev_batches[4][0])
    bce_ref, dice_ref = segtrain_ref.loss_terms(logits.cpu().double(), batches[4][1].double())
    assert abs(dice - (1.0 - float(dice_ref))) <= 1e-5 and abs(bce - float(bce_ref)) <= 1e-5 * max(1.0, float(bce_ref))
    trained = net.eval()(x)                                      # the file fit() wrote holds these weights
    assert torch.isfinite(trained).all() and not torch.equal(trained, untrained)
    fresh = ldh.SegUNet()
    assert checkpoint.load_seg_checkpoint(out, fresh) == {"n_tensors": 118}
    assert torch.equal(fresh.to(DEV).eval()(x), trained)


def test_three_channels_and_a_non_square_input_against_fp64():
    """n_channels = 3 (the padded inc convolution: the image copy, the strided view of its padded weight gradient, Adam's
    strided read) at H != W (the kernels' separate row / column arithmetic), B = 2 at 32 x 48: loss_and_grads against the
    restatement in fp64 with the whole-net bounds (loss 1e-5, the head's gradients relative L2 1e-5, every parameter within
    4 x grad_spread of G19), then one step: every parameter moves by about lr against its gradient's sign."""
    g = np.load(os.path.join(GOLD, "g19_segtrain.npz"))
    sd = weights.procedural_seg_state_dict(int(g["seed"]), n_channels=3)
    B, H, W = 2, 32, 48
    base = rnd((B, 1, H, W), 77, 0.0, 1.0)
    ramp = torch.linspace(0.0, 2.5, W).view(1, 1, 1, W) * torch.linspace(0.5, 1.0, H).view(1, 1, H, 1)
    x = torch.cat([base + ramp, 0.5 * base - 0.3 * ramp, ramp - base], dim=1) - 0.6
    t = ((base + ramp) > 2.6).float()
    assert 0.01 < float(t.mean()) < 0.3
    net = ldh.SegUNet(n_channels=3)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    net = net.to(DEV).train()
    tr = ldh.SegTrainer(net)
    params, buffers = segtrain_ref.params_of(sd, torch.float64)
    loss64, grads64 = segtrain_ref.loss_and_grads(params, buffers, x, t)
    loss, grads = tr.loss_and_grads(x.to(DEV), t.to(DEV))
    e_loss = abs(float(loss) - float(loss64)) / abs(float(loss64))
    rel = {k: segtrain_ref.rel_l2(grads[k].cpu(), grads64[k]) for k in grads64}
    loose = 4.0 * float(g["grad_spread"])
    print(f"3 channels, 32 x 48: loss rel err {e_loss:.2e}, head grads {rel['outc.conv.weight']:.2e} / {rel['outc.conv.bias']:.2e}, "
          f"inc.double_conv.0.weight {rel['inc.double_conv.0.weight']:.2e}, worst {max(rel.values()):.2e} (bound {loose:.2e}), "
          f"{sum(r <= 1e-4 for r in rel.values())} of 64 within 1e-4")
    assert grads["inc.double_conv.0.weight"].shape == (64, 3, 3, 3)
    assert e_loss <= 1e-5 and rel["outc.conv.weight"] <= 1e-5 and rel["outc.conv.bias"] <= 1e-5
    assert max(rel.values()) <= loose, (max(rel, key=rel.get), max(rel.values()))
    before = net.inc.double_conv[0].weight.detach().clone()
    tr.step(x.to(DEV), t.to(DEV))
    assert_packed_weights_are_current(net)                      # cin = 3 padded to 64: the mirror writes 3 lanes of 64
    moved = (net.inc.double_conv[0].weight.detach() - before).cpu()
    g0 = grads64["inc.double_conv.0.weight"]
    big = g0.abs() > 1e-2 * g0.abs().max()                      # Adam's first step: -lr g / (|g| + eps), about -lr sign(g)
    assert int(big.sum()) > 100
    assert torch.allclose(moved[big], (-1e-3 * g0[big] / (g0[big].abs() + 1e-8)).float(), rtol=1e-2, atol=0)


def test_train_seg_tool_end_to_end(tmp_path):
    g, sd, batches = g19()
    mini = abs((0 - 610.7180906353575) / 1018.7631901605115)
    imgs = np.concatenate([b[0].numpy() for b in batches[:3]]) + np.float32(mini)      # the tool applies seg_preprocess
    masks = np.concatenate([b[1].numpy() for b in batches[:3]])
    np.save(tmp_path / "img.npy", imgs)
    np.save(tmp_path / "mask.npy", masks)
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_seg.py"), "--images", str(tmp_path / "img.npy"),
                        "--masks", str(tmp_path / "mask.npy"), "--epochs", "2", "--batch-size", "4", "--out", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (out_dir / "train.csv").exists() and (out_dir / "val.csv").exists()
    rows = open(out_dir / "train.csv").read().strip().splitlines()
    assert rows[0] == "epoch,loss" and len(rows) == 3 and all(np.isfinite(float(x.split(",")[1])) for x in rows[1:])
    assert (out_dir / "best_dice.pth").exists()                  # dice > 0 = the initial best after the first epoch
    fresh = ldh.SegUNet()
    assert checkpoint.load_seg_checkpoint(str(out_dir / "best_dice.pth"), fresh) == {"n_tensors": 118}
    assert not torch.equal(fresh.outc.conv.bias, torch.from_numpy(np.asarray(weights.procedural_seg_state_dict(0)["outc.conv.bias"])))
