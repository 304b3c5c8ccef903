"""GPU tests of the second slice of the denoiser's backward pass: the RMSNorm and attention-core kernels of
csrc/linattn_grad.hip one by one, then ``LinearAttention`` as a whole and under torch.autograd.

Yardstick: torch.autograd in fp64 on the CPU through oracle.unet_ref.linear_attention / rms_norm (tests/linattn_ref.py).
What is element-wise given its inputs (RMSNorm's out and dx) is held to RTOL["fp32"] = 2e-5 of the tensor's max-abs against
fp32 eager torch; everything behind a sum over pixels to max(1e-5, 4 d) of the fp64 value, d = fp32 eager torch's own
distance to it (resblock_ref.reduction_bound).  Every buffer handed to a kernel is filled with NaN first, padding included,
and padding must come out as zero.  Every test prints HIP's and torch's distances; the values of an MI355X run are not
recorded in the docstrings yet (no MI355X was available when the tests were written: docs/findings.md, 122)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi

from hip_helpers import DEV, NAN, RTOL, nans, pad64, padded, st, unpadded
import linattn_ref as R
import resblock_ref

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def work(nbytes):
    assert int(nbytes) > 0
    return nans(int(nbytes) // 8, dtype=F64)


# ------------------------------------------------------------------------------------------------ 1. RMSNorm
def hip_rms(x, g, dout, ldc, in_place=False):
    B, Cc, H, W = x.shape
    lib = cabi.lib()
    xp, gd = padded(x, ldc), g.to(DEV)
    rinv, out = nans(B, H, W), nans(B, H, W, ldc)
    cabi.check(lib.ld_dn_rms_forward(xp.data_ptr(), gd.data_ptr(), rinv.data_ptr(), out.data_ptr(), B, H, W, Cc, ldc, st()),
               "dn_rms_forward")
    src = padded(dout, ldc)
    dx = src if in_place else nans(B, H, W, ldc)
    dg = nans(Cc)
    cabi.check(lib.ld_dn_rms_backward(src.data_ptr(), xp.data_ptr(), gd.data_ptr(), rinv.data_ptr(),
                                      work(lib.ld_dn_rms_work_bytes(B, H, W, Cc)).data_ptr(), dg.data_ptr(), dx.data_ptr(), B, H,
                                      W, Cc, ldc, st()), "dn_rms_backward")
    return out, dx, dg


RMS_CASES = [(2, 32, 5, 3, 64), (3, 64, 7, 7, 64), (2, 96, 9, 9, 128), (1, 256, 8, 8, 256)]


def rms_inputs(B, Cc, H, W):
    key = 10 * Cc + H
    return (R.uniform((B, Cc, H, W), key, -2.0, 2.0) + 0.3, R.uniform((Cc,), key + 1, 0.5, 1.5),
            R.uniform((B, Cc, H, W), key + 2) / (B * H * W))


@pytest.mark.parametrize("B,Cc,H,W,ldc", RMS_CASES)
def test_rmsnorm_forward_and_backward(B, Cc, H, W, ldc):
    """ld_dn_rms_forward / ld_dn_rms_backward against autograd through oracle.unet_ref.rms_norm; the padding of x and dout
    holds NaN (never read) and comes out as zeros; dx written over dout equals dx written elsewhere bit for bit.
    The distances on an MI355X are not recorded yet: none was available when the test was written."""
    x, g, dout = rms_inputs(B, Cc, H, W)
    out, dx, dg = hip_rms(x, g, dout, ldc)
    _, dx_in, dg_in = hip_rms(x, g, dout, ldc, in_place=True)
    ref32, ref64 = R.rms(x, g, dout, F32), R.rms(x, g, dout, F64)
    tag = f"rms B{B} C{Cc} {H}x{W}"
    R.elementwise_bound(unpadded(out, Cc), ref32["out"], ref64["out"], tag + " out", RTOL["fp32"])
    R.elementwise_bound(unpadded(dx, Cc), ref32["x"], ref64["x"], tag + " dx", RTOL["fp32"])
    R.reduction_bound(dg.cpu(), ref64["g"], ref32["g"], tag + " dg")
    if ldc > Cc:
        assert bool((out[..., Cc:] == 0).all()) and bool((dx[..., Cc:] == 0).all())
    assert torch.equal(dx, dx_in) and torch.equal(dg, dg_in)


def test_rmsnorm_with_an_all_zero_pixel():
    """A pixel whose channels are all zero: the forward gives zeros there, the backward is finite everywhere and within the
    bounds at the other pixels (the zero pixel is masked out on both sides)."""
    B, Cc, H, W, ldc = 2, 32, 5, 3, 64
    x, g, dout = rms_inputs(B, Cc, H, W)
    x[1, :, 2, 1] = 0.0
    out, dx, dg = hip_rms(x, g, dout, ldc)
    ref32, ref64 = R.rms(x, g, dout, F32), R.rms(x, g, dout, F64)
    out, dx = unpadded(out, Cc), unpadded(dx, Cc)
    assert bool((out[1, :, 2, 1] == 0).all())
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dg).all())
    keep = torch.ones(B, 1, H, W)
    keep[1, :, 2, 1] = 0.0
    R.elementwise_bound(out, ref32["out"], ref64["out"], "rms zero pixel out", RTOL["fp32"])
    R.elementwise_bound(dx * keep, ref32["x"] * keep, ref64["x"] * keep, "rms zero pixel dx", RTOL["fp32"])
    R.reduction_bound(dg.cpu(), ref64["g"], ref32["g"], "rms zero pixel dg")


# ------------------------------------------------------------------------------------------------ 2, 3. the attention core
CORE_CASES = [(2, 1, 5, 3, False), (2, 4, 14, 14, False), (1, 2, 33, 31, False), (3, 4, 8, 8, False), (2, 4, 14, 14, True)]


@functools.lru_cache(maxsize=None)
def core_case(B, heads, H, W, shifted):
    """Inputs, the HIP results of the four passes and the two references of one case (computed once, never changed)."""
    hidden, n = 32 * heads, H * W
    key = 1000 * heads + 10 * H + W
    qkv = R.uniform((B, 3 * hidden, H, W), key, -2.0, 2.0)
    if shifted:                                          # k logits near +100 in the last quarter of the pixels only
        qkv.reshape(B, 3 * hidden, n)[:, hidden:2 * hidden, n - n // 4:] += 100.0
    dout = R.uniform((B, hidden, H, W), key + 1)
    lib = cabi.lib()
    ld3, ldo = pad64(3 * hidden), pad64(hidden)
    qp, dop = padded(qkv, ld3), padded(dout, ldo)
    ctx, kstat, out = nans(B, heads, 32, 32), nans(B, heads, 32, 2), nans(B, H, W, ldo)
    cabi.check(lib.ld_dn_la_context(qp.data_ptr(), work(lib.ld_dn_la_work_bytes(B, heads, H, W)).data_ptr(), ctx.data_ptr(),
                                    kstat.data_ptr(), B, H, W, heads, ld3, st()), "dn_la_context")
    cabi.check(lib.ld_dn_la_out(qp.data_ptr(), ctx.data_ptr(), out.data_ptr(), B, H, W, heads, ld3, ldo, st()), "dn_la_out")
    dctx, rk, dqkv = nans(B, heads, 32, 32), nans(B, heads, 32), nans(B, H, W, ld3)
    cabi.check(lib.ld_dn_la_backward_reduce(qp.data_ptr(), dop.data_ptr(), ctx.data_ptr(),
                                            work(lib.ld_dn_la_work_bytes(B, heads, H, W)).data_ptr(), dctx.data_ptr(),
                                            rk.data_ptr(), B, H, W, heads, ld3, ldo, st()), "dn_la_backward_reduce")
    cabi.check(lib.ld_dn_la_backward_apply(qp.data_ptr(), dop.data_ptr(), ctx.data_ptr(), kstat.data_ptr(), dctx.data_ptr(),
                                           rk.data_ptr(), dqkv.data_ptr(), B, H, W, heads, ld3, ldo, st()),
               "dn_la_backward_apply")
    torch.cuda.synchronize()
    hip = dict(ctx=ctx.cpu(), kstat=kstat.cpu(), out=out.cpu(), dctx=dctx.cpu(), rk=rk.cpu(), dqkv=dqkv.cpu())
    return hip, R.core(qkv, heads, dout, F32), R.core(qkv, heads, dout, F64)


@pytest.mark.parametrize("B,heads,H,W,shifted", CORE_CASES)
def test_context_and_output_passes(B, heads, H, W, shifted):
    """ld_dn_la_context / ld_dn_la_out from a qkv tensor fed directly, against the fp64 formulas.  15 pixels are fewer than a
    wave, 1,023 pixels are 16 parts of the split, 196 pixels are four; the shifted case has its k logits near +100 in the
    last quarter of the pixels only (two of its four parts): a missing maximum overflows, a wrong merge of the parts misses
    the bound."""
    hip, ref32, ref64 = core_case(B, heads, H, W, shifted)
    hidden = 32 * heads
    tag = f"core B{B} h{heads} {H}x{W}{' shifted' if shifted else ''}"
    splits = int(cabi.lib().ld_dn_la_splits(B, heads, H, W))
    print(f"{tag}: {splits} parts")
    if H * W > 64:
        assert splits >= 2
    for v in hip.values():
        assert bool(torch.isfinite(v).all())
    R.reduction_bound(hip["kstat"][..., 0], ref64["m"], ref32["m"], tag + " m")
    R.reduction_bound(hip["kstat"][..., 1], ref64["Z"], ref32["Z"], tag + " Z")
    R.reduction_bound(hip["ctx"], ref64["ctx"], ref32["ctx"], tag + " ctx")
    R.reduction_bound(hip["out"][..., :hidden].permute(0, 3, 1, 2), ref64["out"], ref32["out"], tag + " out")
    assert bool((hip["out"][..., hidden:] == 0).all())


@pytest.mark.parametrize("B,heads,H,W,shifted", CORE_CASES)
def test_backward_reduce_and_apply(B, heads, H, W, shifted):
    """ld_dn_la_backward_reduce / ld_dn_la_backward_apply against autograd through the same formulas: dctx, dqkv (and with
    it rk, which dk is made of); the padding channels of dqkv are zero."""
    hip, ref32, ref64 = core_case(B, heads, H, W, shifted)
    hidden = 32 * heads
    tag = f"core backward B{B} h{heads} {H}x{W}{' shifted' if shifted else ''}"
    R.reduction_bound(hip["dctx"], ref64["dctx"], ref32["dctx"], tag + " dctx")
    R.reduction_bound(hip["dqkv"][..., :3 * hidden].permute(0, 3, 1, 2), ref64["dqkv"], ref32["dqkv"], tag + " dqkv")
    for i, name in enumerate("qkv"):                     # each third by itself: dq, dk, dv differ in scale
        sl = slice(i * hidden, (i + 1) * hidden)
        R.reduction_bound(hip["dqkv"][..., sl].permute(0, 3, 1, 2), ref64["dqkv"][:, sl], ref32["dqkv"][:, sl], f"{tag} d{name}")
    assert bool((hip["dqkv"][..., 3 * hidden:] == 0).all())


# ------------------------------------------------------------------------------------------------ 4. the module
def hip_module(dim, heads, sd):
    mod = ldh.LinearAttention(dim, heads=heads)
    mod.load_state_dict(sd)
    return mod.to(DEV)


def hip_forward_backward(mod, x, dout):
    xd = x.to(DEV).requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    out = mod(xd)
    out.backward(dout.to(DEV))
    grads = {"x": xd.grad}
    grads.update({k: p.grad for k, p in mod.named_parameters() if p.grad is not None})
    return out.detach(), grads


MODULE_CASES = [(2, 32, 1, 5, 3), (2, 64, 4, 14, 14), (1, 96, 2, 33, 31), (3, 128, 4, 8, 8)]


@pytest.mark.parametrize("B,dim,heads,H,W", MODULE_CASES)
def test_module_forward_and_every_gradient(B, dim, heads, H, W):
    """Forward and the gradients of x and of the five parameters against the yardstick, dout = uniform / (B H W).  The same
    call again, and again with every buffer the module allocates filled with NaN first, gives the same bits: no padded
    channel, no stale scratch and no arrival order enters a result."""
    sd = R.make_attn(dim, heads, key=dim + heads)
    x = R.uniform((B, dim, H, W), 11 * dim + H)
    dout = R.uniform((B, dim, H, W), 17 * dim + H) / (B * H * W)
    mod = hip_module(dim, heads, sd)
    out, grads = hip_forward_backward(mod, x, dout)
    (o32, g32), (o64, g64) = (R.yardstick(sd, x, dout, heads, dtype=dt) for dt in (F32, F64))
    tag = f"module B{B} dim{dim} h{heads} {H}x{W}"
    assert set(grads) == set(g64), set(grads) ^ set(g64)
    R.reduction_bound(out.cpu(), o64, o32, tag + " out")
    for k in g64:
        assert grads[k].shape == g64[k].shape, k
        R.reduction_bound(grads[k].cpu(), g64[k], g32[k], f"{tag} d {k}")
    for fill in (None, NAN):
        mod.debug_fill = fill
        out2, grads2 = hip_forward_backward(mod, x, dout)
        assert torch.equal(out, out2)
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), (k, fill)


# ------------------------------------------------------------------------------------------------ 5. autograd behaviour
def test_autograd_contract():
    """backward twice accumulates into .grad; a no_grad forward equals the grad-mode forward bit for bit and needs no
    gradient; autograd.grad works; an in-place change of a parameter (its _version moves) rebuilds the packed weights."""
    dim, heads = 32, 2
    sd = R.make_attn(dim, heads, key=31)
    x, dout = R.uniform((2, dim, 7, 7), 81), R.uniform((2, dim, 7, 7), 83)
    mod = hip_module(dim, heads, sd)
    out, g1 = hip_forward_backward(mod, x, dout)
    g1 = {k: v.clone() for k, v in g1.items()}
    mod(x.to(DEV)).backward(dout.to(DEV))                                   # a second backward without zero_grad
    for k, p in mod.named_parameters():
        assert torch.equal(p.grad, 2 * g1[k]), k
    with torch.no_grad():
        quiet = mod(x.to(DEV))
    assert not quiet.requires_grad and torch.equal(quiet, out)
    (gw,) = torch.autograd.grad(mod(x.to(DEV).requires_grad_(True)).sum(), [mod.to_qkv.weight])
    assert gw.shape == mod.to_qkv.weight.shape
    with torch.no_grad():
        mod.to_out[0].weight.mul_(0.5)
        mod.norm.g.add_(0.25)
        after = mod(x.to(DEV))
    assert not torch.equal(after, out)
    sd_new = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    assert R.rel_err(after.cpu(), R.forward(sd_new, x, heads, F64)) <= 1e-5


def test_module_reads_channels_last_in_place():
    """A channels_last x with dim = 64 is the kernels' NHWC already: same bits as from a contiguous x, x.grad included."""
    dim, heads = 64, 2
    sd = R.make_attn(dim, heads, key=5)
    x, dout = R.uniform((2, dim, 9, 6), 51), R.uniform((2, dim, 9, 6), 53)
    mod = hip_module(dim, heads, sd)
    out, grads = hip_forward_backward(mod, x, dout)
    xl = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    out2 = mod(xl)
    out2.backward(dout.to(DEV).contiguous(memory_format=torch.channels_last))
    assert torch.equal(out, out2) and torch.equal(grads["x"], xl.grad)
    assert torch.equal(grads["to_qkv.weight"], mod.to_qkv.weight.grad)
    _, g64 = R.yardstick(sd, x, dout, heads, dtype=F64)
    _, g32 = R.yardstick(sd, x, dout, heads, dtype=F32)
    R.reduction_bound(xl.grad.cpu(), g64["x"], g32["x"], "channels_last dx")
    assert torch.equal(xl.detach().cpu(), x)                                # the input itself was not written


def test_chain_of_a_block_and_the_attention_under_the_loss_gradient():
    """ResnetBlock(64, 64, time_emb_dim=128) -> attn(h) + h with LinearAttention(64) -> the gradient of the pred_v training
    loss (ld_p_losses_grad) as the upstream gradient, at B = 2, 12 x 12, against the fp64 yardstick of the same chain: dx
    and the parameter gradients of both modules.  The residual add is autograd's, between the two Functions."""
    B, dim, H, tdim, heads = 2, 64, 12, 128, 4
    sd1, sd2 = resblock_ref.make_block(dim, dim, tdim, key=21), R.make_attn(dim, heads, key=22)
    x, temb = R.uniform((B, dim, H, H), 61), R.uniform((B, tdim), 62)
    x0, nz = R.uniform((B, dim, H, H), 63), R.uniform((B, dim, H, H), 64)
    t = torch.tensor([0, 3])
    sab, s1m, lw = torch.tensor([0.99, 0.9, 0.7, 0.4]), torch.tensor([0.14, 0.43, 0.71, 0.92]), torch.tensor([1.0, 0.8, 0.5, 0.3])
    blk = ldh.ResnetBlock(dim, dim, time_emb_dim=tdim)
    blk.load_state_dict(sd1)
    blk, attn = blk.to(DEV), hip_module(dim, heads, sd2)
    xd, td = x.to(DEV).requires_grad_(True), temb.to(DEV)
    h = blk(xd, td)
    out = attn(h) + h
    od = out.detach().contiguous()
    up = nans(*od.shape)
    dev = [v.to(DEV) for v in (x0, nz, t.int(), sab, s1m, lw)]
    cabi.check(cabi.lib().ld_p_losses_grad(od.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                                           dev[3].data_ptr(), dev[4].data_ptr(), dev[5].data_ptr(), 1.0, up.data_ptr(), B,
                                           dim * H * H, cabi.OBJ["pred_v"], st()), "p_losses_grad")
    out.backward(up)
    got = {"x": xd.grad}
    got.update({"block." + k: p.grad for k, p in blk.named_parameters()})
    got.update({"attn." + k: p.grad for k, p in attn.named_parameters()})
    ref = {}
    for dt in (F32, F64):
        l1 = {k: v.to(dt).clone().requires_grad_(True) for k, v in sd1.items()}
        l2 = {k: v.to(dt).clone().requires_grad_(True) for k, v in sd2.items()}
        xin = x.to(dt).requires_grad_(True)
        hh = R.unet_ref.resnet_block({"a." + k: v for k, v in l1.items()}, "a", xin, temb.to(dt))
        o = R.unet_ref.linear_attention({"b." + k: v for k, v in l2.items()}, "b", hh, heads, 32) + hh
        ext = (slice(None), None, None, None)
        target = sab.to(dt)[t][ext] * nz.to(dt) - s1m.to(dt)[t][ext] * x0.to(dt)
        loss = (((o - target) ** 2).reshape(B, -1).mean(dim=1) * lw.to(dt)[t]).mean()
        names = ["x"] + ["block." + k for k in l1] + ["attn." + k for k in l2]
        ref[dt] = dict(zip(names, torch.autograd.grad(loss, [xin] + list(l1.values()) + list(l2.values()))))
    assert set(got) == set(ref[F64])
    for k in ref[F64]:
        R.reduction_bound(got[k].cpu(), ref[F64][k], ref[F32][k], "chain d " + k)


def test_adam_lowers_a_fixed_mse_at_every_step():
    """Five steps of torch.optim.Adam(module.parameters(), lr=1e-3) on a fixed batch: the optimiser's in-place updates move
    the parameters' versions, the kernel-layout weights follow, and the loss falls at every step."""
    sd = R.make_attn(32, 2, key=41)
    x, target = R.uniform((2, 32, 8, 8), 91).to(DEV), R.uniform((2, 32, 8, 8), 93).to(DEV)
    mod = hip_module(32, 2, sd)
    opt = torch.optim.Adam(mod.parameters(), lr=1e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = F.mse_loss(mod(x), target)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print("adam losses:", " ".join(f"{v:.6f}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_with_device_pointers():
    mod = ldh.LinearAttention(32, heads=1).to(DEV)
    with pytest.raises(ValueError, match="float32"):
        mod(torch.zeros(1, 32, 4, 4, dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError, match="CPU"):
        mod(torch.zeros(1, 32, 4, 4))
    with pytest.raises(ValueError, match="parameter"):
        ldh.LinearAttention(32, heads=1)(torch.zeros(1, 32, 4, 4, device=DEV))
    lib = cabi.lib()
    buf = torch.zeros(8192, device=DEV)
    p = buf.data_ptr()
    assert lib.ld_dn_rms_forward(p, p, None, None, 1, 4, 4, 32, 32, st()) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_rms_forward(p + 4, p, None, p, 1, 4, 4, 32, 32, st()) == -1 and b"aligned" in lib.ld_last_error()
    assert lib.ld_dn_rms_backward(p, p, p, p, p, p, p, 1, 4, 4, 32, 16, st()) == -1
    assert lib.ld_dn_la_context(p, p, p, p, 1, 4, 4, 0, 128, st()) == -1
    assert lib.ld_dn_la_out(p, p, p, 1, 4, 4, 1, 64, 64, st()) == -1                  # ld3 < 96
    assert lib.ld_dn_la_backward_reduce(p, p, p, p, p, None, 1, 4, 4, 1, 128, 64, st()) == -1
    assert lib.ld_dn_la_backward_apply(p, p + 4, p, p, p, p, p, 1, 4, 4, 1, 128, 64, st()) == -1
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
