"""GPU tests of ``act_storage="bf16"``: the four entry points that read or write a bf16 activation (csrc/conv16.hip,
csrc/denoiser_grad.hip) against the ones that read or write fp32, then ``ResnetBlock`` and ``DenoiserTrainer`` with the switch
against themselves without it.  Storing what the bf16 convolutions round anyway changes no bit, so every comparison is
``torch.equal``; no input holds a NaN or a subnormal.  Every output buffer holds NaN first."""
import ctypes as C

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd.trainable import TrainableModule

from hip_helpers import DEV, NAN, nans, pad64, padded, st
import conv16_ref as P
import resblock_ref as R
import unet_grad_ref as UR

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def normal(t):
    """No NaN, no infinity, no subnormal."""
    return bool(torch.isfinite(t).all()) and bool(((t == 0) | (t.abs() >= torch.finfo(F32).tiny)).all())


# ------------------------------------------------------------------------------------------------ 1. ld_dn_conv16_from16
def ohwi_bf16(w):
    return w.permute(0, 2, 3, 1).contiguous().to(DEV, BF16).reshape(-1)


def conv16_both(src, wb, shift, residual, cin, cout, k):
    """ld_dn_conv16 on ``src`` [B, H, W, cin] (fp32, device) and ld_dn_conv16_from16 on ``src.to(bfloat16)``."""
    B, H, W, _ = src.shape
    ones, sh = torch.ones(cout, device=DEV), shift.to(DEV, F32)
    src16 = src.to(BF16)
    assert normal(src) and src16.is_contiguous()
    outs = []
    for fn, s in ((cabi.lib().ld_dn_conv16, src), (cabi.lib().ld_dn_conv16_from16, src16)):
        out = nans(B, H, W, cout)
        a = cabi.PcConvArgs()
        a.src, a.weight, a.scale, a.shift, a.residual, a.out = s.data_ptr(), None, ones.data_ptr(), sh.data_ptr(), cabi.ptr(residual), out.data_ptr()
        a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout, a.ksize, a.stride, a.relu = B, H, W, cin, H, W, cout, k, 1, 0
        cabi.check(fn(C.byref(a), wb.data_ptr(), st()), "conv16")
        outs.append(out)
    return outs


@pytest.mark.parametrize("shape", P.CONV_SHAPES)
@pytest.mark.parametrize("kind", ["ties", "uniform"])
def test_conv16_from16_gives_conv16s_bits(shape, kind):
    """A partial tile, the seam between two images, ksize 1 and the residual + shift epilogue, on operands bf16 does not hold."""
    B, cin, cout, H, W, k = shape
    epi = shape == P.CONV_WITH_EPILOGUE
    if kind == "ties":
        x, w = P.ties_and_neighbours((B, cin, H, W), 5000 + cin + H).float(), P.trits((cout, cin, k, k), 5001 + cin + H).float()
    else:
        x, w = R.uniform((B, cin, H, W), 5002 + cin + H), R.uniform((cout, cin, k, k), 5003 + cin + H)
    shift = R.uniform((cout,), 5004 + cin) if epi else torch.zeros(cout)
    res = padded(R.uniform((B, cout, H, W), 5005 + cin), cout) if epi else None
    assert not torch.equal(P.q(x), x)
    want, got = conv16_both(padded(x, cin), ohwi_bf16(w), shift, res, cin, cout, k)
    assert not bool(want.isnan().any()) and bool(want.any())
    assert torch.equal(got, want)


@pytest.mark.parametrize("kind", ["ties", "uniform"])
def test_conv16_from16_as_the_data_gradient(kind):
    """The data-gradient use (Cin 64, Cout 32 padded to 64): a bf16 dy against the packed, flipped weight."""
    B, cin, cout, H, W, k = P.DGRAD_SHAPE
    cop, cip = pad64(cout), pad64(cin)
    if kind == "ties":
        dy, w = P.ties_and_neighbours((B, cout, H, W), 5100).float(), P.trits((cout, cin, k, k), 5101).float()
    else:
        dy, w = R.uniform((B, cout, H, W), 5102), R.uniform((cout, cin, k, k), 5103)
    wd = w.to(DEV).contiguous()
    fwd, dgr = nans(cop * k * k * cip, dtype=BF16), nans(cip * k * k * cop, dtype=BF16)
    cabi.check(cabi.lib().ld_dn_pack_conv16(wd.data_ptr(), fwd.data_ptr(), dgr.data_ptr(), cout, cop, cin, cip, k, st()), "dn_pack_conv16")
    want, got = conv16_both(padded(dy, cop, fill=0.0), dgr, torch.zeros(cip), None, cop, cip, k)
    assert not bool(want.isnan().any()) and bool(want.any())
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 2. ld_dn_wgrad16_from16
@pytest.mark.parametrize("shape,splits", P.WGRAD_CASES)
@pytest.mark.parametrize("kind", ["ties", "uniform"])
def test_wgrad16_from16_gives_wgrad16s_bits(shape, splits, kind):
    """Both split settings (the hand-picked one leaves the last split without a chunk); dy stays fp32."""
    B, cin, cout, H, W, k = shape
    lib = cabi.lib()
    if kind == "ties":
        dy, a = P.trits((B, cout, H, W), 5200 + cin + k).float(), P.ties_and_neighbours((B, cin, H, W), 5201 + cin + k).float()
    else:
        dy, a = R.uniform((B, cout, H, W), 5202 + cin + k), R.uniform((B, cin, H, W), 5203 + cin + k)
    assert not torch.equal(P.q(a), a)
    splits = int(lib.ld_seg_wgrad_splits(B, H, W, cin, cout, k)) if splits is None else splits
    n = cout * k * k * cin
    dyp, ap = padded(dy, cout), padded(a, cin)
    ap16 = ap.to(BF16)
    assert normal(ap)
    res = []
    for fn, act in ((lib.ld_dn_wgrad16, ap), (lib.ld_dn_wgrad16_from16, ap16)):
        work, dw = nans(splits * n), nans(n)
        cabi.check(fn(dyp.data_ptr(), act.data_ptr(), work.data_ptr(), dw.data_ptr(), B, H, W, cin, cout, k, splits, st()), "wgrad16")
        res.append((dw, work))
    (want, want_work), (got, got_work) = res
    assert not bool(want.isnan().any()) and bool(want.any())
    assert torch.equal(got, want) and torch.equal(got_work, want_work)


# ------------------------------------------------------------------------------------------------ 3. ld_dn_gn_forward_to16
@pytest.mark.parametrize("B,Cc,H,W,ldc,with_film", [(2, 32, 14, 14, 64, True), (3, 64, 7, 7, 64, False)])
def test_gn_forward_to16_is_gn_forward_rounded(B, Cc, H, W, ldc, with_film):
    """out = ld_dn_gn_forward's, cast to bf16 by torch (nearest even); stat equal; the padded channels of a buffer that held
    NaN are zero; with an fp32 residual too."""
    groups, key, lib = 8, 5300 + 10 * Cc + H, cabi.lib()
    y = R.uniform((B, Cc, H, W), key, -2.0, 2.0) + 0.3
    g, b = R.uniform((Cc,), key + 1, 0.5, 1.5).to(DEV), R.uniform((Cc,), key + 2, -0.5, 0.5).to(DEV)
    film = R.uniform((B, 2 * Cc), key + 3, -0.5, 0.5).to(DEV) if with_film else None
    yp = padded(y, ldc)                                                      # (its padding holds NaN: never read)
    nwork = int(lib.ld_dn_gn_work_bytes(B, H, W, Cc)) // 8
    for res in (None, padded(R.uniform((B, Cc, H, W), key + 4), ldc)):
        outs = []
        for fn, dt in ((lib.ld_dn_gn_forward, F32), (lib.ld_dn_gn_forward_to16, BF16)):
            stat, out, work = nans(B, groups, 2), nans(B, H, W, ldc, dtype=dt), nans(nwork, dtype=F64)
            cabi.check(fn(yp.data_ptr(), g.data_ptr(), b.data_ptr(), cabi.ptr(film), cabi.ptr(res), work.data_ptr(), stat.data_ptr(),
                          out.data_ptr(), B, H, W, Cc, ldc, groups, st()), "gn_forward")
            outs.append((out, stat))
        (want, want_stat), (got, got_stat) = outs
        assert normal(want) and bool(want[..., :Cc].any()) and not torch.equal(want.to(BF16).float(), want)
        assert got.dtype == BF16 and torch.equal(got, want.to(BF16))
        assert torch.equal(got_stat, want_stat) and not bool(got_stat.isnan().any())
        if ldc > Cc:
            assert bool((got[..., Cc:] == 0).all())


# ------------------------------------------------------------------------------------------------ 4. ld_dn_pack_nhwc_to16
@pytest.mark.parametrize("view", ["nchw", "non_contiguous"])
def test_pack_nhwc_to16_is_pack_nhwc_rounded(view):
    B, Cc, H, W, ldc = 2, 32, 6, 5, 64
    if view == "nchw":
        x = R.uniform((B, Cc, H, W), 5400).to(DEV)
    else:
        x = R.uniform((B, H + 1, 2 * W, Cc + 8), 5401).to(DEV)[:, 1:, ::2, 3:3 + Cc].permute(0, 3, 1, 2)
        assert not x.is_contiguous()
    assert tuple(x.shape) == (B, Cc, H, W)
    sb, sc, sh, sw = x.stride()
    want, got = nans(B, H, W, ldc), nans(B, H, W, ldc, dtype=BF16)
    cabi.check(cabi.lib().ld_dn_pack_nhwc(x.data_ptr(), want.data_ptr(), B, Cc, H, W, sb, sc, sh, sw, ldc, st()), "pack_nhwc")
    cabi.check(cabi.lib().ld_dn_pack_nhwc_to16(x.data_ptr(), got.data_ptr(), B, Cc, H, W, sb, sc, sh, sw, ldc, st()), "pack_nhwc_to16")
    assert torch.equal(want[..., :Cc], x.permute(0, 2, 3, 1)) and not torch.equal(want.to(BF16).float(), want)
    assert torch.equal(got, want.to(BF16)) and bool((got[..., Cc:] == 0).all())


# ------------------------------------------------------------------------------------------------ 5. ResnetBlock
def forward_backward(blk, x, temb, dout):
    """out, gradients and the bytes autograd keeps for the backward."""
    xd = x.detach().requires_grad_(True)
    td = None if temb is None else temb.detach().requires_grad_(True)
    blk.zero_grad(set_to_none=True)
    out = blk(xd, td)
    saved = out.grad_fn.saved_tensors
    kept = sum(t.numel() * t.element_size() for t in saved)
    dtypes = sorted(str(t.dtype) for t in saved if t.dim() == 4 and t.dtype != F32)
    out.backward(dout)
    grads = {"x": xd.grad}
    if td is not None:
        grads["time_emb"] = td.grad
    grads.update({k: p.grad for k, p in blk.named_parameters() if p.grad is not None})
    return out.detach().clone(), {k: v.detach().clone() for k, v in grads.items()}, kept, dtypes


@pytest.mark.parametrize("B,dim,dim_out,H,W,tdim,channels_last,n16", [
    (2, 32, 64, 6, 5, 32, False, 2),       # res_conv: the copy of x and h1 are bf16
    (2, 32, 32, 5, 3, None, False, 1),     # identity skip with a copy: xp is the fp32 residual, h1 is bf16
    (1, 64, 64, 4, 4, None, True, 1)])     # x read in place: h1 is bf16
def test_resnet_block_keeps_its_bits_and_saves_less(B, dim, dim_out, H, W, tdim, channels_last, n16):
    """At ``conv_precision="bf16"`` with every buffer filled with NaN first: output and every gradient at
    ``act_storage="bf16"`` equal those at ``"fp32"``, autograd keeps B H W 64 2 bytes less per bf16 tensor, and setting the
    attribute back restores fp32 saved tensors."""
    sd = R.make_block(dim, dim_out, tdim, key=dim + dim_out + 1)
    x = R.uniform((B, dim, H, W), 5500 + dim + H).to(DEV)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    temb = None if tdim is None else R.uniform((B, tdim), 5501 + dim).to(DEV)
    dout = (R.uniform((B, dim_out, H, W), 5502 + dim) / (B * H * W)).to(DEV)
    blk = ldh.ResnetBlock(dim, dim_out, time_emb_dim=tdim)
    blk.load_state_dict(sd)
    blk = blk.to(DEV)
    blk.debug_fill = NAN
    blk.conv_precision = "bf16"
    out32, g32, kept32, dt32 = forward_backward(blk, x, temb, dout)
    packed = blk._packed
    blk.act_storage = "bf16"
    out16, g16, kept16, dt16 = forward_backward(blk, x, temb, dout)
    assert blk._packed is packed                                            # the weights were not packed again
    assert dt32 == [] and dt16 == ["torch.bfloat16"] * n16
    assert kept32 - kept16 == n16 * B * H * W * 64 * 2, (kept32, kept16)
    assert bool(torch.isfinite(out32).all()) and bool(out32.any())
    assert torch.equal(out16, out32)
    assert set(g16) == set(g32) and len(g32) >= 9
    for k in g32:
        assert bool(torch.isfinite(g32[k]).all()) and bool(g32[k].any()), k
        assert torch.equal(g16[k], g32[k]), k
    with torch.no_grad():                                                   # the path that keeps nothing
        assert torch.equal(blk(x, temb), out32)
    blk.act_storage = "fp32"
    out_b, g_b, kept_b, dt_b = forward_backward(blk, x, temb, dout)
    assert kept_b == kept32 and dt_b == [] and torch.equal(out_b, out32)
    for k in g32:
        assert torch.equal(g_b[k], g32[k]), k


def test_a_bf16_activation_at_fp32_convolutions_is_refused():
    """``Run.conv`` and ``Run.wgrad_packed`` pick the entry point from the activation's dtype; at ``conv_precision="fp32"`` a
    bf16 activation is a ``RuntimeError`` before any launch."""
    blk = ldh.ResnetBlock(64, 64).to(DEV)
    x = torch.zeros(1, 64, 4, 4, device=DEV)
    run = blk._run(x)
    a16, dy = torch.zeros(1, 4, 4, 64, dtype=BF16, device=DEV), torch.zeros(1, 4, 4, 64, device=DEV)
    with pytest.raises(RuntimeError, match="bfloat16 activation at conv_precision 'fp32'"):
        run.conv(a16, run.p.w1f, run.p.b1, 64, 64, 3)
    with pytest.raises(RuntimeError, match="bfloat16 activation at conv_precision 'fp32'"):
        run.wgrad_packed(dy, a16, 64, 64, 3)
    assert run.nhwc(x, 64, 64, dtype=BF16).dtype == BF16                    # (NCHW: a copy, in the dtype asked for)
    xl = x.contiguous(memory_format=torch.channels_last)
    assert run.nhwc(xl, 64, 64, dtype=BF16) is xl                           # read in place: stays what it is


# ------------------------------------------------------------------------------------------------ 6. the whole net
OPTS = dict(branch_out=False, start_intermediate=False, start_timestep=2, mask_x=False, ood_AD=False, ood_confidence=False,
            classifier=False, use_gt=False, data="mnist")
NB, SIZE, TIMESTEPS = 2, 28, 250


def make_trainer(**kw):
    inf = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **UR.KWARGS["mnist"])
    inf.load_state_dict(UR.state("mnist"))
    gd = ldh.GaussianDiffusion(OPTS, inf, image_size=SIZE, timesteps=TIMESTEPS, objective="pred_v").to(DEV)
    return ldh.DenoiserTrainer(gd, train_lr=1e-3, **kw)


def test_trainer_with_bf16_storage_holds_the_bf16_trainers_bits():
    """After one ``accumulate`` + ``apply``: the loss, the flat gradient (before ``apply``) and the parameters at
    ``conv_precision="bf16", act_storage="bf16"`` are those of ``conv_precision="bf16"`` alone, bit for bit."""
    hr, lr = R.uniform((NB, 1, SIZE, SIZE), 3400, 0.0, 1.0).to(DEV), R.uniform((NB, 1, SIZE, SIZE), 3401, 0.0, 1.0).to(DEV)
    t, noise = torch.tensor([3, 200], device=DEV), R.uniform((NB, 1, SIZE, SIZE), 3402, -1.7, 1.7).to(DEV)
    seen = []
    for storage in ("fp32", "bf16"):
        tr = make_trainer(conv_precision="bf16", act_storage=storage)
        assert tr.act_storage == storage and tr.online_model.act_storage == storage
        tr.online_model.debug_fill = NAN
        for m in tr.online_model.modules():
            if isinstance(m, TrainableModule):
                assert m.act_storage == (storage if isinstance(m, ldh.ResnetBlock) else "fp32")
        loss = tr.accumulate(hr, lr, t=t, noise=noise)
        grad = torch.cat([p.grad.reshape(-1) for p in tr.online_model.parameters() if p.grad is not None]).clone()
        tr.apply()
        tr.check_finite()
        params = torch.cat([p.detach().reshape(-1) for p in tr.online_model.parameters()]).clone()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and bool(grad.any())
        seen.append((loss.clone(), grad, params))
    for a, b in zip(*seen):
        assert torch.equal(a, b)
