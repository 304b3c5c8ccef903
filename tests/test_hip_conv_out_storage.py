"""GPU tests of ``conv_out_storage="bf16"``: the five entry points that write or read a bf16 convolution output
(csrc/conv16.hip, csrc/denoiser_grad.hip) against the fp32 ones, then ``ResnetBlock`` and ``DenoiserTrainer`` with the switch
against themselves without it but with the same rounding applied by torch.  A convolution's ``_to16`` launch is the fp32
launch rounded to nearest even, and a bf16 widens to fp32 exactly, so every comparison is HIP against HIP and ``torch.equal``.
Every output buffer holds NaN first."""
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


def is_tie(t):
    """The fp32 values that lie exactly between two bf16 values: the low half of the pattern is 0x8000."""
    return (t.contiguous().view(torch.int32) & 0xFFFF) == 0x8000


# ------------------------------------------------------------------------------------------------ 1. the convolutions
def ohwi_bf16(w):
    return w.permute(0, 2, 3, 1).contiguous().to(DEV, BF16).reshape(-1)


def conv16_all(src, wb, shift, residual, cin, cout, k):
    """ld_dn_conv16 on ``src`` [B, H, W, cin] (fp32, device), then ld_dn_conv16_to16 on it and ld_dn_conv16_from16_to16 on
    ``src.to(bfloat16)``: (fp32 out, [bf16 out, bf16 out])."""
    B, H, W, _ = src.shape
    lib = cabi.lib()
    ones, sh = torch.ones(cout, device=DEV), shift.to(DEV, F32)
    src16 = src.to(BF16)
    outs = []
    for fn, s, dt in ((lib.ld_dn_conv16, src, F32), (lib.ld_dn_conv16_to16, src, BF16), (lib.ld_dn_conv16_from16_to16, src16, BF16)):
        out = nans(B, H, W, cout, dtype=dt)
        a = cabi.PcConvArgs()
        a.src, a.weight, a.scale, a.shift, a.residual, a.out = s.data_ptr(), None, ones.data_ptr(), sh.data_ptr(), cabi.ptr(residual), out.data_ptr()
        a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout, a.ksize, a.stride, a.relu = B, H, W, cin, H, W, cout, k, 1, 0
        cabi.check(fn(C.byref(a), wb.data_ptr(), st()), "conv16")
        outs.append(out)
    return outs[0], outs[1:]


@pytest.mark.parametrize("shape", P.CONV_SHAPES)
@pytest.mark.parametrize("kind", ["ints", "uniform"])
def test_conv16_to16_is_conv16_rounded(shape, kind):
    """A partial pixel tile, the seam between two images, ksize 1 and the shift + fp32 residual epilogue.  On the integer
    operands every sum is exact in fp32, so the expected tensor holds exact ties of the bf16 rounding: the elements that
    tell round-to-nearest-even from any other rounding."""
    B, cin, cout, H, W, k = shape
    assert P.CONV_WITH_EPILOGUE in P.CONV_SHAPES
    epi = shape == P.CONV_WITH_EPILOGUE
    key = 8200 + cin + H
    if kind == "ints":
        x, w = P.ints((B, cin, H, W), key, -32, 32).float(), P.trits((cout, cin, k, k), key + 1).float()
        shift = P.ints((cout,), key + 2, -4, 4).float() if epi else torch.zeros(cout)
        res = padded(P.ints((B, cout, H, W), key + 3, -4, 4).float(), cout) if epi else None
    else:
        x, w = R.uniform((B, cin, H, W), key + 4), R.uniform((cout, cin, k, k), key + 5)
        shift = R.uniform((cout,), key + 6) if epi else torch.zeros(cout)
        res = padded(R.uniform((B, cout, H, W), key + 7), cout) if epi else None
    want, gots = conv16_all(padded(x, cin), ohwi_bf16(w), shift, res, cin, cout, k)
    assert bool(torch.isfinite(want).all()) and bool(want.any()) and not torch.equal(want.to(BF16).float(), want)
    if kind == "ints":
        ref = P.conv_ref(x, w, shift, None if res is None else res.permute(0, 3, 1, 2).cpu())
        assert torch.equal(want.permute(0, 3, 1, 2).cpu(), ref)             # exact sums: the fp32 launch gives the integers
        assert int(is_tie(want).sum()) > 0
    for got in gots:
        assert got.dtype == BF16 and torch.equal(got, want.to(BF16))


@pytest.mark.parametrize("kind", ["ints", "uniform"])
def test_conv16_to16_writes_zeros_into_padded_channels(kind):
    """Cout 32 padded to 64 through ld_dn_pack_conv16: the padded output channels of a buffer that held NaN are zero."""
    B, cin, cout, H, W, k = P.DGRAD_SHAPE
    cop, cip = pad64(cout), pad64(cin)
    if kind == "ints":
        x, w = P.ints((B, cin, H, W), 8300, -32, 32).float(), P.trits((cout, cin, k, k), 8301).float()
    else:
        x, w = R.uniform((B, cin, H, W), 8302), R.uniform((cout, cin, k, k), 8303)
    wd = w.to(DEV).contiguous()
    fwd, dgr = nans(cop * k * k * cip, dtype=BF16), nans(cip * k * k * cop, dtype=BF16)
    cabi.check(cabi.lib().ld_dn_pack_conv16(wd.data_ptr(), fwd.data_ptr(), dgr.data_ptr(), cout, cop, cin, cip, k, st()), "dn_pack_conv16")
    want, gots = conv16_all(padded(x, cip, fill=0.0), fwd, torch.zeros(cop), None, cip, cop, k)
    assert bool(torch.isfinite(want).all()) and bool(want[..., :cout].any())
    for got in gots:
        assert torch.equal(got, want.to(BF16)) and bool((got[..., cout:] == 0).all())


# ------------------------------------------------------------------------------------------------ 2. GroupNorm forward
GN_CASES = [(2, 32, 14, 14, 64, True), (3, 64, 7, 7, 64, False)]


def gn_operands(B, Cc, H, W, ldc, with_film, key):
    y = R.uniform((B, Cc, H, W), key, -2.0, 2.0) + 0.3
    g, b = R.uniform((Cc,), key + 1, 0.5, 1.5).to(DEV), R.uniform((Cc,), key + 2, -0.5, 0.5).to(DEV)
    film = R.uniform((B, 2 * Cc), key + 3, -0.5, 0.5).to(DEV) if with_film else None
    y16 = padded(y, ldc).to(BF16)                                            # (its padding holds NaN: never read)
    y32 = y16.float()
    assert not torch.equal(y32[..., :Cc], padded(y, ldc)[..., :Cc]) and bool(y16[..., Cc:].isnan().all())
    return y16, y32, g, b, film


@pytest.mark.parametrize("B,Cc,H,W,ldc,with_film", GN_CASES)
def test_gn_forward_from16_is_gn_forward_on_the_widened_tensor(B, Cc, H, W, ldc, with_film):
    """out and stat of the two ``_from16`` entry points on ``y16`` equal those of the fp32 ones on ``y16.float()``, with and
    without an fp32 residual; the padded outputs are zero."""
    groups, key, lib = 8, 8400 + 10 * Cc + H, cabi.lib()
    y16, y32, g, b, film = gn_operands(B, Cc, H, W, ldc, with_film, key)
    nwork = int(lib.ld_dn_gn_work_bytes(B, H, W, Cc)) // 8
    for res in (None, padded(R.uniform((B, Cc, H, W), key + 4), ldc)):
        for dt, ref_fn, fn in ((F32, lib.ld_dn_gn_forward, lib.ld_dn_gn_forward_from16),
                               (BF16, lib.ld_dn_gn_forward_to16, lib.ld_dn_gn_forward_from16_to16)):
            seen = []
            for f, y in ((ref_fn, y32), (fn, y16)):
                stat, out, work = nans(B, groups, 2), nans(B, H, W, ldc, dtype=dt), nans(nwork, dtype=F64)
                cabi.check(f(y.data_ptr(), g.data_ptr(), b.data_ptr(), cabi.ptr(film), cabi.ptr(res), work.data_ptr(), stat.data_ptr(),
                             out.data_ptr(), B, H, W, Cc, ldc, groups, st()), "gn_forward")
                seen.append((out, stat))
            (want, want_stat), (got, got_stat) = seen
            assert bool(torch.isfinite(want.float()).all()) and bool(want[..., :Cc].any())
            assert got.dtype == dt and torch.equal(got, want)
            assert torch.equal(got_stat, want_stat) and bool(torch.isfinite(got_stat).all())
            if ldc > Cc:
                assert bool((got[..., Cc:] == 0).all())


# ------------------------------------------------------------------------------------------------ 3. GroupNorm backward
@pytest.mark.parametrize("B,Cc,H,W,ldc,with_film", GN_CASES)
@pytest.mark.parametrize("in_place", [False, True])
def test_gn_backward_from16_is_gn_backward_on_the_widened_tensor(B, Cc, H, W, ldc, with_film, in_place):
    """dgamma, dbeta, dfilm and dy; once with a dy of its own and once with dy aliasing dout (what block1 does)."""
    groups, key, lib = 8, 8500 + 10 * Cc + H, cabi.lib()
    y16, y32, g, b, film = gn_operands(B, Cc, H, W, ldc, with_film, key)
    nwork = int(lib.ld_dn_gn_work_bytes(B, H, W, Cc)) // 8
    stat, out, work = nans(B, groups, 2), nans(B, H, W, ldc), nans(nwork, dtype=F64)
    cabi.check(lib.ld_dn_gn_forward(y32.data_ptr(), g.data_ptr(), b.data_ptr(), cabi.ptr(film), None, work.data_ptr(), stat.data_ptr(),
                                    out.data_ptr(), B, H, W, Cc, ldc, groups, st()), "gn_forward")
    dout = padded(R.uniform((B, Cc, H, W), key + 5) / (B * H * W), ldc)      # (its padding holds NaN: never read)
    seen = []
    for fn, y in ((lib.ld_dn_gn_backward, y32), (lib.ld_dn_gn_backward_from16, y16)):
        d = dout.clone()
        dy = d if in_place else nans(B, H, W, ldc)
        dg, db, work = nans(Cc), nans(Cc), nans(nwork, dtype=F64)
        dfilm = nans(B, 2 * Cc) if with_film else None
        cabi.check(fn(d.data_ptr(), y.data_ptr(), stat.data_ptr(), g.data_ptr(), b.data_ptr(), cabi.ptr(film), work.data_ptr(),
                      dg.data_ptr(), db.data_ptr(), cabi.ptr(dfilm), dy.data_ptr(), B, H, W, Cc, ldc, groups, st()), "gn_backward")
        seen.append([dg, db, dy] + ([dfilm] if with_film else []))
    want, got = seen
    for w_, g_ in zip(want, got):
        assert bool(torch.isfinite(w_).all()) and bool(w_.any())
        assert torch.equal(g_, w_)
    if ldc > Cc:
        assert bool((got[2][..., Cc:] == 0).all())


# ------------------------------------------------------------------------------------------------ 4. ResnetBlock
class RoundingRun(ldh.ResnetBlock.Run):
    """The block's launches at ``conv_out_storage="fp32"`` with the outputs of the two 3x3 convolutions of ``forward`` rounded
    to bf16 by torch and widened again: what the switch computes, in fp32 storage.  ``backward`` is untouched."""

    in_forward = False

    def forward(self, x, temb, keep=True):
        self.in_forward = True
        try:
            return super().forward(x, temb, keep=keep)
        finally:
            self.in_forward = False

    def conv(self, src, weight, shift, cin, cout, k, **kw):
        out = super().conv(src, weight, shift, cin, cout, k, **kw)
        return out.to(BF16).float() if self.in_forward and k == 3 else out


def forward_backward(blk, x, temb, dout):
    """out, gradients, the bytes autograd keeps for the backward and the dtypes of its 4-D tensors that are not fp32."""
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


@pytest.mark.parametrize("B,dim,dim_out,H,W,tdim,channels_last", [
    (2, 32, 64, 6, 5, 32, False),          # res_conv (its fp32 output is the second GroupNorm's residual and output), FiLM
    (2, 32, 32, 5, 3, None, False),        # identity skip with a copy
    (1, 64, 64, 4, 4, None, True)])        # x read in place
@pytest.mark.parametrize("act", ["fp32", "bf16"])
def test_resnet_block_computes_the_rounded_forward_and_its_exact_gradient(B, dim, dim_out, H, W, tdim, channels_last, act):
    """At ``conv_precision="bf16"`` with every buffer filled with NaN first: output, every gradient and the ``no_grad`` result
    at ``conv_out_storage="bf16"`` are those of the same block at ``"fp32"`` under ``RoundingRun``; autograd keeps 2 B H W cop
    2 bytes less, in two more bf16 tensors; setting the switch back restores the fp32 bits without repacking; and the output
    differs from the unrounded one inside the project's window for one bf16 rounding of a block.

    rel_err(out at "bf16", out at "fp32") measured on the MI355X (the CPU restatement gives 3.2e-3 ... 6.4e-3):
    32 -> 64 @ 6 x 5: 3.785e-3; 32 -> 32 @ 5 x 3: 3.340e-3; 64 -> 64 @ 4 x 4: 2.913e-3 (the same at either ``act_storage``)."""
    sd = R.make_block(dim, dim_out, tdim, key=dim + dim_out + 1)
    x = R.uniform((B, dim, H, W), 8600 + dim + H).to(DEV)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    temb = None if tdim is None else R.uniform((B, tdim), 8601 + dim).to(DEV)
    dout = (R.uniform((B, dim_out, H, W), 8602 + dim) / (B * H * W)).to(DEV)
    blk = ldh.ResnetBlock(dim, dim_out, time_emb_dim=tdim)
    blk.load_state_dict(sd)
    blk = blk.to(DEV)
    blk.debug_fill = NAN
    blk.conv_precision, blk.act_storage = "bf16", act
    out32, g32, kept32, dt32 = forward_backward(blk, x, temb, dout)          # the switch off: the unrounded block
    packed = blk._packed
    blk.Run = RoundingRun                                                    # (on the instance)
    want, gwant, kept_r, dt_r = forward_backward(blk, x, temb, dout)
    with torch.no_grad():
        assert torch.equal(blk(x, temb), want)
    del blk.Run
    assert blk.Run is ldh.ResnetBlock.Run and kept_r == kept32 and dt_r == dt32
    blk.conv_out_storage = "bf16"
    out16, g16, kept16, dt16 = forward_backward(blk, x, temb, dout)
    assert blk._packed is packed                                            # the weights were not packed again
    assert dt16 == dt32 + ["torch.bfloat16"] * 2
    assert kept32 - kept16 == 2 * B * H * W * pad64(dim_out) * 2, (kept32, kept16)
    assert bool(torch.isfinite(want).all()) and bool(want.any())
    assert torch.equal(out16, want)
    assert set(g16) == set(gwant) and len(gwant) >= 9
    for k in gwant:
        assert bool(torch.isfinite(gwant[k]).all()) and bool(gwant[k].any()), k
        assert torch.equal(g16[k], gwant[k]), k
    with torch.no_grad():                                                   # the path that keeps nothing
        assert torch.equal(blk(x, temb), want)
    # the switch is wired: one more bf16 rounding of the block's intermediates
    err = R.rel_err(out16, out32)
    print(f"{dim} -> {dim_out} @ {H} x {W}, act_storage {act}: rel_err(out at bf16, out at fp32) = {err:.3e}")
    assert not torch.equal(out16, out32)
    assert 1e-5 < err < 2e-2, err
    blk.conv_out_storage = "fp32"
    out_b, g_b, kept_b, dt_b = forward_backward(blk, x, temb, dout)
    assert blk._packed is packed and kept_b == kept32 and dt_b == dt32 and torch.equal(out_b, out32)
    for k in g32:
        assert torch.equal(g_b[k], g32[k]), k


def test_a_bf16_output_at_fp32_convolutions_is_refused():
    """``Run.conv`` routes on (the source's dtype, ``out_dtype``); at ``conv_precision="fp32"`` a bf16 ``out_dtype`` is a
    ``RuntimeError`` before any launch."""
    blk = ldh.ResnetBlock(64, 64).to(DEV)
    x = torch.zeros(1, 64, 4, 4, device=DEV)
    run = blk._run(x)
    with pytest.raises(RuntimeError, match="bfloat16 convolution output at conv_precision 'fp32'"):
        run.conv(torch.zeros(1, 4, 4, 64, device=DEV), run.p.w1f, run.p.b1, 64, 64, 3, out_dtype=BF16)
    blk.conv_precision = "bf16"
    run = blk._run(x)
    for src_dt in (F32, BF16):
        y = run.conv(torch.zeros(1, 4, 4, 64, dtype=src_dt, device=DEV), run.p.w1f, run.p.b1, 64, 64, 3, out_dtype=BF16)
        assert y.dtype == BF16 and tuple(y.shape) == (1, 4, 4, 64)


# ------------------------------------------------------------------------------------------------ 5. the whole net
OPTS = dict(branch_out=False, start_intermediate=False, start_timestep=2, mask_x=False, ood_AD=False, ood_confidence=False,
            classifier=False, use_gt=False, data="mnist")
NB, SIZE, TIMESTEPS = 2, 28, 250


def make_trainer(**kw):
    inf = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **UR.KWARGS["mnist"])
    inf.load_state_dict(UR.state("mnist"))
    gd = ldh.GaussianDiffusion(OPTS, inf, image_size=SIZE, timesteps=TIMESTEPS, objective="pred_v").to(DEV)
    return ldh.DenoiserTrainer(gd, train_lr=1e-3, conv_precision="bf16", act_storage="bf16", **kw)


def test_trainer_with_bf16_conv_outputs_takes_the_rounded_step():
    """After one ``accumulate`` + ``apply`` at ``conv_precision="bf16", act_storage="bf16", conv_out_storage="bf16"``: the loss,
    the flat gradient (before ``apply``) and the parameters are, bit for bit, those of a trainer at ``conv_out_storage="fp32"``
    whose ``ResnetBlock``s carry ``RoundingRun``; a second trainer built alike with NaN-filled buffers gives the same bits;
    everything is finite; only ``ResnetBlock``s report ``"bf16"``; and the loss differs from the unrounded trainer's.

    On the MI355X: loss 1.0902352 at ``conv_out_storage="bf16"``, 1.0894781 at ``"fp32"``."""
    hr, lr = R.uniform((NB, 1, SIZE, SIZE), 3400, 0.0, 1.0).to(DEV), R.uniform((NB, 1, SIZE, SIZE), 3401, 0.0, 1.0).to(DEV)
    t, noise = torch.tensor([3, 200], device=DEV), R.uniform((NB, 1, SIZE, SIZE), 3402, -1.7, 1.7).to(DEV)
    seen = {}
    for what, storage, fill in (("plain", "fp32", NAN), ("want", "fp32", NAN), ("got", "bf16", None), ("again", "bf16", NAN)):
        tr = make_trainer(conv_out_storage=storage)
        assert tr.conv_out_storage == storage and tr.online_model.conv_out_storage == storage and tr.act_storage == "bf16"
        tr.online_model.debug_fill = fill
        for m in tr.online_model.modules():
            if isinstance(m, TrainableModule):
                assert m.conv_out_storage == (storage if isinstance(m, ldh.ResnetBlock) else "fp32")
            if what == "want" and isinstance(m, ldh.ResnetBlock):
                m.Run = RoundingRun
        loss = tr.accumulate(hr, lr, t=t, noise=noise)
        grad = torch.cat([p.grad.reshape(-1) for p in tr.online_model.parameters() if p.grad is not None]).clone()
        tr.apply()
        tr.check_finite()
        params = torch.cat([p.detach().reshape(-1) for p in tr.online_model.parameters()]).clone()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and bool(grad.any())
        assert bool(torch.isfinite(params).all())
        seen[what] = (loss.clone(), grad, params)
    print(f"loss at conv_out_storage bf16: {float(seen['got'][0]):.7f}, at fp32: {float(seen['plain'][0]):.7f}")
    for other in ("got", "again"):
        for a, b in zip(seen["want"], seen[other]):
            assert torch.equal(a, b), other
    assert not torch.equal(seen["got"][0], seen["plain"][0])
