"""GPU tests of mixed-precision training (``amp``): the fp16 forms of csrc/conv16.hip one by one -- bit for bit on the exact
probes of tests/amp_ref.py, which a launch routed to the bf16 kernel cannot pass, and on uniform operands against the fp64
value of the fp16-ROUNDED operands within the worst-case bound of a K-term fp32 sum (tests/test_hip_conv16.py's rule) --, the
loss scaler's kernels of csrc/denoiser_opt.hip on the synthetic table of tests/test_hip_denoiser_train.py, and
``DenoiserTrainer(amp=True)`` against the real ``torch.amp.GradScaler`` on the CPU.  Every output buffer holds NaN first."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd.denoiser_train import SCALER_KEYS, EmulatedRank
from localdiffusion_hallucination_amd.trainable import TrainableModule

from hip_helpers import DEV, NAN, nans, pad64, padded, st, unpadded
import amp_ref as A
import conv16_ref as P
import denoiser_train_ref as T
import unet_grad_ref as R

pytestmark = pytest.mark.gpu

F32, F64, F16 = torch.float32, torch.float64, torch.float16
INF = float("inf")


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int64)


def normal_uniform(shape, key):
    """Uniform in [-1, 1] with the magnitude kept at 2^-10 or more: fp16 normals (its subnormals begin below 2^-14)."""
    u = R.uniform(shape, key)
    return torch.where(u.abs() < 2.0 ** -10, torch.full_like(u, 2.0 ** -10), u)


# ------------------------------------------------------------------------------------------------ kernel wrappers
def ohwi_f16(w):
    """OIHW fp32 (cpu) -> the forward kernel layout [Cout][k][k][Cin] in fp16 on the device (torch's rounding)."""
    return w.permute(0, 2, 3, 1).contiguous().to(DEV, F16).reshape(-1)


def hip_conv_f16(src, wh, shift, residual, cin, cout, k, relu=0):
    B, H, W, _ = src.shape
    out = nans(B, H, W, cout)
    ones, sh = torch.ones(cout, device=DEV), shift.to(DEV, F32)
    a = cabi.PcConvArgs()
    a.src, a.weight, a.scale, a.shift, a.residual, a.out = src.data_ptr(), None, ones.data_ptr(), sh.data_ptr(), cabi.ptr(residual), out.data_ptr()
    a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout, a.ksize, a.stride, a.relu = B, H, W, cin, H, W, cout, k, 1, relu
    cabi.check(cabi.lib().ld_dn_conv_f16(C.byref(a), wh.data_ptr(), st()), "dn_conv_f16")
    return out


def hip_pack_f16(w, cop, cip):
    co, ci, k, _ = w.shape
    wd = w.to(DEV).contiguous()
    fwd, dgr = nans(cop * k * k * cip, dtype=F16), nans(cip * k * k * cop, dtype=F16)
    cabi.check(cabi.lib().ld_dn_pack_conv_f16(wd.data_ptr(), fwd.data_ptr(), dgr.data_ptr(), co, cop, ci, cip, k, st()), "dn_pack_conv_f16")
    return fwd, dgr


def hip_wgrad_f16(dy, a, shape, splits):
    B, cin, cout, H, W, k = shape
    lib = cabi.lib()
    auto = int(lib.ld_seg_wgrad_splits(B, H, W, cin, cout, k))
    assert auto >= 1
    splits = auto if splits is None else splits
    n = cout * k * k * cin
    work, dw = nans(splits * n), nans(n)
    dyp, ap = padded(dy, cout), padded(a, cin)                          # (kept alive past the launch)
    cabi.check(lib.ld_dn_wgrad_f16(dyp.data_ptr(), ap.data_ptr(), work.data_ptr(), dw.data_ptr(), B, H, W, cin, cout, k, splits, st()),
               "dn_wgrad_f16")
    return dw.view(cout, k, k, cin).permute(0, 3, 1, 2).contiguous().cpu(), splits, work.view(splits, n).cpu()


def within(got, ref64, bound, what):
    err = (got.double() - ref64).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: largest error / bound {ratio:.3f} (max error {float(err.max()):.2e})")
    assert bool((err <= bound).all()), (what, ratio)


# ------------------------------------------------------------------------------------------------ 1. the three kernels
@pytest.mark.parametrize("shape", P.CONV_SHAPES)
@pytest.mark.parametrize("kind", ["identity", "rounding"])
def test_conv_f16_exact(shape, kind):
    """Bit for bit: integers that fp16 holds and bf16 does not come through untouched, fp16 ties go to the even neighbour."""
    B, cin, cout, H, W, k = shape
    p = A.conv_probe(shape, kind, epilogue=shape == P.CONV_WITH_EPILOGUE)
    res = None if p.res is None else padded(p.res, cout)
    out = hip_conv_f16(padded(p.x, cin), ohwi_f16(p.w), p.shift, res, cin, cout, k)
    assert torch.equal(unpadded(out, cout), p.ref)


@pytest.mark.parametrize("shape", P.CONV_SHAPES)
def test_conv_f16_random(shape):
    """Uniform operands of fp16-normal magnitude: within (K + 4) 2^-23 (|h(x)| * |h(w)| + |shift| + |residual|) of the fp64
    value of the fp16-rounded operands, K = k^2 Cin.  ReLU on the epilogue case."""
    B, cin, cout, H, W, k = shape
    epi = shape == P.CONV_WITH_EPILOGUE
    x, w = normal_uniform((B, cin, H, W), 4000 + cin + H), normal_uniform((cout, cin, k, k), 4001 + cin + H)
    shift = R.uniform((cout,), 4002 + cin) if epi else torch.zeros(cout)
    res = R.uniform((B, cout, H, W), 4003 + cin) if epi else None
    out = hip_conv_f16(padded(x, cin), ohwi_f16(w), shift, None if res is None else padded(res, cout), cin, cout, k)
    ref64 = P.conv_ref(x, w, shift, res, F64, A.h)
    mag = P.conv_ref(x.abs(), w.abs(), shift.abs(), None if res is None else res.abs(), F64, A.h)
    within(unpadded(out, cout), ref64, P.sum_bound(k * k * cin, mag), f"conv_f16 {shape}")
    assert not torch.equal(ref64, P.conv_ref(x, w, shift, res, F64))         # (the bf16 yardstick is another number)
    if epi:
        relu = hip_conv_f16(padded(x, cin), ohwi_f16(w), shift, padded(res, cout), cin, cout, k, relu=1)
        assert torch.equal(relu, out.clamp_min(0.0)) and bool((out < 0).any())


@pytest.mark.parametrize("kind", ["identity_w", "rounding_w", "identity_dy", "rounding_dy", "random"])
def test_conv_f16_as_the_data_gradient_on_the_packed_weight(kind):
    """(Cin 64, Cout 32 padded to 64) on ld_dn_pack_conv_f16's data-gradient layout: the transposed convolution."""
    B, cin, cout, H, W, k = P.DGRAD_SHAPE
    cop, cip = pad64(cout), pad64(cin)
    if kind == "random":
        dy, w = normal_uniform((B, cout, H, W), 4100), normal_uniform((cout, cin, k, k), 4101)
    else:
        p = A.dgrad_probe(P.DGRAD_SHAPE, kind)
        dy, w = p.dy, p.w
    _, dgr = hip_pack_f16(w, cop, cip)
    out = unpadded(hip_conv_f16(padded(dy, cop, fill=0.0), dgr, torch.zeros(cip), None, cop, cip, k), cin)
    if kind == "random":
        bound = P.sum_bound(k * k * cout, P.dgrad_ref(dy.abs(), w.abs(), F64, A.h))
        within(out, P.dgrad_ref(dy, w, F64, A.h), bound, f"conv_f16 data gradient {P.DGRAD_SHAPE}")
    else:
        assert torch.equal(out, p.ref)


@pytest.mark.parametrize("shape,splits", P.WGRAD_CASES)
@pytest.mark.parametrize("kind", ["identity_dy", "rounding_dy", "identity_a", "rounding_a"])
def test_wgrad_f16_exact(shape, splits, kind):
    """Bit for bit; the hand-picked split count leaves the last split without a chunk: its slab is written as zeros."""
    B, cin, cout, H, W, k = shape
    p = A.wgrad_probe(shape, kind)
    dw, used, work = hip_wgrad_f16(p.dy, p.a, shape, splits)
    assert torch.equal(dw, p.ref)
    if splits is not None:
        nchunks = (B * H * W + 31) // 32
        per = (nchunks + used - 1) // used
        assert used < int(cabi.lib().ld_seg_wgrad_splits(B, H, W, cin, cout, k)) and per * (used - 1) >= nchunks
        assert not bool(work[-1].any()) and bool(work[0].any())


@pytest.mark.parametrize("shape,splits", P.WGRAD_CASES)
def test_wgrad_f16_random(shape, splits):
    """Within (K + 4) 2^-23 (|h(dy)| * |h(a)|) of the fp64 value of the fp16-rounded operands, K = B H W."""
    B, cin, cout, H, W, k = shape
    dy, a = normal_uniform((B, cout, H, W), 4200 + cin + k), normal_uniform((B, cin, H, W), 4201 + cin + k)
    dw, _, _ = hip_wgrad_f16(dy, a, shape, splits)
    within(dw, P.wgrad_ref(dy, a, k, F64, A.h), P.sum_bound(B * H * W, P.wgrad_ref(dy.abs(), a.abs(), k, F64, A.h)),
           f"wgrad_f16 {shape} splits {splits}")


@pytest.mark.parametrize("shape", P.PACK_SHAPES)
def test_pack_conv_f16(shape):
    """Both layouts bit for bit against h(w) permuted in torch, the padded channels zero; NaN and inf are kept; a weight
    beyond 65504 becomes inf."""
    p = A.pack_probe(shape)
    fwd, dgr = hip_pack_f16(p.w, p.cop, p.cip)
    assert fwd.dtype == F16 and torch.equal(fwd.float().cpu(), p.fwd) and torch.equal(dgr.float().cpu(), p.dgr)
    w = normal_uniform(tuple(p.w.shape), 4300)
    fwd, dgr = hip_pack_f16(w, p.cop, p.cip)
    want_f, want_d = P.pack_ref(A.h(w), p.cop, p.cip)
    assert torch.equal(fwd.float().cpu(), want_f) and torch.equal(dgr.float().cpu(), want_d)
    w[0, 0, 0, 0], w[1, 0, 0, 0] = NAN, 1e5
    fwd, dgr = hip_pack_f16(w, p.cop, p.cip)
    assert int(fwd.isnan().sum()) == 1 and int(dgr.isnan().sum()) == 1 and int(fwd.isinf().sum()) == 1 and int(dgr.isinf().sum()) == 1


def test_kernel_refusals_use_the_bf16_twins_words():
    """A refused call returns -1 with the bf16 entry point's text under the new name, and writes nothing."""
    lib = cabi.lib()
    src, out, w = nans(1, 4, 4, 32), nans(1, 4, 4, 64), torch.zeros(64 * 9 * 32, dtype=F16, device=DEV)
    ones = torch.ones(64, device=DEV)

    def conv(fn, wp, **kw):
        a = cabi.PcConvArgs()
        a.src, a.scale, a.shift, a.out = src.data_ptr(), ones.data_ptr(), ones.data_ptr(), out.data_ptr()
        a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout, a.ksize, a.stride, a.relu = 1, 4, 4, 32, 4, 4, 64, 3, 1, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return fn(C.byref(a), wp, st()), lib.ld_last_error().decode()
    for kw, wp in ((dict(ksize=5), w.data_ptr()), (dict(Cin=48), w.data_ptr()), (dict(Cout=32), w.data_ptr()), (dict(stride=2), w.data_ptr()),
                   (dict(), None), (dict(), w.data_ptr() + 2), (dict(src=src.data_ptr() + 4), w.data_ptr())):
        (r16, e16), (rf, ef) = conv(lib.ld_dn_conv16, wp, **kw), conv(lib.ld_dn_conv_f16, wp, **kw)
        assert r16 == rf == -1 and ef == e16.replace("ld_dn_conv16", "ld_dn_conv_f16") and ef.startswith("ld_dn_conv_f16:"), (kw, ef)
    dy = nans(1, 4, 4, 64)
    work, dw = nans(64 * 9 * 64), nans(64 * 9 * 64)
    for args in ((1, 4, 4, 32, 64, 3, 1), (1, 4, 4, 64, 64, 3, 2), (1, 4, 4, 64, 64, 2, 1)):
        r16 = lib.ld_dn_wgrad16(dy.data_ptr(), dy.data_ptr(), work.data_ptr(), dw.data_ptr(), *args, st())
        e16 = lib.ld_last_error().decode()
        rf = lib.ld_dn_wgrad_f16(dy.data_ptr(), dy.data_ptr(), work.data_ptr(), dw.data_ptr(), *args, st())
        assert r16 == rf == -1 and lib.ld_last_error().decode() == e16.replace("ld_dn_wgrad16", "ld_dn_wgrad_f16"), args
    r16 = lib.ld_dn_pack_conv16(src.data_ptr(), w.data_ptr(), w.data_ptr(), 20, 63, 3, 64, 3, st())
    e16 = lib.ld_last_error().decode()
    rf = lib.ld_dn_pack_conv_f16(src.data_ptr(), w.data_ptr(), w.data_ptr(), 20, 63, 3, 64, 3, st())
    assert r16 == rf == -1 and lib.ld_last_error().decode() == e16.replace("ld_dn_pack_conv16", "ld_dn_pack_conv_f16")
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and bool(dw.isnan().all()) and not bool(w.any())


# ------------------------------------------------------------------------------------------------ 2. overflow
def test_an_overflow_is_an_inf_not_a_saturation():
    """One activation of 1e5 among small ones: the loader rounds it to inf (65504 would be a saturation), so exactly the
    outputs whose 3x3 window covers it are inf or NaN, in every channel; all others are finite and what they are without it."""
    shape = B, cin, cout, H, W, k = P.CONV_SHAPES[0]
    x, w = normal_uniform((B, cin, H, W), 4400) / 8, normal_uniform((cout, cin, k, k), 4401)
    y0, x0 = 2, 1
    clean = x.clone()
    clean[0, 7, y0, x0] = 0.0
    x[0, 7, y0, x0] = 1e5
    out = unpadded(hip_conv_f16(padded(x, cin), ohwi_f16(w), torch.zeros(cout), None, cin, cout, k), cout)
    covered = torch.zeros(B, cout, H, W, dtype=torch.bool)
    covered[0, :, max(0, y0 - 1):y0 + 2, max(0, x0 - 1):x0 + 2] = True
    assert covered.sum() == cout * 9 and H * W > 9
    assert bool((~torch.isfinite(out[covered])).all()) and bool(torch.isfinite(out[~covered]).all())
    ref64 = P.conv_ref(clean, w, None, None, F64, A.h)
    mag = P.conv_ref(clean.abs(), w.abs(), None, None, F64, A.h)
    err, bound = (out.double() - ref64).abs()[~covered], P.sum_bound(k * k * cin, mag)[~covered]
    assert bool((err <= bound).all())
    # the weight gradient sees it through dy the same way: one inf row of output channels
    ws = P.WGRAD_CASES[0][0]
    dy, a = normal_uniform((ws[0], ws[2], ws[3], ws[4]), 4410), normal_uniform((ws[0], ws[1], ws[3], ws[4]), 4411)
    dy[0, 5, 2, 1] = -1e5
    dw, _, _ = hip_wgrad_f16(dy, a, ws, None)
    assert bool((~torch.isfinite(dw[5])).all()) and bool(torch.isfinite(dw[:5]).all()) and bool(torch.isfinite(dw[6:]).all())


def test_what_the_matrix_cores_do_with_fp16_subnormals():
    """A probe that asserts nothing about the outcome: operands of 2^-20 (an fp16 subnormal, held exactly) times 2^10.  Kept,
    every output is K 2^-10; flushed to zero, it is 0.  Prints which."""
    B, cin, cout, H, W, k = P.CONV_SHAPES[2]
    x, w = torch.full((B, cin, H, W), 2.0 ** -20), torch.full((cout, cin, k, k), 2.0 ** 10)
    assert torch.equal(A.h(x), x)
    out = unpadded(hip_conv_f16(padded(x, cin), ohwi_f16(w), torch.zeros(cout), None, cin, cout, k), cout)
    kept = cin * k * k * 2.0 ** -10
    verdict = "kept" if bool((out == kept).all()) else "flushed to zero" if not bool(out.any()) else "something else"
    print(f"fp16 subnormal operands (2^-20 x 2^10, K = {cin * k * k}): outputs {float(out.min()):.6g} .. {float(out.max()):.6g}, "
          f"exact value {kept:.6g}: {verdict}")
    assert bool(torch.isfinite(out).all())


def test_a_resnet_block_under_amp_and_back():
    """``blk.amp = "fp16"`` repacks the weights as fp16 (``amp`` is in the cache key) and moves the output and the gradients
    off the fp32 path by less than ``conv_precision = "bf16"`` does; ``amp = "no"`` again reproduces the fp32 bits.  Every
    buffer of the module holds NaN first."""
    import resblock_ref as RB
    B, dim, dim_out, H, W, tdim = 2, 32, 64, 6, 5, 32
    blk = ldh.ResnetBlock(dim, dim_out, time_emb_dim=tdim)
    blk.load_state_dict(RB.make_block(dim, dim_out, tdim, key=dim + dim_out))
    blk = blk.to(DEV)
    blk.debug_fill = NAN
    x, temb = RB.uniform((B, dim, H, W), 11 * dim + H), RB.uniform((B, tdim), 13 * dim + H)
    dout = RB.uniform((B, dim_out, H, W), 17 * dim + H)                      # (of fp16-normal size: no scale needed)

    def run():
        xd, td = x.to(DEV).requires_grad_(True), temb.to(DEV).requires_grad_(True)
        blk.zero_grad(set_to_none=True)
        out = blk(xd, td)
        out.backward(dout.to(DEV))
        g = {"x": xd.grad, "time_emb": td.grad, **{k: p.grad for k, p in blk.named_parameters()}}
        return out.detach().clone(), {k: v.detach().clone() for k, v in g.items()}
    out32, g32 = run()
    assert blk._packed[1].w1f.dtype == F32
    blk.amp = "fp16"
    out16, g16 = run()
    assert blk._packed[1].w1f.dtype == F16 and blk._packed[1].w2d.dtype == F16 and blk._packed[1].wrf.dtype == F16
    blk.amp = "no"
    blk.conv_precision = "bf16"
    outb, gb = run()
    blk.conv_precision = "fp32"
    again, g_again = run()
    assert blk._packed[1].w1f.dtype == F32 and torch.equal(again, out32) and all(torch.equal(g_again[k], g32[k]) for k in g32)
    e16, eb = RB.rel_err(out16, out32), RB.rel_err(outb, out32)
    print(f"ResnetBlock output off the fp32 path: amp fp16 {e16:.2e}, conv_precision bf16 {eb:.2e}")
    assert 0.0 < e16 < eb < 2e-2 and e16 < 2e-3
    for k in ("x", "block1.proj.weight", "block2.proj.weight"):
        assert not torch.equal(g16[k], g32[k]) and RB.rel_err(g16[k], g32[k]) < RB.rel_err(gb[k], g32[k]), k


# ------------------------------------------------------------------------------------------------ 3. the optimiser kernels
SIZES = [1, 3, 2, 5, 32, 1000, 4099, 4097, 294912]        # (2 and 4099: the entries without moments)
NO_MOMENTS = (2, 6)
MISALIGNED = 5
CANARY, PAD = 7.5, 64
LR = 1e-3
B1, B2 = T.ADAM["betas"]


class Table:
    """tests/test_hip_denoiser_train.py's synthetic table (the same sizes, canaries and misaligned entry) with the scaler's
    state in a canaried buffer of its own and the scaled launches."""

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
        assert host[MISALIGNED].param % 16 == 4 and host[0].param % 16 == 0
        self.table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
        self.bufs = {k: torch.full((self.flat + 2 * PAD,), CANARY, dtype=F32, device=DEV) for k in ("grad", "m", "v", "ema")}
        self.work = torch.full((self.n_wg + 1 + 2 * PAD,), CANARY, dtype=F64, device=DEV)
        self.state = torch.full((8 + 2 * PAD,), 0x40F00000, dtype=torch.int32, device=DEV)       # (the bits of 7.5)
        self.adam = [i for i in range(n) if i not in NO_MOMENTS]

    def ptr(self, k):
        return self.bufs[k].data_ptr() + 4 * PAD

    def seg(self, k, i):
        t = self.params if k == "p" else self.bufs[k]
        at = self.starts[i] if k == "p" else PAD + self.off[i]
        return t[at:at + SIZES[i]]

    def sumsq_ptr(self):
        return self.work.data_ptr() + 8 * PAD

    def state_ptr(self):
        return self.state.data_ptr() + 4 * PAD

    def init(self, scale, adam_steps=0, tracker=0):
        cabi.check(cabi.lib().ld_dn_scaler_init(self.state_ptr(), scale, adam_steps, tracker, st()), "dn_scaler_init")

    def read(self):
        s = cabi.DnScalerState.from_buffer_copy(self.state[PAD:PAD + 8].cpu().numpy().tobytes())
        return {k: getattr(s, k) for k, _ in cabi.DnScalerState._fields_}

    def fill(self, key, grads=None, scale=1.0):
        """Parameters, EMA and zero moments from ``key``; ``grads`` {i: tensor} times ``scale`` (NaN where there is none)."""
        for i in range(self.n):
            self.seg("p", i).copy_(R.uniform((SIZES[i],), key + i))
            self.seg("ema", i).copy_(R.uniform((SIZES[i],), key + 100 + i))
            if i in self.adam:
                self.seg("m", i).zero_()
                self.seg("v", i).zero_()
        if grads is not None:
            self.set_grads(grads, scale)

    def set_grads(self, grads, scale=1.0):
        for i in range(self.n):
            self.seg("grad", i).copy_(grads[i] * scale if i in self.adam else torch.full((SIZES[i],), NAN))

    def scaled_step(self, max_norm, mode, w, growth=2.0, backoff=0.5, interval=2000):
        lib = cabi.lib()
        cabi.check(lib.ld_dn_opt_sqnorm(self.table.data_ptr(), self.n, self.n_wg, self.ptr("grad"), self.flat,
                                        self.sumsq_ptr() + 8, self.sumsq_ptr(), st()), "dn_opt_sqnorm")
        cabi.check(lib.ld_dn_opt_scaler_update(self.state_ptr(), self.sumsq_ptr(), LR, B1, B2, growth, backoff, interval, st()),
                   "dn_opt_scaler_update")
        cabi.check(lib.ld_dn_opt_step_scaled(self.table.data_ptr(), self.n, self.n_wg, self.ptr("grad"), self.ptr("m"),
                                             self.ptr("v"), self.ptr("ema"), self.flat, self.sumsq_ptr(), self.state_ptr(), max_norm,
                                             B1, B2, T.ADAM["eps"], mode, w, st()), "dn_opt_step_scaled")

    def snapshot(self):
        return {k: v.clone() for k, v in dict(self.bufs, p=self.params).items()}

    def outside_is_untouched(self):
        for k in ("grad", "m", "v", "ema", "p"):
            t = (self.params if k == "p" else self.bufs[k]).cpu()
            keep = torch.ones(t.numel(), dtype=torch.bool)
            for i, c in enumerate(SIZES):
                at = self.starts[i] if k == "p" else PAD + self.off[i]
                keep[at:at + c] = False
            assert bool((t[keep] == CANARY).all()), k
        w = self.work.cpu()
        assert bool((w[:PAD] == CANARY).all()) and bool((w[PAD + 1 + self.n_wg:] == CANARY).all())
        s = self.state.cpu()
        assert bool((s[:PAD] == 0x40F00000).all()) and bool((s[PAD + 8:] == 0x40F00000).all())


def table_grads(tb, key, norm):
    raw = {i: R.uniform((SIZES[i],), key + i) for i in tb.adam}
    scale = norm / math.sqrt(sum(float((g.double() ** 2).sum()) for g in raw.values()))
    return {i: (g.double() * scale).float() for i, g in raw.items()}


def test_scaled_step_on_a_synthetic_table():
    """Three calls at total norms 0.5, 3 and 0.9 (max_norm 1) with ema_mode 1, 2 (w 0.25) and 2 (w 0.63) at scale 1:
    parameters and the lerped EMA under ``adam_close`` (rtol 2.4e-7, atol 1e-5 lr) of fp32 torch, the moments within 1e-5 of
    the fp64 replica, gradients zeroed, canaries untouched.  The same three calls at scale 2^16 on gradients multiplied by
    2^16 leave the same bits everywhere: every scaling and unscaling by a power of two is exact."""
    calls = ((0.5, 1, 0.0), (3.0, 2, 0.25), (0.9, 2, 0.63))
    results = {}
    for scale in (1.0, 2.0 ** 16):
        tb = Table()
        tb.fill(3000)
        tb.init(scale)
        p0 = [tb.seg("p", i).cpu() for i in range(tb.n)]
        rep32 = T.Replica({str(i): p0[i] for i in range(tb.n)}, LR, 1.0, F32, None, no_grad=[str(i) for i in NO_MOMENTS])
        rep64 = T.Replica({str(i): p0[i] for i in range(tb.n)}, LR, 1.0, F64, None, no_grad=[str(i) for i in NO_MOMENTS])
        snaps = []
        for call, (norm, mode, w) in enumerate(calls, start=1):
            grads = table_grads(tb, 3200 + 10 * call, norm)
            tb.set_grads(grads, scale)
            ema_before = [tb.seg("ema", i).cpu() for i in range(tb.n)]
            tb.scaled_step(1.0, mode, w)
            tb.outside_is_untouched()
            s = tb.read()
            assert (s["scale"], s["growth_tracker"], s["adam_steps"], s["skipped_steps"], s["found_inf"]) == (scale, call, call, 0, 0)
            assert s["inv_scale"] == 1.0 / scale
            snaps.append(tb.snapshot())
            if scale != 1.0:
                continue
            rep32.step({str(i): g for i, g in grads.items()})
            rep64.step({str(i): g for i, g in grads.items()})
            for i in range(tb.n):
                p, e = tb.seg("p", i).cpu(), tb.seg("ema", i).cpu()
                if i in tb.adam:
                    T.adam_close(p, rep32.p[str(i)].detach(), LR, f"call {call} param {i}")
                    m64, v64 = rep64.moments(str(i))
                    em, ev = R.rel_err(tb.seg("m", i).cpu(), m64), R.rel_err(tb.seg("v", i).cpu(), v64)
                    assert em <= 1e-5 and ev <= 1e-5, (call, i, em, ev)
                    assert bool((tb.seg("grad", i) == 0).all()), (call, i)
                else:
                    assert torch.equal(p, p0[i]) and bool(tb.seg("grad", i).isnan().all()), (call, i)
                if mode == 1:
                    assert torch.equal(e, p), (call, i)
                else:
                    T.adam_close(e, torch.lerp(ema_before[i], p, w), LR, f"call {call} ema {i}")
            rep32.reset_params({str(i): tb.seg("p", i).cpu() for i in tb.adam})
        results[scale] = snaps
    for a, b in zip(results[1.0], results[2.0 ** 16]):
        for k in a:
            assert torch.equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("bad", [INF, -INF, NAN])
def test_a_planted_inf_skips_the_step(bad):
    """One non-finite gradient element: parameters and both moments keep their bits, the gradients are zeroed, the EMA did
    its action (a lerp towards the unchanged parameters), the scale halved, the tracker is 0, ``adam_steps`` stayed and
    ``skipped_steps`` went up; the next finite call steps with Adam's count 2, not 3."""
    tb = Table()
    tb.fill(3000)
    tb.init(2.0 ** 16, adam_steps=1, tracker=5)
    for i in tb.adam:
        tb.seg("m", i).copy_(R.uniform((SIZES[i],), 3300 + i) * 0.1)
        tb.seg("v", i).copy_(R.uniform((SIZES[i],), 3400 + i).abs() * 0.01)
    grads = table_grads(tb, 3500, 3.0)
    tb.set_grads(grads, 2.0 ** 16)
    tb.seg("grad", 5)[17] = bad
    before = tb.snapshot()
    tb.scaled_step(1.0, 2, 0.25)
    after = tb.snapshot()
    s = tb.read()
    assert (s["scale"], s["growth_tracker"], s["adam_steps"], s["skipped_steps"], s["found_inf"]) == (2.0 ** 15, 0, 1, 1, 1)
    assert s["inv_scale"] == 2.0 ** -16
    for k in ("p", "m", "v"):
        assert torch.equal(bits(before[k]), bits(after[k])), k
    for i in range(tb.n):
        if i in tb.adam:
            assert bool((tb.seg("grad", i) == 0).all()), i
        p = tb.seg("p", i).cpu()
        at = PAD + tb.off[i]
        e0 = before["ema"][at:at + SIZES[i]].cpu()
        T.adam_close(tb.seg("ema", i).cpu(), torch.lerp(e0, p, 0.25), LR, f"ema {i}")
        assert not torch.equal(tb.seg("ema", i).cpu(), e0), i
    tb.outside_is_untouched()
    # the next finite step is Adam's second: against a table that never saw the skipped call
    other = Table()
    other.params.copy_(after["p"])
    for k in ("m", "v", "ema"):
        other.bufs[k].copy_(after[k])
    other.init(2.0 ** 15, adam_steps=1)
    nxt = table_grads(tb, 3600, 0.7)
    for t in (tb, other):
        t.set_grads(nxt, 2.0 ** 15)
        t.scaled_step(1.0, 1, 0.0)
    a, b = tb.snapshot(), other.snapshot()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert tb.read()["adam_steps"] == 2 and tb.read()["skipped_steps"] == 1 and not torch.equal(bits(a["p"]), bits(after["p"]))


def test_the_scale_grows_after_growth_interval_finite_steps():
    tb = Table()
    tb.fill(3000)
    tb.init(2.0 ** 10)
    seen = []
    for call in range(5):
        tb.set_grads(table_grads(tb, 3700 + 10 * call, 0.5), 2.0 ** 10)       # (finite whatever the scale has become)
        tb.scaled_step(1.0, 0, 0.0, interval=2)
        s = tb.read()
        seen.append((s["scale"], s["growth_tracker"], s["adam_steps"]))
    assert seen == [(2.0 ** 10, 1, 1), (2.0 ** 11, 0, 2), (2.0 ** 11, 1, 3), (2.0 ** 12, 0, 4), (2.0 ** 12, 1, 5)]
    tb.outside_is_untouched()


def test_bias_corrections_on_the_device_follow_the_hosts():
    """``ld_dn_opt_scaler_update`` in a loop on a finite norm: ``step_size`` and ``bc2_sqrt`` for t = 1 .. 3000 lie within one
    fp32 ulp of ``apply()``'s host formula rounded to fp32 (the kernel's ``pow`` against Python's)."""
    tb = Table()
    tb.init(2.0 ** 16)
    tb.work[PAD] = 4.0
    n = 3000
    log = torch.zeros(n, 8, dtype=torch.int32, device=DEV)
    for t in range(n):
        cabi.check(cabi.lib().ld_dn_opt_scaler_update(tb.state_ptr(), tb.sumsq_ptr(), LR, B1, B2, 2.0, 0.5, 1 << 30, st()),
                   "dn_opt_scaler_update")
        log[t].copy_(tb.state[PAD:PAD + 8])
    got = log.cpu().numpy()
    assert got[:, 2].tolist() == list(range(1, n + 1)) and not got[:, 3].any() and not got[:, 4].any()
    step_size, bc2 = got[:, 6].copy().view(np.float32), got[:, 7].copy().view(np.float32)
    worst = [0.0, 0.0]
    for t in range(1, n + 1):
        for j, (have, want) in enumerate(((step_size[t - 1], LR / (1.0 - B1 ** t)), (bc2[t - 1], math.sqrt(1.0 - B2 ** t)))):
            want32 = np.float32(want)
            ulps = abs(float(have) - float(want32)) / float(np.spacing(want32))
            worst[j] = max(worst[j], ulps)
            assert ulps <= 1.0, (t, j, float(have), float(want32))
    print(f"device bias corrections, t = 1 .. {n}: step_size at most {worst[0]:.0f} ulp, bc2_sqrt at most {worst[1]:.0f} ulp from the host's")
    tb.outside_is_untouched()


# ------------------------------------------------------------------------------------------------ 4. the trainer
OPTS = dict(branch_out=False, start_intermediate=False, start_timestep=2, mask_x=False, ood_AD=False, ood_confidence=False,
            classifier=False, use_gt=False)
TIMESTEPS = 250
CASE = R.CASES[1]


def make_diffusion(seed=0):
    inf = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **R.KWARGS["mnist"])
    inf.load_state_dict(R.state("mnist", seed))
    return ldh.GaussianDiffusion(dict(OPTS, data="mnist"), inf, image_size=28, timesteps=TIMESTEPS, objective="pred_v").to(DEV)


def make_trainer(seed=0, **kw):
    args = dict(train_lr=LR, ema_update_every=T.EMA_KW["update_every"], ema_update_after_step=T.EMA_KW["update_after_step"])
    args.update(kw)
    tr = ldh.DenoiserTrainer(make_diffusion(seed), **args)
    tr.online_model.debug_fill = NAN
    return tr


def dev_batch(step, j):
    return tuple(v.to(DEV) for v in T.batch(CASE, step, j, TIMESTEPS))


def accumulate_step(tr, step, n_batches=2):
    total = None
    for j in range(n_batches):
        hr, lr, t, noise = dev_batch(step, j)
        value = tr.accumulate(hr, lr, scale=1.0 / n_batches, t=t, noise=noise)
        total = value if total is None else total + value
    return total


def cpu_state(tr):
    p = {k: v.detach().cpu().clone() for k, v in tr.online_model.named_parameters()}
    ema = {k: v.cpu() for k, v in tr.ema_state_dict().items()}
    mom = {k: (m.cpu(), v.cpu()) for k, (m, v) in tr.moments().items()}
    return p, ema, mom


def same_bits(a, b, what):
    sa, sb = cpu_state(a), cpu_state(b)
    for k in sa[0]:
        assert torch.equal(bits(sa[0][k]), bits(sb[0][k])) and torch.equal(bits(sa[1][k]), bits(sb[1][k])), (what, k)
        if k not in T.NO_GRAD:
            assert torch.equal(bits(sa[2][k][0]), bits(sb[2][k][0])) and torch.equal(bits(sa[2][k][1]), bits(sb[2][k][1])), (what, k)


def test_amp_steps_given_the_same_gradients():
    """Eight steps of ``amp=True`` (init_scale 2^16, growth_interval 3): before each ``apply()`` the accumulated, SCALED
    ``.grad``s go to CPU replicas whose Adam the real ``GradScaler`` drives (amp_ref.ScaledReplica).  After every step the
    scaler's five keys, Adam's step count and which steps were skipped are torch's; parameters and EMA under ``adam_close``
    of the fp32 replica, the moments within 1e-5 of the fp64 one (a skipped step: unchanged bits); every module packed fp16
    weights; the loss the trainer returns is unscaled."""
    kw = dict(init_scale=2.0 ** 16, growth_interval=3)
    tr = make_trainer(amp=True, scaler_kwargs=kw)
    assert tr.amp and tr.conv_precision == "fp32" and tr.online_model.amp == "fp16" and tr.scaler["growth_interval"] == 3
    plain = make_trainer()
    sd = R.state("mnist")
    rep32 = A.ScaledReplica(sd, LR, 1.0, F32, T.EMA_KW, **kw)
    rep64 = A.ScaledReplica(sd, LR, 1.0, F64, None, **kw)
    worst = dict(p=0.0, m=0.0, v=0.0, ema=0.0)
    for step in range(8):
        scale = tr.scaler_state()["scale"]
        loss = accumulate_step(tr, step)
        if step == 0:
            want = accumulate_step(plain, step)
            rel = abs(float(loss) - float(want)) / float(want)
            print(f"amp loss {float(loss):.6f}, fp32 {float(want):.6f} (rel {rel:.2e})")
            assert 0.0 < rel < 2e-3                                          # unscaled, and not the fp32 path's bits
            g16 = torch.cat([p.grad.reshape(-1) for p in tr.online_model.parameters() if p.grad is not None])
            g32 = torch.cat([p.grad.reshape(-1) for p in plain.online_model.parameters() if p.grad is not None])
            assert R.rel_err(g16 / scale, g32) < 2e-2 and not torch.equal(g16 / scale, g32)
        grads = {k: p.grad.detach().cpu().clone() for k, p in tr.online_model.named_parameters() if k not in T.NO_GRAD}
        before = cpu_state(tr)
        tr.apply()
        rep32.step(grads)
        rep64.step(grads)
        got, sd32 = tr.scaler_state(), rep32.scaler.state_dict()
        assert {k: got[k] for k in SCALER_KEYS} == sd32, (step, got, sd32)
        assert got["adam_steps"] == rep32.adam_steps() and got["found_inf"] == rep32.skipped[-1], (step, got)
        assert got["skipped_steps"] == sum(rep32.skipped) and tr.step == step + 1 and tr.ema_step == step + 1
        p, ema, mom = cpu_state(tr)
        for k in sd:
            if k in T.NO_GRAD:
                assert torch.equal(p[k], sd[k]) and k not in mom, k
                continue
            assert not bool(tr.online_model.get_parameter(k).grad.any()), k
            if got["found_inf"]:
                assert torch.equal(bits(p[k]), bits(before[0][k])) and torch.equal(bits(mom[k][0]), bits(before[2][k][0])) and \
                    torch.equal(bits(mom[k][1]), bits(before[2][k][1])), (step, k)
                continue
            worst["p"] = max(worst["p"], T.adam_close(p[k], rep32.p[k].detach(), LR, f"step {step} {k}"))
            worst["ema"] = max(worst["ema"], T.adam_close(ema[k], rep32.ema[k], LR, f"step {step} ema {k}"))
            m64, v64 = rep64.moments(k)
            em, ev = R.rel_err(mom[k][0], m64), R.rel_err(mom[k][1], v64)
            worst["m"], worst["v"] = max(worst["m"], em), max(worst["v"], ev)
            assert em <= 1e-5 and ev <= 1e-5, (step, k, em, ev)
        norm = tr.check_finite()                                             # (never raises under a scaler)
        assert (not math.isfinite(norm)) == got["found_inf"]
        rep32.reset_params({k: p[k] for k in grads}, {k: ema[k] for k in grads})
    assert rep32.adam_steps() >= 4, rep32.skipped
    mods = [m for m in tr.online_model.modules() if isinstance(m, TrainableModule)]
    dtypes = [{v.dtype for v in vars(m._packed[1]).values() if isinstance(v, torch.Tensor) and v.numel() >= 2048} for m in mods]
    assert all(m.amp == "fp16" for m in mods) and all(d == {F16} for d in dtypes if d) and sum(1 for d in dtypes if not d) == 1
    print(f"amp, eight steps (skipped: {rep32.skipped}): params {worst['p']:.2f} and ema {worst['ema']:.2f} of the allclose bound; "
          f"moments rel err exp_avg {worst['m']:.2e}, exp_avg_sq {worst['v']:.2e} (bound 1e-5); scale {got['scale']:.0f}")


def test_an_overflowing_init_scale_is_backed_off_and_then_trains():
    """init_scale 2^30 (test_amp_ref.py shows that the fp16-operand CPU denoiser overflows there): step 1 is skipped -- the
    weights keep their bits, the scale halves --, so are the next ones until the scale fits, and the later steps train.  The
    run ends bit-identical to a run started at the scale the first one backed off to and fed the steps that trained, with
    the same Adam count."""
    n = 18
    a = make_trainer(amp=True, scaler_kwargs=dict(init_scale=2.0 ** 30))
    w0 = cpu_state(a)[0]
    first = None
    for step in range(n):
        accumulate_step(a, step)
        a.apply()
        s = a.scaler_state()
        if step == 0:
            assert s["found_inf"] and (s["scale"], s["_growth_tracker"], s["adam_steps"], s["skipped_steps"]) == (2.0 ** 29, 0, 0, 1)
            assert not math.isfinite(a.check_finite())
            w1 = cpu_state(a)[0]
            assert all(torch.equal(bits(w0[k]), bits(w1[k])) for k in w0)
            assert not any(bool(p.grad.any()) for p in a.online_model.parameters() if p.grad is not None)
        if first is None and not s["found_inf"]:
            first = step
            assert s["scale"] == 2.0 ** (30 - first) and s["adam_steps"] == 1 and s["skipped_steps"] == first
    end = a.scaler_state()
    print(f"init_scale 2^30: the first {first} steps were skipped, {end['adam_steps']} of {n} trained, final scale {end['scale']:.0f}")
    assert first is not None and 1 <= first <= n - 3 and end["adam_steps"] >= 3 and end["adam_steps"] + end["skipped_steps"] == n
    assert a.step == n and a.ema_step == n
    assert not all(torch.equal(w0[k], v) for k, v in cpu_state(a)[0].items())
    b = make_trainer(amp=True, scaler_kwargs=dict(init_scale=2.0 ** (30 - first)))
    b.ema_step, b.ema_initted = first, a_initted_after(first)              # the EMA's counters advance on skipped steps too
    for step in range(first, n):
        accumulate_step(b, step)
        b.apply()
    same_bits(a, b, "after the back-off")
    sb = b.scaler_state()
    assert (sb["adam_steps"], sb["scale"], sb["_growth_tracker"]) == (end["adam_steps"], end["scale"], end["_growth_tracker"])
    assert (b.ema_step, b.ema_initted) == (a.ema_step, a.ema_initted)


def a_initted_after(calls):
    """``ema_initted`` after ``calls`` EMA updates at the trainer tests' ``update_every`` / ``update_after_step``."""
    kw = T.EMA_KW
    return any(s % kw["update_every"] == 0 and s > kw["update_after_step"] for s in range(calls))


def test_amp_save_load_and_three_more_steps(tmp_path):
    """``save`` after four steps of an amp run (init_scale 2^20, growth_interval 3), ``load`` into a second amp trainer (other
    weights, other initial scale), three more steps on both: parameters, moments, EMA, counters and the scaler bit-equal.  The
    file's ``'scaler'`` has ``GradScaler``'s five keys and its Adam steps are the count of steps that were not skipped; a
    trainer without amp refuses that file when steps were skipped (its two counts must agree) and otherwise ignores
    ``'scaler'``."""
    kw = dict(init_scale=2.0 ** 20, growth_interval=3)
    a = make_trainer(amp=True, scaler_kwargs=kw)
    for step in range(4):
        accumulate_step(a, step)
        a.apply()
    path = str(tmp_path / "model-best100.pt")
    a.save(path)
    sa = a.scaler_state()
    data = torch.load(path, map_location="cpu", weights_only=True)
    assert set(data["scaler"]) == set(SCALER_KEYS) == set(torch.amp.GradScaler("cpu").state_dict())
    assert data["scaler"] == {k: sa[k] for k in SCALER_KEYS} and data["step"] == 4
    assert {float(s["step"]) for s in data["opt"]["state"].values()} == {float(sa["adam_steps"])}
    b = make_trainer(seed=5, amp=True, scaler_kwargs=dict(init_scale=2.0 ** 8, growth_interval=3))
    info = b.load(path)
    assert info["source"] == "ema" and (b.step, b.ema_step, b.ema_initted) == (a.step, a.ema_step, a.ema_initted)
    assert b.scaler_state() == dict(sa, found_inf=False)
    for step in range(4, 7):
        for tr in (a, b):
            accumulate_step(tr, step)
            tr.apply()
    same_bits(a, b, "after load")
    assert a.scaler_state() == b.scaler_state() and (b.step, b.ema_step, b.ema_initted) == (7, 7, True)
    c = make_trainer(seed=6)
    if sa["skipped_steps"]:
        with pytest.raises(RuntimeError, match="Adam's step count"):
            c.load(path)
    else:
        c.load(path)
        assert c.step == 4
    with pytest.raises(RuntimeError, match="no loss scaler"):
        c.scaler_state()


def test_an_amp_step_does_not_synchronise():
    """tests/test_hip_denoiser_train.py's method: after a warm-up step, ``accumulate`` and ``apply`` of an amp trainer run under
    ``set_sync_debug_mode('error')``; ``scaler_state`` and ``check_finite`` are the calls that read back."""
    tr = make_trainer(amp=True)
    hr, lr, t, noise = dev_batch(0, 0)
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
        drawn = tr.accumulate(hr, lr, scale=0.5)
        tr.apply()
        with pytest.raises(RuntimeError):
            tr.scaler_state()
        with pytest.raises(RuntimeError):
            tr.check_finite()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    s = tr.scaler_state()
    assert math.isfinite(float(value)) and math.isfinite(float(drawn)) and tr.step == 2 and s["adam_steps"] + s["skipped_steps"] == 2


def test_two_emulated_amp_ranks_equal_one_rank():
    """Two emulated ranks (``EmulatedRank`` / ``gathered=``) under amp against one plain amp trainer that accumulates the same
    two micro-batches in order, from an init_scale of 2^30 with a back-off of 2^-6 so that the first step (at least) is a
    skip: after every step the online weights, both moments, the EMA, the squared norm, the loss and the scaler's state hold
    the same bits on both ranks and on the plain trainer."""
    kw = dict(init_scale=2.0 ** 30, backoff_factor=2.0 ** -6, growth_interval=2)
    ranks = [make_trainer(amp=True, scaler_kwargs=kw, comm=EmulatedRank(2, r)) for r in range(2)]
    plain = make_trainer(amp=True, scaler_kwargs=kw)
    for step in range(5):
        for r, tr in enumerate(ranks):
            hr, lr, t, noise = dev_batch(step, r)
            tr.accumulate(hr, lr, scale=0.5, t=t, noise=noise)
        gathered = torch.stack([tr.send_buffer() for tr in ranks]).contiguous()
        losses = [tr.apply(gathered=gathered) for tr in ranks]
        want = accumulate_step(plain, step)
        assert plain.apply() is None
        sp = plain.scaler_state()
        for r, tr in enumerate(ranks):
            same_bits(tr, plain, (step, r))
            assert torch.equal(bits(tr._work[:1]), bits(plain._work[:1])) and tr.scaler_state() == sp, (step, r)
            assert torch.equal(bits(losses[r]), bits(want)), (step, r)
            assert bool((tr.send_buffer() == 0).all())
        if step == 0:
            assert sp["found_inf"] and sp["scale"] == 2.0 ** 24
    assert sp["skipped_steps"] >= 1 and sp["adam_steps"] >= 2, sp


def test_without_amp_the_step_is_the_untouched_launch_pair():
    """``amp=False``: three steps through ``apply()`` against the same steps with ``ld_dn_opt_sqnorm`` and ``ld_dn_opt_step``
    called directly on a second trainer's buffers, the host's bias corrections as arguments -- parameters, moments and EMA
    ``torch.equal``: the fp32 launches were not rerouted.  No module carries ``amp``, and there is no scaler."""
    a, b = make_trainer(), make_trainer(amp=False, mixed_precision_type="fp16")
    lib = cabi.lib()
    for tr in (a, b):
        assert not tr.amp and tr.scaler is None and tr._scaler_state is None and tr.online_model.amp == "no"
        assert all("amp" not in vars(m) for m in tr.online_model.modules() if isinstance(m, TrainableModule))
    for step in range(3):
        la, lb = accumulate_step(a, step), accumulate_step(b, step)
        assert torch.equal(la, lb)
        a.apply()
        t = step + 1
        mode, decay = ldh.denoiser_train.ema_action(b.ema_step, initted=b.ema_initted, **b.ema_kw)
        sumsq = b._work.data_ptr()
        cabi.check(lib.ld_dn_opt_sqnorm(b._table.data_ptr(), b._n, b._n_wg, b._grad.data_ptr(), b._flat, sumsq + 8, sumsq, st()),
                   "dn_opt_sqnorm")
        cabi.check(lib.ld_dn_opt_step(b._table.data_ptr(), b._n, b._n_wg, b._grad.data_ptr(), b._m.data_ptr(), b._v.data_ptr(),
                                      b._ema.data_ptr(), b._flat, sumsq, b.max_grad_norm, B1, B2, b.eps, LR / (1.0 - B1 ** t),
                                      math.sqrt(1.0 - B2 ** t), mode, 1.0 - decay, st()), "dn_opt_step")
        torch.autograd.graph.increment_version(b._params)
        if b.ema_step % b.ema_kw["update_every"] == 0 and b.ema_step > b.ema_kw["update_after_step"]:
            b.ema_initted = True
        b.step += 1
        b.ema_step += 1
        same_bits(a, b, step)
        assert a.last_ema == (mode, decay)
    assert a.state()["scaler"] is None and float(a.state()["opt"]["state"][0]["step"]) == 3.0
