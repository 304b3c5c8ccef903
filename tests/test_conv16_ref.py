"""CPU tests of the bf16 convolutions' yardstick (tests/conv16_ref.py), of the three entry points' argument validation and
of the ``conv_precision`` switch's refusals.  No GPU: the probes' preconditions are proved here, at every shape
tests/test_hip_conv16.py compares on the GPU."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd.trainable import TrainableModule

import conv16_ref as P
import resblock_ref as R

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------ 1. the probes
def test_rounding_operands_hit_every_case():
    """Ties to even in both directions, round down, round up, and values bf16 holds."""
    v = P.ties_and_neighbours((4096,), 1).abs()
    r = P.q(v)
    odd = v[v < 512]
    assert bool((odd % 2 == 1).all()) and bool(((P.q(odd) - odd).abs() == 1).all()) and bool((P.q(odd) % 4 == 0).all())
    assert bool((P.q(odd) > odd).any()) and bool((P.q(odd) < odd).any())
    wide = v[v > 512]
    for residue, delta in ((0, 0), (1, -1), (3, 1)):
        sel = wide[wide % 4 == residue]
        assert sel.numel() and bool((P.q(sel) - sel == delta).all())
    tie = wide[wide % 4 == 2]
    assert tie.numel() and bool((P.q(tie) % 8 == 0).all())
    assert bool((P.trunc(v) <= v).all()) and not torch.equal(P.trunc(v), r)
    assert torch.equal(P.trunc(-v), -P.trunc(v))


@pytest.mark.parametrize("shape", P.CONV_SHAPES)
@pytest.mark.parametrize("kind", ["identity", "rounding"])
def test_conv_probes(shape, kind):
    p = P.conv_probe(shape, kind, epilogue=shape == P.CONV_WITH_EPILOGUE)
    assert p.ref.shape == (shape[0], shape[2], shape[3], shape[4]) and bool(p.ref.any())
    if shape == P.CONV_WITH_EPILOGUE:
        assert bool(p.shift.any()) and bool(p.res.any())


@pytest.mark.parametrize("kind", ["identity", "rounding_w", "rounding_dy"])
def test_dgrad_probes(kind):
    B, cin, cout, H, W, k = P.DGRAD_SHAPE
    p = P.dgrad_probe(P.DGRAD_SHAPE, kind)
    assert p.ref.shape == (B, cin, H, W)
    leaf = torch.zeros(B, cin, H, W, dtype=F64, requires_grad=True)          # it IS the transposed convolution
    (want,) = torch.autograd.grad(F.conv2d(leaf, P.q(p.w).double(), padding=k // 2), leaf, P.q(p.dy).double())
    assert torch.equal(p.ref.double(), want)


@pytest.mark.parametrize("shape", P.WGRAD_SHAPES)
@pytest.mark.parametrize("kind", ["identity", "rounding_dy", "rounding_a"])
def test_wgrad_probes(shape, kind):
    B, cin, cout, H, W, k = shape
    p = P.wgrad_probe(shape, kind)
    assert p.ref.shape == (cout, cin, k, k)
    leaf = torch.zeros(cout, cin, k, k, dtype=F64, requires_grad=True)
    (want,) = torch.autograd.grad(F.conv2d(P.q(p.a).double(), leaf, padding=k // 2), leaf, P.q(p.dy).double())
    assert torch.equal(p.ref.double(), want)


@pytest.mark.parametrize("shape", P.PACK_SHAPES)
def test_pack_probes(shape):
    co, ci, k = shape
    p = P.pack_probe(shape)
    fwd, dgr = p.fwd.view(p.cop, k * k, p.cip), p.dgr.view(p.cip, k * k, p.cop)
    assert torch.equal(fwd[co - 1, 0, :ci], P.q(p.w)[co - 1, :, 0, 0]) and torch.equal(dgr[:ci, k * k - 1, 0], P.q(p.w)[0, :, 0, 0])
    assert not bool(fwd[co:].any()) and not bool(fwd[..., ci:].any()) and not bool(dgr[ci:].any()) and not bool(dgr[..., co:].any())
    # the data-gradient layout, read as a forward OHWI weight of the transposed convolution, gives conv_transpose2d
    dy = P.trits((1, co, 4, 3), 5)
    w_t = dgr.view(p.cip, k, k, p.cop)[:ci, :, :, :co].permute(0, 3, 1, 2)
    assert torch.equal(F.conv2d(dy, w_t, padding=k // 2), F.conv_transpose2d(dy, P.q(p.w), padding=k // 2))


# ------------------------------------------------------------------------------------------------ 2. Bf16Conv
def test_bf16conv_gradients_are_their_definitions():
    """dx, dw and db of ``Bf16Conv`` on a tiny case in fp64: dx and dw are autograd's through a plain convolution of the
    ROUNDED operands with the ROUNDED upstream gradient, db is the sum of the upstream gradient as it is."""
    x, w, b = R.uniform((2, 3, 5, 4), 1).double(), R.uniform((4, 3, 3, 3), 2).double(), R.uniform((4,), 3).double()
    dout = R.uniform((2, 4, 5, 4), 4).double()
    assert not torch.equal(P.q(x), x) and not torch.equal(P.q(dout), dout)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    out = P.Bf16Conv.apply(*leaves)
    dx, dw, db = torch.autograd.grad(out, leaves, dout)
    xq, wq = P.q(x).requires_grad_(True), P.q(w).requires_grad_(True)
    plain = F.conv2d(xq, wq, padding=1)
    assert torch.equal(out, plain + b[None, :, None, None])
    dxr, dwr = torch.autograd.grad(plain, [xq, wq], P.q(dout))
    assert torch.allclose(dx, dxr, rtol=0, atol=1e-13) and torch.allclose(dw, dwr, rtol=0, atol=1e-13)
    assert torch.equal(db, dout.sum(dim=(0, 2, 3)))
    direct = torch.zeros_like(dw)                     # the weight gradient, term by term
    xp = F.pad(P.q(x), (1, 1, 1, 1))
    for i in range(3):
        for j in range(3):
            direct[:, :, i, j] = torch.einsum("boyx,bcyx->oc", P.q(dout), xp[:, :, i:i + 5, j:j + 4])
    assert torch.allclose(dw, direct, rtol=0, atol=1e-13)


def test_block_on_bf16conv_differs_from_the_fp32_block_by_the_rounding():
    """The restated block is the oracle's block up to the bf16 rounding of the convolutions' operands (a few 2^-9)."""
    sd = R.make_block(32, 64, 32, key=96)
    x, temb, dout = R.uniform((2, 32, 6, 5), 1), R.uniform((2, 32), 2), R.uniform((2, 64, 6, 5), 3)
    out16, g16 = P.block_yardstick(sd, x, temb, dout, F64)
    out32, g32 = R.yardstick(sd, x, temb, dout, dtype=F64)
    assert set(g16) == set(g32)
    e = R.rel_err(out16, out32)
    assert 1e-4 < e < 2e-2, e
    for k in g32:
        if k == "res_conv.bias":                      # the plain sum of dout: no rounded operand on its way
            assert torch.equal(g16[k], g32[k])
        else:
            assert 1e-5 < R.rel_err(g16[k], g32[k]) < 5e-2, k


# ------------------------------------------------------------------------------------------------ 3. the entry points refuse
def conv_args(**kw):
    a = cabi.PcConvArgs()
    p = 1 << 20                                          # (never dereferenced: every call below is refused on the host)
    a.src, a.weight, a.scale, a.shift, a.residual, a.out = p, None, p, p, None, p
    a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout, a.ksize, a.stride, a.relu = 1, 4, 4, 64, 4, 4, 64, 3, 1, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_validation_needs_no_gpu():
    lib = cabi.lib()
    p = 1 << 20
    for kw, word in ((dict(stride=2, Ho=2, Wo=2), b"stride"), (dict(Cin=48), b"Cin"), (dict(Cout=32), b"Cout"),
                     (dict(ksize=5), b"ksize"), (dict(src=None), b"null"), (dict(out=None), b"null"), (dict(Ho=5), b"output")):
        assert lib.ld_dn_conv16(C.byref(conv_args(**kw)), p, None) == -1, kw
        assert word in lib.ld_last_error(), (kw, lib.ld_last_error())
    assert lib.ld_dn_conv16(C.byref(conv_args()), None, None) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_conv16(None, p, None) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_conv16(C.byref(conv_args()), p + 8, None) == -1 and b"aligned" in lib.ld_last_error()

    def wgrad(dy=p, a=p, work=p, dw=p, B=1, H=4, W=4, Cin=64, Cout=64, k=3, splits=1):
        return lib.ld_dn_wgrad16(dy, a, work, dw, B, H, W, Cin, Cout, k, splits, None)
    for kw, word in ((dict(Cin=48), b"Cin"), (dict(Cin=32), b"Cin"), (dict(Cout=32), b"Cout"), (dict(k=5), b"ksize"),
                     (dict(splits=0), b"splits"), (dict(splits=2), b"splits"), (dict(work=None), b"null"), (dict(dy=None), b"null"),
                     (dict(H=0), b"empty"), (dict(a=p + 4), b"aligned")):
        assert wgrad(**kw) == -1, kw
        assert word in lib.ld_last_error(), (kw, lib.ld_last_error())

    def pack(w=p, fwd=p, dgr=p, co=32, cop=64, ci=32, cip=64, k=3):
        return lib.ld_dn_pack_conv16(w, fwd, dgr, co, cop, ci, cip, k, None)
    for kw, word in ((dict(k=5), b"ksize"), (dict(w=None), b"null"), (dict(dgr=None), b"null"), (dict(cop=16), b"co "),
                     (dict(ci=0), b"ci "), (dict(cip=33), b"even"), (dict(fwd=p + 2), b"aligned")):
        assert pack(**kw) == -1, kw
        assert word in lib.ld_last_error(), (kw, lib.ld_last_error())


# ------------------------------------------------------------------------------------------------ 4. the switch
MNIST = dict(dim=32, dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist")


def test_conv_precision_defaults_and_refusals():
    assert TrainableModule.conv_precision == "fp32"
    mods = [ldh.ResnetBlock(32, 64, time_emb_dim=32), ldh.LinearAttention(32), ldh.Attention(32), ldh.Downsample(32, 64),
            ldh.Upsample(64, 32), ldh.Conv2d(32, 32, 3, padding=1), ldh.BasicBlock(32, 32, 64), ldh.ResUnet("mnist")]
    for m in mods[:-1]:
        assert m.conv_precision == "fp32", type(m).__name__
        m.conv_precision = "bf16"
        assert m.conv_precision == "bf16"
        for bad in ("x", "fp16", None, 16):
            with pytest.raises(ValueError, match="conv_precision"):
                m.conv_precision = bad
        assert m.conv_precision == "bf16"
        m.conv_precision = "fp32"
    for blk in mods[-1].modules():                                       # the encoder's blocks take the attribute
        if isinstance(blk, ldh.BasicBlock):
            blk.conv_precision = "bf16"
    with pytest.raises(ValueError, match="conv_precision"):
        ldh.TrainableUnet(**MNIST, conv_precision="fp8")
    with pytest.raises(ValueError, match="conv_precision"):
        ldh.DenoiserTrainer(None, conv_precision="fp16")
    with pytest.raises(ValueError, match="conv_precision"):
        ldh.ResnetBlock(32, 32).conv_precision = "x"


def test_the_unet_hands_the_precision_to_every_module():
    net = ldh.TrainableUnet(**MNIST)
    subs = [m for m in net.modules() if isinstance(m, TrainableModule)]
    assert len(subs) > 20 and net.conv_precision == "fp32" and all(m.conv_precision == "fp32" for m in subs)
    assert "conv_precision" not in "".join(net.state_dict())
    net.conv_precision = "bf16"
    assert net.conv_precision == "bf16" and all(m.conv_precision == "bf16" for m in subs)
    with pytest.raises(ValueError, match="conv_precision"):
        net.conv_precision = "tf32"
    assert net.conv_precision == "bf16" and all(m.conv_precision == "bf16" for m in subs)
    made = ldh.TrainableUnet(**MNIST, conv_precision="bf16")
    assert all(m.conv_precision == "bf16" for m in made.modules() if isinstance(m, TrainableModule))
    assert list(made.state_dict()) == list(ldh.TrainableUnet(**MNIST).state_dict())


def test_the_packed_weights_key_holds_the_precision():
    """``_packed_for`` repacks when the precision changes (a stand-in ``_pack`` counts; no GPU)."""
    blk = ldh.ResnetBlock(32, 32)
    calls = []
    blk._pack = lambda dev: calls.append(blk.conv_precision) or len(calls)
    assert blk._packed_for("d") == 1 and blk._packed_for("d") == 1
    blk.conv_precision = "bf16"
    assert blk._packed_for("d") == 2 and blk._packed_for("d") == 2
    blk.conv_precision = "fp32"
    assert blk._packed_for("d") == 3 and calls == ["fp32", "bf16", "fp32"]
