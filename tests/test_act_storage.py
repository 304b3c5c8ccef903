"""CPU tests of ``act_storage`` (bf16 storage of the activations that only bf16 convolutions read): the attribute's defaults
and refusals on every module, the combination with ``conv_precision="fp32"`` that is refused, how ``TrainableUnet`` hands the
value down, the host-side argument validation of the four entry points, and the principle the switch rests on -- rounding an
activation that the convolution rounds anyway changes no bit.  No GPU."""
import ctypes as C

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd.trainable import TrainableModule, check_act_storage, check_act_storage_precision

import conv16_ref as P
import resblock_ref as R

NEW_SYMBOLS = ["ld_dn_conv16_from16", "ld_dn_wgrad16_from16", "ld_dn_gn_forward_to16", "ld_dn_pack_nhwc_to16"]
MNIST = dict(dim=32, dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist")
BAD = ("x", "fp16", "BF16", None, 16)


# ------------------------------------------------------------------------------------------------ 1. the attribute
def test_act_storage_defaults_and_refusals():
    """``"fp32"`` everywhere; ``"bf16"`` on ``ResnetBlock`` only; a refused value leaves the old one in place."""
    assert TrainableModule.act_storage == "fp32"
    blk = ldh.ResnetBlock(32, 64, time_emb_dim=32)
    others = [ldh.LinearAttention(32), ldh.Attention(32), ldh.Downsample(32, 64), ldh.Upsample(64, 32),
              ldh.Conv2d(32, 32, 3, padding=1), ldh.BasicBlock(32, 32, 64)]
    others += [m for m in ldh.ResUnet("mnist").modules() if isinstance(m, TrainableModule)]
    assert len(others) > 6
    for m in others:
        assert m.act_storage == "fp32", type(m).__name__
        m.act_storage = "fp32"
        for bad in BAD + ("bf16",):
            with pytest.raises(ValueError, match="act_storage"):
                m.act_storage = bad
        assert m.act_storage == "fp32" and "act_storage" not in "".join(m.state_dict())
    assert blk.act_storage == "fp32"
    blk.act_storage = "bf16"
    assert blk.act_storage == "bf16"
    for bad in BAD:
        with pytest.raises(ValueError, match="act_storage"):
            blk.act_storage = bad
        assert blk.act_storage == "bf16"
    blk.act_storage = "fp32"
    assert blk.act_storage == "fp32" and "act_storage" not in "".join(blk.state_dict())
    with pytest.raises(ValueError, match="act_storage"):
        ldh.TrainableUnet(**MNIST, act_storage="fp16")
    with pytest.raises(ValueError, match="act_storage"):
        ldh.DenoiserTrainer(None, act_storage="fp8")


def test_the_two_checks():
    assert check_act_storage("m", "bf16") == "bf16" and check_act_storage("m", "fp32", ("fp32",)) == "fp32"
    with pytest.raises(ValueError, match="m: act_storage 'bf16' is not one of 'fp32'"):
        check_act_storage("m", "bf16", ("fp32",))
    for storage, precision, ok in (("fp32", "fp32", True), ("fp32", "bf16", True), ("bf16", "bf16", True), ("bf16", "fp32", False)):
        if ok:
            check_act_storage_precision("m", storage, precision)
        else:
            with pytest.raises(ValueError, match="m: act_storage 'bf16' needs conv_precision 'bf16'"):
                check_act_storage_precision("m", storage, precision)


def test_bf16_storage_needs_the_bf16_convolutions():
    """``ResnetBlock.forward`` refuses the combination before it looks at the device (x is a CPU tensor here), and accepts it
    again -- as far as the device check -- once either attribute is set to match; ``DenoiserTrainer`` refuses it in its
    constructor, before it looks at its diffusion."""
    blk = ldh.ResnetBlock(32, 32)
    x = torch.zeros(1, 32, 4, 4)
    blk.act_storage = "bf16"
    with pytest.raises(ValueError, match="act_storage 'bf16' needs conv_precision 'bf16'"):
        blk(x)
    blk.conv_precision = "bf16"
    with pytest.raises(ValueError, match="CPU tensor"):
        blk(x)
    blk.conv_precision = "fp32"
    with pytest.raises(ValueError, match="act_storage 'bf16' needs conv_precision 'bf16'"):
        blk(x)
    blk.act_storage = "fp32"
    with pytest.raises(ValueError, match="CPU tensor"):
        blk(x)
    with pytest.raises(ValueError, match="act_storage 'bf16' needs conv_precision 'bf16'"):
        ldh.DenoiserTrainer(None, act_storage="bf16")
    with pytest.raises(ValueError, match="act_storage 'bf16' needs conv_precision 'bf16'"):
        ldh.DenoiserTrainer(None, act_storage="bf16", conv_precision="fp32")
    with pytest.raises(ValueError, match="diffusion must be"):              # the combination that is allowed gets further
        ldh.DenoiserTrainer(None, act_storage="bf16", conv_precision="bf16")


def test_the_unet_hands_the_storage_to_its_resnet_blocks_only():
    net = ldh.TrainableUnet(**MNIST)
    subs = [m for m in net.modules() if isinstance(m, TrainableModule)]
    blocks = [m for m in subs if isinstance(m, ldh.ResnetBlock)]
    rest = [m for m in subs if not isinstance(m, ldh.ResnetBlock)]
    assert len(blocks) >= 14 and len(rest) > 8
    assert net.act_storage == "fp32" and all(m.act_storage == "fp32" for m in subs)
    assert all("act_storage" not in vars(m) for m in subs)                  # the default is the class attribute
    keys = list(net.state_dict())
    net.act_storage = "bf16"
    assert net.act_storage == "bf16" and all(m.act_storage == "bf16" for m in blocks)
    assert all(m.act_storage == "fp32" and "act_storage" not in vars(m) for m in rest)
    assert net.conv_precision == "fp32" and all(m.conv_precision == "fp32" for m in subs)     # (the other switch is untouched)
    for bad in BAD:
        with pytest.raises(ValueError, match="act_storage"):
            net.act_storage = bad
        assert net.act_storage == "bf16" and all(m.act_storage == "bf16" for m in blocks)
    assert list(net.state_dict()) == keys and "act_storage" not in "".join(keys)
    net.act_storage = "fp32"
    assert all(m.act_storage == "fp32" for m in subs)
    made = ldh.TrainableUnet(**MNIST, conv_precision="bf16", act_storage="bf16")
    assert made.act_storage == "bf16" and made.conv_precision == "bf16"
    for m in made.modules():
        if isinstance(m, TrainableModule):
            assert m.act_storage == ("bf16" if isinstance(m, ldh.ResnetBlock) else "fp32"), type(m).__name__
    assert list(made.state_dict()) == keys


def test_the_packed_weights_key_does_not_hold_the_storage():
    """``_packed_for`` does not repack when ``act_storage`` changes (a stand-in ``_pack`` counts; no GPU)."""
    blk = ldh.ResnetBlock(32, 32)
    blk.conv_precision = "bf16"
    calls = []
    blk._pack = lambda dev: calls.append(blk.act_storage) or len(calls)
    assert blk._packed_for("d") == 1
    blk.act_storage = "bf16"
    assert blk._packed_for("d") == 1
    blk.act_storage = "fp32"
    assert blk._packed_for("d") == 1 and calls == ["fp32"]


# ------------------------------------------------------------------------------------------------ 2. the entry points refuse
def test_symbols_are_exported():
    lib = cabi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


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
    # ld_dn_conv16_from16: ld_dn_conv16's refusals, the alignment rule for the bf16 source
    for kw, word in ((dict(stride=2, Ho=2, Wo=2), b"stride"), (dict(Cin=48), b"Cin"), (dict(Cout=32), b"Cout"),
                     (dict(ksize=5), b"ksize"), (dict(src=None), b"null"), (dict(out=None), b"null"), (dict(Ho=5), b"output"),
                     (dict(B=0), b"empty"), (dict(src=p + 8), b"aligned"), (dict(src=p + 2), b"aligned")):
        assert lib.ld_dn_conv16_from16(C.byref(conv_args(**kw)), p, None) == -1, kw
        err = lib.ld_last_error()
        assert word in err and b"ld_dn_conv16_from16" in err, (kw, err)
    assert lib.ld_dn_conv16_from16(C.byref(conv_args()), None, None) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_conv16_from16(None, p, None) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_conv16_from16(C.byref(conv_args()), p + 8, None) == -1 and b"aligned" in lib.ld_last_error()

    def wgrad(dy=p, a=p, work=p, dw=p, B=1, H=4, W=4, Cin=64, Cout=64, k=3, splits=1):
        return lib.ld_dn_wgrad16_from16(dy, a, work, dw, B, H, W, Cin, Cout, k, splits, None)
    for kw, word in ((dict(Cin=48), b"Cin"), (dict(Cin=32), b"Cin"), (dict(Cout=32), b"Cout"), (dict(k=5), b"ksize"),
                     (dict(splits=0), b"splits"), (dict(splits=2), b"splits"), (dict(work=None), b"null"), (dict(dy=None), b"null"),
                     (dict(a=None), b"null"), (dict(H=0), b"empty"), (dict(a=p + 8), b"aligned"), (dict(dy=p + 4), b"aligned")):
        assert wgrad(**kw) == -1, kw
        err = lib.ld_last_error()
        assert word in err and b"ld_dn_wgrad16_from16" in err, (kw, err)

    def gn(y=p, g=p, b=p, film=None, res=None, work=p, stat=p, out=p + 4096, B=1, H=4, W=4, Cc=32, ldc=64, groups=8):
        return lib.ld_dn_gn_forward_to16(y, g, b, film, res, work, stat, out, B, H, W, Cc, ldc, groups, None)
    for kw, word in ((dict(Cc=24), b"groups"), (dict(ldc=16), b"ldc"), (dict(ldc=66), b"ldc"), (dict(B=0), b"B=0"),
                     (dict(y=None), b"null"), (dict(work=None), b"null"), (dict(stat=None), b"null"), (dict(out=None), b"null"),
                     (dict(out=p + 8), b"aligned"), (dict(y=p + 4), b"aligned"), (dict(film=p + 4), b"aligned"),
                     (dict(res=p + 4096), b"alias")):
        assert gn(**kw) == -1, kw
        err = lib.ld_last_error()
        assert word in err and b"ld_dn_gn_forward_to16" in err, (kw, err)

    def pack(x=p, out=p, B=1, Cc=32, H=4, W=4, sb=512, sc=16, sh=4, sw=1, ldc=64):
        return lib.ld_dn_pack_nhwc_to16(x, out, B, Cc, H, W, sb, sc, sh, sw, ldc, None)
    for kw, word in ((dict(ldc=16), b"shape"), (dict(B=0), b"shape"), (dict(Cc=33, ldc=33), b"even"), (dict(sc=-16), b"negative"),
                     (dict(x=None), b"null"), (dict(out=None), b"null"), (dict(out=p + 2), b"aligned")):
        assert pack(**kw) == -1, kw
        err = lib.ld_last_error()
        assert word in err and b"ld_dn_pack_nhwc_to16" in err, (kw, err)


# ------------------------------------------------------------------------------------------------ 3. the principle
@pytest.mark.parametrize("shape", [P.CONV_SHAPES[0], P.CONV_WITH_EPILOGUE])
def test_rounding_what_the_convolution_rounds_changes_no_bit(shape):
    """``q`` is idempotent, so the yardstick of the bf16 convolution gives the same bits on ``q(x)`` as on ``x``, and so does
    the weight gradient's on ``q(a)``: a tensor that only these kernels read can be stored rounded.  On operands bf16 does not
    hold (ties and neighbours, uniform), which the fp32 convolution does tell apart."""
    B, cin, cout, H, W, k = shape
    for x in (P.ties_and_neighbours((B, cin, H, W), 41).float(), R.uniform((B, cin, H, W), 42)):
        w, dy = R.uniform((cout, cin, k, k), 43), R.uniform((B, cout, H, W), 44)
        xq = P.q(x)
        assert not torch.equal(xq, x) and torch.equal(P.q(xq), xq)
        assert torch.equal(xq, x.to(torch.bfloat16).float())                 # (what the stored tensor holds)
        assert torch.equal(P.conv_ref(xq, w), P.conv_ref(x, w))
        assert torch.equal(P.wgrad_ref(dy, xq, k), P.wgrad_ref(dy, x, k))
        same = lambda t: t                                                   # noqa: E731  (the unrounded forms do differ)
        assert not torch.equal(P.conv_ref(xq, w, rnd=same), P.conv_ref(x, w, rnd=same))
        assert not torch.equal(P.wgrad_ref(dy, xq, k, rnd=same), P.wgrad_ref(dy, x, k, rnd=same))
