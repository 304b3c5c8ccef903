"""CPU tests of ``conv_out_storage`` (bf16 storage of the convolution outputs ``y1`` / ``y2`` that a ``ResnetBlock``'s
GroupNorms read): the attribute's defaults and refusals on every module, the combination with ``conv_precision="fp32"`` that
is refused, how ``TrainableUnet`` hands the value down, the host-side argument validation of the five entry points, and the
principle the GPU tests rest on -- on integer operands the convolution's sums are exact, so its rounded output is known bit
for bit and holds exact ties of the bf16 rounding.  No GPU."""
import ctypes as C

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import trainable
from localdiffusion_hallucination_amd.trainable import TrainableModule

import conv16_ref as P

NEW_SYMBOLS = ["ld_dn_conv16_to16", "ld_dn_conv16_from16_to16", "ld_dn_gn_forward_from16", "ld_dn_gn_forward_from16_to16",
               "ld_dn_gn_backward_from16"]
MNIST = dict(dim=32, dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist")
BAD = ("x", "fp16", "BF16", None, 16)
NEEDS = "conv_out_storage 'bf16' needs conv_precision 'bf16'"


def is_tie(t):
    """The fp32 values that lie exactly between two bf16 values: the low half of the pattern is 0x8000."""
    return (t.contiguous().view(torch.int32) & 0xFFFF) == 0x8000


# ------------------------------------------------------------------------------------------------ 1. the attribute
def test_conv_out_storage_defaults_and_refusals():
    """``"fp32"`` everywhere; ``"bf16"`` on ``ResnetBlock`` only; a refused value (``check_switch``'s text) leaves the old one
    in place; no ``state_dict`` knows the name."""
    assert trainable.SWITCHES["conv_out_storage"] == "CONV_OUT_STORAGES"
    assert TrainableModule.conv_out_storage == "fp32" and TrainableModule.CONV_OUT_STORAGES == ("fp32",)
    blk = ldh.ResnetBlock(32, 64, time_emb_dim=32)
    others = [ldh.LinearAttention(32), ldh.Attention(32), ldh.Downsample(32, 64), ldh.Upsample(64, 32),
              ldh.Conv2d(32, 32, 3, padding=1), ldh.BasicBlock(32, 32, 64)]
    others += [m for m in ldh.ResUnet("mnist").modules() if isinstance(m, TrainableModule)]
    assert len(others) > 6
    for m in others:
        assert m.conv_out_storage == "fp32", type(m).__name__
        m.conv_out_storage = "fp32"
        for bad in BAD + ("bf16",):
            with pytest.raises(ValueError, match=f"{type(m).__name__}: conv_out_storage {bad!r} is not one of 'fp32'$"):
                m.conv_out_storage = bad
        assert m.conv_out_storage == "fp32" and "conv_out_storage" not in "".join(m.state_dict())
    assert blk.conv_out_storage == "fp32" and type(blk).CONV_OUT_STORAGES == ("fp32", "bf16")
    blk.conv_out_storage = "bf16"
    assert blk.conv_out_storage == "bf16" and blk.act_storage == "fp32" and blk.conv_precision == "fp32"
    for bad in BAD:
        with pytest.raises(ValueError, match=f"ResnetBlock: conv_out_storage {bad!r} is not one of 'fp32', 'bf16'"):
            blk.conv_out_storage = bad
        assert blk.conv_out_storage == "bf16"
    blk.conv_out_storage = "fp32"
    assert blk.conv_out_storage == "fp32" and "conv_out_storage" not in "".join(blk.state_dict())
    with pytest.raises(ValueError, match="conv_out_storage"):
        ldh.TrainableUnet(**MNIST, conv_out_storage="fp16")
    with pytest.raises(ValueError, match="conv_out_storage"):
        ldh.DenoiserTrainer(None, conv_out_storage="fp8")


def test_the_generalised_check_and_the_old_name():
    for switch in ("act_storage", "conv_out_storage"):
        for storage, precision, ok in (("fp32", "fp32", True), ("fp32", "bf16", True), ("bf16", "bf16", True), ("bf16", "fp32", False)):
            if ok:
                trainable.check_storage_precision("m", switch, storage, precision)
            else:
                with pytest.raises(ValueError, match=f"m: {switch} 'bf16' needs conv_precision 'bf16' "):
                    trainable.check_storage_precision("m", switch, storage, precision)
    with pytest.raises(ValueError, match="m: act_storage 'bf16' needs conv_precision 'bf16'"):
        trainable.check_act_storage_precision("m", "bf16", "fp32")


def test_bf16_outputs_need_the_bf16_convolutions():
    """``ResnetBlock.forward`` refuses the combination before it looks at the device (x is a CPU tensor here), whatever
    ``act_storage`` says; ``DenoiserTrainer`` refuses it in its constructor, before it looks at its diffusion."""
    blk = ldh.ResnetBlock(32, 32)
    x = torch.zeros(1, 32, 4, 4)
    blk.conv_out_storage = "bf16"
    with pytest.raises(ValueError, match="ResnetBlock: " + NEEDS):
        blk(x)
    blk.conv_precision = "bf16"
    with pytest.raises(ValueError, match="CPU tensor"):
        blk(x)
    blk.act_storage = "bf16"                                                  # all four combinations of the two storages
    with pytest.raises(ValueError, match="CPU tensor"):
        blk(x)
    blk.conv_out_storage = "fp32"
    with pytest.raises(ValueError, match="CPU tensor"):
        blk(x)
    blk.act_storage, blk.conv_out_storage, blk.conv_precision = "fp32", "bf16", "fp32"
    with pytest.raises(ValueError, match=NEEDS):
        blk(x)
    blk.conv_out_storage = "fp32"
    with pytest.raises(ValueError, match="CPU tensor"):
        blk(x)
    with pytest.raises(ValueError, match="DenoiserTrainer: " + NEEDS):
        ldh.DenoiserTrainer(None, conv_out_storage="bf16")
    with pytest.raises(ValueError, match=NEEDS):
        ldh.DenoiserTrainer(None, conv_out_storage="bf16", conv_precision="fp32")
    for act in ("fp32", "bf16"):                                              # the combination that is allowed gets further
        with pytest.raises(ValueError, match="diffusion must be"):
            ldh.DenoiserTrainer(None, conv_out_storage="bf16", conv_precision="bf16", act_storage=act)


def test_the_unet_hands_the_storage_to_its_resnet_blocks_only():
    net = ldh.TrainableUnet(**MNIST)
    subs = [m for m in net.modules() if isinstance(m, TrainableModule)]
    blocks = [m for m in subs if isinstance(m, ldh.ResnetBlock)]
    rest = [m for m in subs if not isinstance(m, ldh.ResnetBlock)]
    assert len(blocks) >= 14 and len(rest) > 8
    assert net.conv_out_storage == "fp32" and all(m.conv_out_storage == "fp32" for m in subs)
    assert all("conv_out_storage" not in vars(m) for m in subs)             # the default is the class attribute
    keys = list(net.state_dict())
    net.conv_out_storage = "bf16"
    assert net.conv_out_storage == "bf16" and all(m.conv_out_storage == "bf16" for m in blocks)
    assert all(m.conv_out_storage == "fp32" and "conv_out_storage" not in vars(m) for m in rest)
    for other in ("conv_precision", "act_storage", "attn_precision", "full_attn_precision"):       # (left alone)
        assert getattr(net, other) == "fp32" and all(getattr(m, other, "fp32") == "fp32" for m in subs), other
    for bad in BAD:
        with pytest.raises(ValueError, match="conv_out_storage"):
            net.conv_out_storage = bad
        assert net.conv_out_storage == "bf16" and all(m.conv_out_storage == "bf16" for m in blocks)
    assert list(net.state_dict()) == keys and "conv_out_storage" not in "".join(keys)
    net.conv_out_storage = "fp32"
    assert all(m.conv_out_storage == "fp32" for m in subs)
    made = ldh.TrainableUnet(**MNIST, conv_precision="bf16", conv_out_storage="bf16")
    assert made.conv_out_storage == "bf16" and made.conv_precision == "bf16" and made.act_storage == "fp32"
    for m in made.modules():
        if isinstance(m, TrainableModule):
            assert m.conv_out_storage == ("bf16" if isinstance(m, ldh.ResnetBlock) else "fp32"), type(m).__name__
            assert m.act_storage == "fp32"
    assert list(made.state_dict()) == keys


def test_the_packed_weights_key_does_not_hold_the_storage():
    """``_packed_for`` does not repack when ``conv_out_storage`` changes (a stand-in ``_pack`` counts; no GPU)."""
    blk = ldh.ResnetBlock(32, 32)
    blk.conv_precision = "bf16"
    calls = []
    blk._pack = lambda dev: calls.append(blk.conv_out_storage) or len(calls)
    assert blk._packed_for("d") == 1
    blk.conv_out_storage = "bf16"
    assert blk._packed_for("d") == 1
    blk.conv_out_storage = "fp32"
    assert blk._packed_for("d") == 1 and calls == ["fp32"]


# ------------------------------------------------------------------------------------------------ 2. the entry points refuse
def test_symbols_are_exported():
    lib = cabi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def conv_args(**kw):
    a = cabi.PcConvArgs()
    p = 1 << 20                                          # (never dereferenced: every call below is refused on the host)
    a.src, a.weight, a.scale, a.shift, a.residual, a.out = p, None, p, p, None, p + 4096
    a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout, a.ksize, a.stride, a.relu = 1, 4, 4, 64, 4, 4, 64, 3, 1, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("name", ["ld_dn_conv16_to16", "ld_dn_conv16_from16_to16"])
def test_conv_to16_argument_validation_needs_no_gpu(name):
    """``ld_dn_conv16``'s refusals under the new name, the 4-byte alignment of the bf16 output and the aliasing case."""
    lib = cabi.lib()
    fn, p = getattr(lib, name), 1 << 20
    for kw, word in ((dict(stride=2, Ho=2, Wo=2), b"stride"), (dict(Cin=48), b"Cin"), (dict(Cout=32), b"Cout"),
                     (dict(ksize=5), b"ksize"), (dict(src=None), b"null"), (dict(out=None), b"null"), (dict(Ho=5), b"output"),
                     (dict(B=0), b"empty"), (dict(src=p + 8), b"aligned"), (dict(out=p + 4098), b"aligned"),
                     (dict(out=p + 4097), b"aligned"), (dict(residual=p + 4096), b"alias")):
        assert fn(C.byref(conv_args(**kw)), p, None) == -1, kw
        err = lib.ld_last_error()
        assert word in err and name.encode() + b":" in err, (kw, err)
    assert fn(C.byref(conv_args()), None, None) == -1 and b"null" in lib.ld_last_error() and name.encode() in lib.ld_last_error()
    assert fn(None, p, None) == -1 and b"null" in lib.ld_last_error() and name.encode() in lib.ld_last_error()
    assert fn(C.byref(conv_args()), p + 8, None) == -1 and b"aligned" in lib.ld_last_error()


@pytest.mark.parametrize("name", ["ld_dn_gn_forward_from16", "ld_dn_gn_forward_from16_to16"])
def test_gn_forward_from16_argument_validation_needs_no_gpu(name):
    lib = cabi.lib()
    fn, p = getattr(lib, name), 1 << 20

    def gn(y=p, g=p, b=p, film=None, res=None, work=p, stat=p, out=p + 4096, B=1, H=4, W=4, Cc=32, ldc=64, groups=8):
        return fn(y, g, b, film, res, work, stat, out, B, H, W, Cc, ldc, groups, None)
    cases = [(dict(Cc=24), b"groups"), (dict(ldc=16), b"ldc"), (dict(ldc=66), b"ldc"), (dict(B=0), b"B=0"),
             (dict(y=None), b"null"), (dict(work=None), b"null"), (dict(stat=None), b"null"), (dict(out=None), b"null"),
             (dict(out=p + 8), b"aligned"), (dict(y=p + 8), b"aligned"), (dict(y=p + 2), b"aligned"), (dict(film=p + 4), b"aligned"),
             (dict(res=p + 4), b"aligned")]
    if name.endswith("_to16"):
        cases.append((dict(res=p + 4096), b"alias"))
    for kw, word in cases:
        assert gn(**kw) == -1, kw
        err = lib.ld_last_error()
        assert word in err and name.encode() + b":" in err, (kw, err)


def test_gn_backward_from16_argument_validation_needs_no_gpu():
    lib = cabi.lib()
    name, p = b"ld_dn_gn_backward_from16:", 1 << 20

    def gnb(dout=p, y=p, stat=p, g=p, b=p, film=None, work=p, dg=p, db=p, dfilm=None, dy=p, B=1, H=4, W=4, Cc=32, ldc=64, groups=8):
        return lib.ld_dn_gn_backward_from16(dout, y, stat, g, b, film, work, dg, db, dfilm, dy, B, H, W, Cc, ldc, groups, None)
    for kw, word in ((dict(Cc=24), b"groups"), (dict(ldc=16), b"ldc"), (dict(ldc=66), b"ldc"), (dict(B=0), b"B=0"),
                     (dict(y=None), b"null"), (dict(dout=None), b"null"), (dict(stat=None), b"null"), (dict(work=None), b"null"),
                     (dict(dg=None), b"null"), (dict(dy=None), b"null"), (dict(film=p), b"go together"),
                     (dict(dfilm=p), b"go together"), (dict(y=p + 8), b"aligned"), (dict(y=p + 2), b"aligned"),
                     (dict(dout=p + 4), b"aligned"), (dict(dy=p + 4), b"aligned")):
        assert gnb(**kw) == -1, kw
        err = lib.ld_last_error()
        assert word in err and name in err, (kw, err)


# ------------------------------------------------------------------------------------------------ 3. the principle
@pytest.mark.parametrize("shape", P.CONV_SHAPES)
def test_the_rounded_output_of_an_exact_convolution_holds_ties(shape):
    """x integers in [-32, 32], w in {-1, 0, 1}: both are bf16 values and every sum is an integer far below 2^24, so the
    convolution's output is exact in fp32 in any order and ``q`` of it is THE rounded output.  It differs from the
    unrounded one, and some elements are exact ties of the bf16 rounding -- the elements that tell round-to-nearest-even
    from every other rounding (97 to 3,398 of them at these shapes)."""
    B, cin, cout, H, W, k = shape
    x, w = P.ints((B, cin, H, W), 8100 + cin + H, -32, 32).float(), P.trits((cout, cin, k, k), 8101 + cin + H).float()
    assert torch.equal(P.q(x), x) and torch.equal(P.q(w), w)
    y = P.conv_ref(x, w)
    assert torch.equal(y.double(), P.conv_ref(x, w, dt=torch.float64)) and float(y.abs().max()) < P.LIMIT
    yq = P.q(y)
    ties = is_tie(y)
    n = int(ties.sum())
    print(f"{shape}: {n} ties among {y.numel()} elements, {int((yq != y).sum())} elements moved")
    assert not torch.equal(yq, y)
    assert n > 0
    assert torch.equal(yq, y.to(torch.bfloat16).float())                     # (what the stored tensor holds)
    # nearest even: at a tie the kept pattern has an even last bit, and truncation or round-half-up would differ somewhere
    assert bool(((yq[ties].view(torch.int32) >> 16) & 1 == 0).all())
    assert not torch.equal(P.trunc(y), yq)
    half_up = ((y.view(torch.int32) + 0x8000) & -65536).view(torch.float32)
    assert not torch.equal(half_up, yq)
