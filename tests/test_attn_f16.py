"""CPU tests of ``amp_attn`` (the attention cores on the fp16 matrix cores): the exact probes of tests/attn_f16_ref.py prove
their own preconditions here, without a GPU; the Python surface -- ``AMP_ATTN_TYPES``, the defaults, every refusal in both
orders of assignment, ``TrainableUnet`` handing the value down, nothing in a ``state_dict`` --; and the reason for the one
operand pair that differs from the bf16 contract: the folded dv product is no further from the unrounded value than the one
that rounds ``ks``."""
import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import denoiser_train, trainable

import attn_f16_ref as P
import linattn_ref as R
import unet_grad_ref as UR
from amp_ref import h
from conv16_ref import _same, q

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ the probes
@pytest.mark.parametrize("shape", P.LA_PROBE_SHAPES)
@pytest.mark.parametrize("kind", P.LA_PROBE_KINDS)
def test_linear_probes_prove_themselves(shape, kind):
    """The builder's own assertions (exact below 2^24; bf16 rounding, truncation and no rounding show), and the folded dv:
    a bit-exact expectation exactly where the map has a power of two of pixels (8 x 8 and 16 x 32)."""
    pr = P.la_probe(shape, kind)
    n = shape[2] * shape[3]
    assert pr.want.dv_exact == (n in (64, 512))
    assert bool((pr.want.dv_bound == 0).all()) == pr.want.dv_exact
    assert pr.qkv.shape == (shape[0], 96 * shape[1], shape[2], shape[3]) and pr.qkv.dtype == torch.float32


@pytest.mark.parametrize("shape", P.FA_PROBE_SHAPES)
@pytest.mark.parametrize("kind", P.FA_FORWARD_KINDS)
def test_full_forward_probes_prove_themselves(shape, kind):
    pr = P.fa_forward_probe(shape, kind)
    assert pr.feeds == ("out" if kind == "v" else "lse") and bool(torch.isfinite(pr.want.lse).all())


@pytest.mark.parametrize("shape", P.FA_PROBE_SHAPES)
@pytest.mark.parametrize("kind", P.FA_BACKWARD_KINDS)
def test_full_backward_probes_prove_themselves(shape, kind):
    pr = P.fa_backward_probe(shape, kind)
    assert all(bool(torch.isfinite(getattr(pr.want, name)).all()) for name in ("dq", "dk", "dv"))


def test_the_probe_operands_tell_the_formats_apart():
    """``fp16_ties``: fp16 rounds some (the ties, to the even neighbour) and keeps the rest; bf16 keeps almost none."""
    from amp_ref import fp16_ties
    v = fp16_ties((4, 32, 64), 1)
    kept = h(v) == v
    assert bool(kept.any()) and not bool(kept.all())
    assert bool(((h(v) - v).abs() <= 1).all())
    assert bool(((h(v)[~kept] / 2) % 2 == 0).all())                  # a tie goes to the neighbour whose last bit is 0
    assert float((q(v) == v).float().mean()) < 0.1


# ------------------------------------------------------------------------------------------------ the surface
def test_types_and_defaults():
    assert trainable.AMP_ATTN_TYPES == ("fp32", "fp16")
    assert "amp_attn" not in trainable.SWITCHES
    assert ldh.LinearAttention.amp_attn == "fp32" and ldh.Attention.amp_attn == "fp32"
    lin, full = ldh.LinearAttention(32, heads=1), ldh.Attention(64, heads=2)
    assert lin.amp_attn == "fp32" and full.amp_attn == "fp32" and "amp_attn" not in vars(lin)
    net = ldh.TrainableUnet(dim=32, **UR.KWARGS["mnist"])
    assert net.amp_attn == "fp32"
    # the pinned tuples of the switches did not move
    assert ldh.LinearAttention.ATTN_PRECISIONS == ("fp32", "bf16") and ldh.Attention.FULL_ATTN_PRECISIONS == ("fp32", "bf16")
    assert trainable.AMP_TYPES == ("no", "fp16")


@pytest.mark.parametrize("make,rival", [(lambda: ldh.LinearAttention(32, heads=1), "attn_precision"),
                                        (lambda: ldh.Attention(32, heads=1), "full_attn_precision")])
def test_module_refusals_in_both_orders(make, rival):
    """A value outside ``AMP_ATTN_TYPES`` is refused and leaves the old one; ``"fp16"`` and the bf16 switch of the same
    launches are refused together whichever comes first; ``"fp16"`` stays refused on the switch itself; amp and
    conv_precision are independent of it."""
    mod = make()
    for bad in ("bf16", "no", "FP16", None, 16):
        with pytest.raises(ValueError, match="amp_attn"):
            mod.amp_attn = bad
        assert mod.amp_attn == "fp32"
    mod.amp_attn = "fp16"
    with pytest.raises(ValueError, match="amp_attn 'fp16' and " + rival):
        setattr(mod, rival, "bf16")
    assert getattr(mod, rival) == "fp32" and mod.amp_attn == "fp16"
    with pytest.raises(ValueError):
        setattr(mod, rival, "fp16")
    mod.amp_attn = "fp32"
    setattr(mod, rival, "bf16")
    with pytest.raises(ValueError, match="amp_attn 'fp16' and " + rival):
        mod.amp_attn = "fp16"
    assert mod.amp_attn == "fp32" and getattr(mod, rival) == "bf16"
    setattr(mod, rival, "fp32")
    for amp, conv in (("fp16", "fp32"), ("no", "bf16"), ("no", "fp32")):
        mod.conv_precision, mod.amp = "fp32", "no"
        mod.amp, mod.conv_precision = amp, conv
        mod.amp_attn = "fp16"
        assert (mod.amp, mod.conv_precision, mod.amp_attn) == (amp, conv, "fp16")
        mod.amp_attn = "fp32"


def attention_modules(net):
    lin = [m for m in net.modules() if isinstance(m, ldh.LinearAttention)]
    full = [m for m in net.modules() if isinstance(m, ldh.Attention)]
    return lin, full


def test_the_unet_hands_the_value_down_and_refuses():
    net = ldh.TrainableUnet(dim=32, **UR.KWARGS["mnist"])
    lin, full = attention_modules(net)
    assert len(lin) == 4 and len(full) == 3
    keys = list(net.state_dict())
    net.amp_attn = "fp16"
    assert net.amp_attn == "fp16" and all(m.amp_attn == "fp16" for m in lin + full)
    assert net.amp == "no" and all(m.amp == "no" for m in lin + full)              # independent of amp
    assert not any(hasattr(type(m), "AMP_ATTN_RIVAL") and type(m).AMP_ATTN_RIVAL is None and "amp_attn" in vars(m)
                   for m in net.modules())                                          # nobody else was told
    assert list(net.state_dict()) == keys and not any("amp_attn" in k for k in keys)
    for switch in ("attn_precision", "full_attn_precision"):
        with pytest.raises(ValueError, match="amp_attn 'fp16' and " + switch):
            setattr(net, switch, "bf16")
        assert getattr(net, switch) == "fp32"
    assert all(m.attn_precision == "fp32" for m in lin) and all(m.full_attn_precision == "fp32" for m in full)
    with pytest.raises(ValueError, match="amp_attn"):
        net.amp_attn = "bf16"
    assert net.amp_attn == "fp16"
    net.amp_attn = "fp32"
    assert all(m.amp_attn == "fp32" for m in lin + full)
    for switch in ("attn_precision", "full_attn_precision"):
        setattr(net, switch, "bf16")
        with pytest.raises(ValueError, match="amp_attn 'fp16' and " + switch):
            net.amp_attn = "fp16"
        assert net.amp_attn == "fp32" and all(m.amp_attn == "fp32" for m in lin + full)
        setattr(net, switch, "fp32")
    for kw in (dict(attn_precision="bf16"), dict(full_attn_precision="bf16")):
        with pytest.raises(ValueError, match="amp_attn"):
            ldh.TrainableUnet(dim=32, amp_attn="fp16", **kw, **UR.KWARGS["mnist"])
    with pytest.raises(ValueError, match="amp_attn"):
        ldh.TrainableUnet(dim=32, amp_attn="bf16", **UR.KWARGS["mnist"])
    built = ldh.TrainableUnet(dim=32, amp_attn="fp16", amp="fp16", **UR.KWARGS["mnist"])
    assert all(m.amp_attn == "fp16" for ms in attention_modules(built) for m in ms)


def test_amp_attn_is_no_part_of_a_state_dict():
    for mod in (ldh.LinearAttention(32, heads=1), ldh.Attention(32, heads=1)):
        before = {k: v.clone() for k, v in mod.state_dict().items()}
        mod.amp_attn = "fp16"
        after = mod.state_dict()
        assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
        other = type(mod)(32, heads=1)
        other.load_state_dict(after)
        assert other.amp_attn == "fp32"


def test_the_trainers_argument_check():
    """``check_amp_attn`` (what ``DenoiserTrainer.__init__`` calls before anything touches a GPU): fp16 needs the scaler of
    ``amp=True`` / ``mixed_precision_type="fp16"`` and neither bf16 attention switch."""
    check = denoiser_train.check_amp_attn
    assert check("fp32", "no", "bf16", "bf16") == "fp32" and check("fp16", "fp16", "fp32", "fp32") == "fp16"
    with pytest.raises(ValueError, match="needs amp=True"):
        check("fp16", "no", "fp32", "fp32")
    with pytest.raises(ValueError, match="attn_precision"):
        check("fp16", "fp16", "bf16", "fp32")
    with pytest.raises(ValueError, match="full_attn_precision"):
        check("fp16", "fp16", "fp32", "bf16")
    with pytest.raises(ValueError, match="amp_attn"):
        check("bf16", "fp16", "fp32", "fp32")


class _NoGpuDiffusion:
    """Enough of a diffusion for ``DenoiserTrainer``'s argument checks, which come before any GPU call."""
    model = None


@pytest.mark.parametrize("kw,match", [(dict(amp_attn="fp16"), "needs amp=True"),
                                      (dict(amp_attn="fp16", amp=True, mixed_precision_type="bf16"), "needs amp=True"),
                                      (dict(amp_attn="fp16", amp=True, attn_precision="bf16"), "attn_precision"),
                                      (dict(amp_attn="fp16", amp=True, full_attn_precision="bf16"), "full_attn_precision"),
                                      (dict(amp_attn="half", amp=True), "amp_attn")])
def test_the_trainer_refuses_before_any_gpu_call(kw, match):
    with pytest.raises(ValueError, match=match):
        ldh.DenoiserTrainer(_NoGpuDiffusion(), **kw)


def test_the_tools_take_the_flag():
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import train_denoiser
        a = train_denoiser.parse(["--data", "mnist", "--hr", "a.npy", "--lr", "b.npy", "--amp", "--amp-attn", "fp16"])
        assert a.amp_attn == "fp16" and train_denoiser.parse(["--data", "mnist", "--hr", "a.npy", "--lr", "b.npy"]).amp_attn == "fp32"
    finally:
        sys.path.remove(tools)
    for tool in ("bench_linattn_grad.py", "bench_attention_grad.py", "bench_unet_grad.py", "bench_denoiser_train.py"):
        with open(os.path.join(tools, tool)) as f:
            assert "amp_attn=True" in f.read(), tool


# ------------------------------------------------------------------------------------------------ why dv is folded
@pytest.mark.parametrize("shape", [(1, 1, 128, 128), (1, 1, 256, 256)])
def test_the_folded_dv_is_no_further_from_the_unrounded_value(shape):
    """Operands uniform in [-2, 2], dO uniform / (B H W) x 2^16, one head: the distance (max |difference| / max |value|) of dv
    to the fp64 value of the unrounded operands, for the fp16 contract (1 / Z on the dctx side) and for the one that rounds
    ks = exp(k - m) / Z, which lies in fp16's subnormals from 128 x 128 on.  Both are printed."""
    B, heads, H, W = shape
    qkv = R.uniform((B, 96 * heads, H, W), 31 * H + W, -2.0, 2.0)
    dout = R.uniform((B, 32 * heads, H, W), 37 * H + W) / (B * H * W) * 2.0 ** 16
    first = P.la_core(qkv, heads, dout, None, F64, _same)
    given = dict(ctx=first.ctx.float(), m=first.m.float(), Z=first.Z.float(), dctx=first.dctx.float(), rk=first.rk.float())
    want = P.la_core(qkv, heads, dout, given, F64, _same).dv
    assert torch.equal(want, P.la_core(qkv, heads, dout, given, F64, _same, fold=False).dv) or \
        R.rel_err(P.la_core(qkv, heads, dout, given, F64, _same, fold=False).dv, want) < 1e-12
    folded = R.rel_err(P.la_core(qkv, heads, dout, given, F64, h).dv, want)
    rounds_ks = R.rel_err(P.la_core(qkv, heads, dout, given, F64, h, fold=False).dv, want)
    ks = P.la_core(qkv, heads, dout, given, F64, _same).parts.ks
    print(f"dv at {H}x{W}: folded {folded:.2e}, rounding ks {rounds_ks:.2e} (ratio {rounds_ks / folded:.2f}); "
          f"ks {float(ks.min()):.2e} .. {float(ks.max()):.2e}")
    assert float(ks.min()) < 2.0 ** -14                                  # below fp16's smallest normal number
    assert folded <= rounds_ks
