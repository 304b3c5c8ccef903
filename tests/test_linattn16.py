"""CPU tests of ``attn_precision``: the switch's defaults and refusals, the four bf16 entry points' argument validation, and
the yardstick of tests/linattn16_ref.py -- ``core16`` against autograd, and the preconditions of every exact probe at every
shape tests/test_hip_linattn16.py compares on the GPU.  No GPU."""
import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi

import linattn16_ref as P
import linattn_ref as R

F32, F64 = torch.float32, torch.float64
MNIST = dict(dim=32, dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist")
BAD = ("x", "fp16", None, 16)
NAMES = ("context", "out", "backward_reduce", "backward_apply")
# What this file is about: without the four entry points and the attribute nothing below says anything, so it does not load.
ENTRY = {n: getattr(cabi.lib(), f"ld_dn_la_{n}16") for n in NAMES}
assert ldh.LinearAttention.ATTN_PRECISIONS == ("fp32", "bf16") and ldh.Attention.ATTN_PRECISIONS == ("fp32",)


# ------------------------------------------------------------------------------------------------ 1. the attribute
def test_attn_precision_defaults_and_refusals():
    la, fa = ldh.LinearAttention(32), ldh.Attention(32)
    assert ldh.LinearAttention.attn_precision == "fp32" and ldh.Attention.attn_precision == "fp32"
    assert la.attn_precision == "fp32" and fa.attn_precision == "fp32"
    la.attn_precision = "bf16"
    assert la.attn_precision == "bf16"
    for bad in BAD:
        with pytest.raises(ValueError, match="attn_precision"):
            la.attn_precision = bad
        with pytest.raises(ValueError, match="attn_precision"):
            fa.attn_precision = bad
    assert la.attn_precision == "bf16" and fa.attn_precision == "fp32"          # a refused value leaves the old one
    with pytest.raises(ValueError, match="attn_precision"):
        fa.attn_precision = "bf16"                                               # the full-softmax core: not until its slice
    fa.attn_precision = "fp32"
    la.attn_precision = "fp32"
    assert la.conv_precision == "fp32"                                           # ... and the other switch is its own
    la.conv_precision = "bf16"
    assert la.attn_precision == "fp32"
    with pytest.raises(ValueError, match="attn_precision"):
        ldh.TrainableUnet(**MNIST, attn_precision="fp8")
    with pytest.raises(ValueError, match="attn_precision"):
        ldh.DenoiserTrainer(None, attn_precision="fp16")
    with pytest.raises(ValueError, match="attn_precision"):                      # independent of conv_precision: refused by itself
        ldh.DenoiserTrainer(None, conv_precision="bf16", attn_precision=None)


def test_the_state_dict_does_not_hold_the_precision():
    a, b = ldh.LinearAttention(64), ldh.LinearAttention(64)
    b.attn_precision = "bf16"
    assert list(a.state_dict()) == list(b.state_dict()) and "attn_precision" not in "".join(b.state_dict())
    a.load_state_dict(b.state_dict())
    assert a.attn_precision == "fp32"
    net = ldh.TrainableUnet(**MNIST, attn_precision="bf16")
    assert list(net.state_dict()) == list(ldh.TrainableUnet(**MNIST).state_dict())


def test_the_packed_weights_do_not_depend_on_the_precision():
    """``_packed_for`` keeps its copies when ``attn_precision`` changes (a stand-in ``_pack`` counts; no GPU)."""
    mod = ldh.LinearAttention(32)
    calls = []
    mod._pack = lambda dev: calls.append(mod.attn_precision) or len(calls)
    assert mod._packed_for("d") == 1
    mod.attn_precision = "bf16"
    assert mod._packed_for("d") == 1
    mod.attn_precision = "fp32"
    assert mod._packed_for("d") == 1 and calls == ["fp32"]
    mod.conv_precision = "bf16"                          # (the convolutions' switch does repack)
    assert mod._packed_for("d") == 2


def test_the_unet_hands_the_precision_to_linear_attention_only():
    net = ldh.TrainableUnet(**MNIST)
    lin = [m for m in net.modules() if isinstance(m, ldh.LinearAttention)]
    full = [m for m in net.modules() if isinstance(m, ldh.Attention)]
    assert len(lin) == 4 and len(full) == 3 and net.attn_precision == "fp32"
    net.attn_precision = "bf16"
    assert net.attn_precision == "bf16" and all(m.attn_precision == "bf16" for m in lin)
    assert all(m.attn_precision == "fp32" for m in full)
    assert net.conv_precision == "fp32" and net.act_storage == "fp32"
    assert all(m.conv_precision == "fp32" for m in net.modules() if hasattr(type(m), "conv_precision"))
    for bad in BAD:
        with pytest.raises(ValueError, match="attn_precision"):
            net.attn_precision = bad
    assert net.attn_precision == "bf16" and all(m.attn_precision == "bf16" for m in lin)
    net.attn_precision = "fp32"
    assert all(m.attn_precision == "fp32" for m in lin)
    made = ldh.TrainableUnet(**MNIST, attn_precision="bf16", conv_precision="bf16")
    assert all(m.attn_precision == "bf16" for m in made.modules() if isinstance(m, ldh.LinearAttention))
    made.conv_precision = "fp32"                         # neither switch moves the other
    assert made.attn_precision == "bf16" and all(m.attn_precision == "bf16" for m in made.modules()
                                                 if isinstance(m, ldh.LinearAttention))


# ------------------------------------------------------------------------------------------------ 2. the entry points
def test_the_four_symbols_are_exported():
    lib = cabi.lib()
    for name in NAMES:
        assert callable(getattr(lib, f"ld_dn_la_{name}16")) and callable(ENTRY[name])


@pytest.mark.parametrize("suffix", ["", "16"])
def test_refusals_need_no_gpu(suffix):
    """Each bf16 entry point returns -1 for what its fp32 sibling refuses (both are run on the same arguments; nothing is
    launched and no pointer is dereferenced)."""
    lib = cabi.lib()
    p = 1 << 20
    ctx, out, red, app = (getattr(lib, f"ld_dn_la_{n}{suffix}") for n in NAMES)
    for kw in (dict(heads=0), dict(B=0), dict(H=0), dict(ld3=64), dict(ld3=130), dict(qkv=None), dict(work=None), dict(qkv=p + 4)):
        a = dict(qkv=p, work=p, ctx=p, kstat=p, B=1, H=4, W=4, heads=1, ld3=128)
        a.update(kw)
        assert ctx(a["qkv"], a["work"], a["ctx"], a["kstat"], a["B"], a["H"], a["W"], a["heads"], a["ld3"], None) == -1, kw
    for kw in (dict(ld3=64), dict(ldo=16), dict(ldo=66), dict(out=None), dict(ctx=p + 8), dict(heads=0), dict(W=0)):
        a = dict(qkv=p, ctx=p, out=p, B=1, H=4, W=4, heads=1, ld3=128, ldo=64)
        a.update(kw)
        assert out(a["qkv"], a["ctx"], a["out"], a["B"], a["H"], a["W"], a["heads"], a["ld3"], a["ldo"], None) == -1, kw
    for kw in (dict(rk=None), dict(dout=p + 4), dict(ld3=64), dict(ldo=16), dict(heads=0), dict(work=None)):
        a = dict(qkv=p, dout=p, ctx=p, work=p, dctx=p, rk=p, B=1, H=4, W=4, heads=1, ld3=128, ldo=64)
        a.update(kw)
        assert red(a["qkv"], a["dout"], a["ctx"], a["work"], a["dctx"], a["rk"], a["B"], a["H"], a["W"], a["heads"], a["ld3"],
                   a["ldo"], None) == -1, kw
    for kw in (dict(dout=p + 4), dict(dqkv=None), dict(kstat=None), dict(dctx=p + 4), dict(ld3=92), dict(ldo=0), dict(B=70000)):
        a = dict(qkv=p, dout=p, ctx=p, kstat=p, dctx=p, rk=p, dqkv=p, B=1, H=4, W=4, heads=1, ld3=128, ldo=64)
        a.update(kw)
        assert app(a["qkv"], a["dout"], a["ctx"], a["kstat"], a["dctx"], a["rk"], a["dqkv"], a["B"], a["H"], a["W"], a["heads"],
                   a["ld3"], a["ldo"], None) == -1, kw
    assert b"ld_dn_la_backward_apply" + suffix.encode() in lib.ld_last_error()


# ------------------------------------------------------------------------------------------------ 3. the reference
def test_core16_without_rounding_is_the_oracles_core():
    """``core16`` with the identity as its rounding, in fp64: the oracle's formulas and autograd through them."""
    B, heads, H, W = 2, 2, 5, 4
    qkv, dout = R.uniform((B, 96 * heads, H, W), 3, -2.0, 2.0), R.uniform((B, 32 * heads, H, W), 4)
    got, ref = P.core16(qkv, heads, dout, None, F64, P._same), R.core(qkv, heads, dout, F64)
    hid = 32 * heads
    for name, want in (("out", ref["out"]), ("ctx", ref["ctx"]), ("m", ref["m"]), ("Z", ref["Z"]), ("dctx", ref["dctx"]),
                       ("dq", ref["dqkv"][:, :hid].reshape(got.dq.shape))):
        assert torch.allclose(getattr(got, name), want, rtol=0, atol=1e-13), name
    # dk, dv and rk go through what the kernels keep as fp32 (1 / Z, the stored dctx): a few 2^-24, no more
    assert R.rel_err(got.dqkv[:, hid:], ref["dqkv"][:, hid:]) < 2.0 ** -21
    assert R.rel_err(got.rk, (ref["dctx"] * ref["ctx"]).sum(-1)) < 2.0 ** -21


def test_core16_rounds_the_operands_the_contract_names_and_reads_what_it_is_given():
    B, heads, H, W = 1, 1, 4, 4
    qkv, dout = R.uniform((B, 96, H, W), 5, -2.0, 2.0), R.uniform((B, 32, H, W), 6)
    r, plain = P.core16(qkv, heads, dout, None, F64), P.core16(qkv, heads, dout, None, F64, P._same)
    assert torch.equal(r.m, plain.m) and torch.equal(r.Z, plain.Z)                    # Z sums the unrounded P
    for name in ("ctx", "out", "dctx", "dq", "dk", "dv"):
        e = R.rel_err(getattr(r, name), getattr(plain, name))
        assert 1e-5 < e < 2e-2, (name, e)                                             # a few 2^-9
    _, k, v = P.split(qkv, heads, F64)
    pk = (k - k.amax(-1, keepdim=True)).exp()
    want = torch.einsum("bhdn,bhen->bhde", P.q(pk.float()).double(), P.q(v.float()).double()) / pk.sum(-1)[..., None]
    assert torch.equal(r.ctx, want)
    given = dict(ctx=torch.ones(B, heads, 32, 32), m=r.m.float(), Z=2 * r.Z.float(), dctx=torch.ones(B, heads, 32, 32),
                 rk=torch.zeros(B, heads, 32))
    g = P.core16(qkv, heads, dout, given, F64)
    assert torch.equal(g.ctx, r.ctx) and torch.equal(g.dctx, r.dctx)                  # a pass's own results do not move
    assert torch.allclose(g.out, torch.full_like(g.out, P.SCALE), rtol=2.0 ** -7, atol=0)      # sum_d rnd(p) = 1 up to bf16
    ks = (k - r.m[..., None]).exp() * (1.0 / given["Z"]).double()[..., None]
    assert torch.equal(g.dv, P.q(ks.float()).double().sum(dim=-2, keepdim=True).expand_as(g.dv).reshape(g.dv.shape))


def test_the_module_on_core16_differs_from_the_oracle_by_the_rounding():
    B, dim, heads, H, W = 2, 32, 2, 5, 4
    sd = R.make_attn(dim, heads, key=7)
    x, dout = R.uniform((B, dim, H, W), 8), R.uniform((B, dim, H, W), 9)
    o16, g16 = P.yardstick16(sd, x, dout, heads, F64)
    o64, g64 = R.yardstick(sd, x, dout, heads, dtype=F64)
    assert set(g16) == set(g64) and 1e-5 < R.rel_err(o16, o64) < 2e-2
    for k in g64:
        assert 1e-5 < R.rel_err(g16[k], g64[k]) < 5e-2, k


# ------------------------------------------------------------------------------------------------ 4. the probes
@pytest.mark.parametrize("shape", P.PROBE_SHAPES)
@pytest.mark.parametrize("kind", P.PROBE_KINDS)
def test_probes(shape, kind):
    """Every precondition is asserted inside the builder: P = 1, p = 1 / 32, ks = 1 / n, sums below 2^24, fp32 == fp64, and
    a missing or truncating rounding moves what the probed operand feeds by more than 2^-12."""
    B, heads, H, W = shape
    pr = P.probe(shape, kind)
    assert pr.want.ctx.shape == (B, heads, 32, 32) and pr.want.out.shape == (B, 32 * heads, H, W)
    assert torch.equal(pr.want.kstat[..., 1], torch.full((B, heads, 32), float(H * W)))
    assert bool(pr.want.ctx.any()) and bool(pr.want.dctx.any()) and bool(pr.want.dv.any())


def test_the_bound_holds_for_a_torch_emulation_of_the_contract():
    """``bounds`` against fp32 torch with rounded operands on one small case: the emulation is inside, the unrounded fp32
    result is what the bound is measured from."""
    B, heads, H, W = 2, 2, 7, 5
    qkv, dout = R.uniform((B, 96 * heads, H, W), 11, -2.0, 2.0), R.uniform((B, 32 * heads, H, W), 12)
    ref = P.core16(qkv, heads, dout, None, F64, P._same)
    given = dict(ctx=ref.ctx.float(), m=ref.m.float(), Z=ref.Z.float(), dctx=ref.dctx.float(), rk=ref.rk.float())
    ref = P.core16(qkv, heads, dout, given, F64, P._same)
    emu = P.core16(qkv, heads, dout, given, F32)
    bd = P.bounds(ref)
    for name in ("ctx", "out", "dctx", "dq", "dk", "dv"):
        ratio = float(((getattr(emu, name).double() - getattr(ref, name)).abs() / getattr(bd, name)).max())
        assert 0.0 < ratio < 1.0, (name, ratio)
