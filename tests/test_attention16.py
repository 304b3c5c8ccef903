"""CPU tests of ``full_attn_precision``: the switch's defaults and refusals on ``Attention``, ``TrainableUnet`` and
``DenoiserTrainer``, the two bf16 entry points' argument validation, and the yardstick of tests/attention16_ref.py --
``core16`` against the oracle's formulas, and the preconditions of every exact probe at every shape
tests/test_hip_attention16.py compares on the GPU.  No GPU."""
import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi

import attention16_ref as P
import attention_ref as R

F32, F64 = torch.float32, torch.float64
MNIST = dict(dim=32, dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist")
BAD = ("fp16", "fp8", None, 1)
# What this file is about: without the two entry points and the attribute nothing below says anything, so it does not load.
ENTRY = {n: getattr(cabi.lib(), f"ld_dn_fa_{n}16") for n in ("forward", "backward")}
assert ldh.Attention.FULL_ATTN_PRECISIONS == ("fp32", "bf16")


# ------------------------------------------------------------------------------------------------ 1. the attribute
def test_full_attn_precision_defaults_and_refusals():
    fa, la = ldh.Attention(32), ldh.LinearAttention(32)
    assert ldh.Attention.full_attn_precision == "fp32" and fa.full_attn_precision == "fp32"
    assert "full_attn_precision" not in vars(fa)                                 # a class attribute until it is set
    assert not hasattr(la, "full_attn_precision") and not hasattr(ldh.LinearAttention, "FULL_ATTN_PRECISIONS")
    for bad in BAD:
        with pytest.raises(ValueError, match="full_attn_precision"):
            fa.full_attn_precision = bad
    assert fa.full_attn_precision == "fp32" and "full_attn_precision" not in vars(fa)
    fa.full_attn_precision = "bf16"
    assert fa.full_attn_precision == "bf16"
    for bad in BAD:
        with pytest.raises(ValueError, match="full_attn_precision"):
            fa.full_attn_precision = bad
    assert fa.full_attn_precision == "bf16"                                      # a refused value leaves the old one
    assert fa.attn_precision == "fp32" and fa.conv_precision == "fp32"           # the other switches are their own
    with pytest.raises(ValueError, match="attn_precision"):
        fa.attn_precision = "bf16"                                               # ... and that one still refuses
    fa.conv_precision = "bf16"
    assert fa.full_attn_precision == "bf16"
    fa.full_attn_precision = "fp32"
    assert fa.full_attn_precision == "fp32" and fa.conv_precision == "bf16"
    with pytest.raises(ValueError, match="full_attn_precision"):
        ldh.TrainableUnet(**MNIST, full_attn_precision="fp8")
    with pytest.raises(ValueError, match="full_attn_precision"):
        ldh.DenoiserTrainer(None, full_attn_precision="fp16")
    with pytest.raises(ValueError, match="full_attn_precision"):                 # independent of the others: refused by itself
        ldh.DenoiserTrainer(None, conv_precision="bf16", attn_precision="bf16", full_attn_precision=None)


def test_the_state_dict_does_not_hold_the_precision():
    a, b = ldh.Attention(64), ldh.Attention(64)
    b.full_attn_precision = "bf16"
    assert list(a.state_dict()) == list(b.state_dict()) and "precision" not in "".join(b.state_dict())
    a.load_state_dict(b.state_dict())
    assert a.full_attn_precision == "fp32"
    net = ldh.TrainableUnet(**MNIST, full_attn_precision="bf16")
    assert list(net.state_dict()) == list(ldh.TrainableUnet(**MNIST).state_dict())


def test_the_packed_weights_do_not_depend_on_the_precision():
    """``_packed_for`` keeps its copies when ``full_attn_precision`` changes (a stand-in ``_pack`` counts; no GPU)."""
    mod = ldh.Attention(32)
    calls = []
    mod._pack = lambda dev: calls.append(mod.full_attn_precision) or len(calls)
    assert mod._packed_for("d") == 1
    mod.full_attn_precision = "bf16"
    assert mod._packed_for("d") == 1
    mod.full_attn_precision = "fp32"
    assert mod._packed_for("d") == 1 and calls == ["fp32"]
    mod.conv_precision = "bf16"                          # (the convolutions' switch does repack)
    assert mod._packed_for("d") == 2


def test_the_unet_hands_the_precision_to_full_attention_only():
    net = ldh.TrainableUnet(**MNIST)
    lin = [m for m in net.modules() if isinstance(m, ldh.LinearAttention)]
    full = [m for m in net.modules() if isinstance(m, ldh.Attention)]
    assert len(lin) == 4 and len(full) == 3 and net.full_attn_precision == "fp32"
    assert not any("full_attn_precision" in vars(m) for m in net.modules())      # the default hands nothing down
    net.full_attn_precision = "bf16"
    assert net.full_attn_precision == "bf16" and all(m.full_attn_precision == "bf16" for m in full)
    assert not any(hasattr(m, "full_attn_precision") for m in net.modules() if m is not net and not isinstance(m, ldh.Attention))
    assert net.attn_precision == "fp32" and all(m.attn_precision == "fp32" for m in lin + full)
    assert net.conv_precision == "fp32" and net.act_storage == "fp32"
    assert all(m.conv_precision == "fp32" for m in net.modules() if hasattr(type(m), "conv_precision"))
    for bad in BAD:
        with pytest.raises(ValueError, match="full_attn_precision"):
            net.full_attn_precision = bad
    assert net.full_attn_precision == "bf16" and all(m.full_attn_precision == "bf16" for m in full)
    net.attn_precision = "bf16"                          # the existing setter: LinearAttention only, and not this switch
    assert all(m.attn_precision == "bf16" for m in lin) and all(m.attn_precision == "fp32" for m in full)
    assert all(m.full_attn_precision == "bf16" for m in full)
    net.full_attn_precision = "fp32"
    assert all(m.full_attn_precision == "fp32" for m in full) and all(m.attn_precision == "bf16" for m in lin)
    net.attn_precision = "fp32"
    assert all(m.full_attn_precision == "fp32" for m in full)
    made = ldh.TrainableUnet(**MNIST, full_attn_precision="bf16", conv_precision="bf16")
    assert all(m.full_attn_precision == "bf16" for m in made.modules() if isinstance(m, ldh.Attention))
    made.conv_precision = "fp32"                         # neither switch moves the other
    assert made.full_attn_precision == "bf16" and made.attn_precision == "fp32"
    assert all(m.full_attn_precision == "bf16" for m in made.modules() if isinstance(m, ldh.Attention))


# ------------------------------------------------------------------------------------------------ 2. the entry points
def test_the_two_symbols_are_exported():
    lib = cabi.lib()
    for name in ENTRY:
        assert callable(getattr(lib, f"ld_dn_fa_{name}16")) and callable(ENTRY[name])


@pytest.mark.parametrize("suffix", ["", "16"])
def test_refusals_need_no_gpu(suffix):
    """Each bf16 entry point returns -1 for what its fp32 sibling refuses (both are run on the same arguments; nothing is
    launched and no pointer is dereferenced)."""
    lib = cabi.lib()
    p = 1 << 20
    fwd, bwd = (getattr(lib, f"ld_dn_fa_{n}{suffix}") for n in ("forward", "backward"))
    for kw, word in ((dict(qkv=None), b"null"), (dict(out=None), b"null"), (dict(qkv=p + 4), b"aligned"), (dict(out=p + 8), b"aligned"),
                     (dict(lse=p + 2), b"aligned"), (dict(heads=0), b"heads"), (dict(ld3=64), b"ld3"), (dict(ld3=130), b"ld3"),
                     (dict(ldo=16), b"ldo"), (dict(ldo=66), b"ldo"), (dict(H=0), b"H=0"), (dict(W=0), b"W=0"), (dict(B=0), b"B=0"),
                     (dict(B=70000), b"B=70000")):
        a = dict(qkv=p, out=p, lse=p, B=1, H=4, W=4, heads=1, ld3=128, ldo=64)
        a.update(kw)
        assert fwd(a["qkv"], a["out"], a["lse"], a["B"], a["H"], a["W"], a["heads"], a["ld3"], a["ldo"], None) == -1, kw
        err = lib.ld_last_error()
        assert word in err and b"ld_dn_fa_forward" + suffix.encode() in err, (kw, err)
    for kw, word in ((dict(qkv=None), b"null"), (dict(out=None), b"null"), (dict(dout=None), b"null"), (dict(lse=None), b"null"),
                     (dict(work=None), b"null"), (dict(dqkv=None), b"null"), (dict(dout=p + 4), b"aligned"),
                     (dict(dqkv=p + 8), b"aligned"), (dict(work=p + 1), b"aligned"), (dict(heads=0), b"heads"), (dict(heads=2), b"ld3"),
                     (dict(ld3=92), b"ld3"), (dict(ldo=62), b"ldo"), (dict(ldo=0), b"ldo"), (dict(W=0), b"W=0")):
        a = dict(qkv=p, out=p, dout=p, lse=p, work=p, dqkv=p, B=1, H=4, W=4, heads=1, ld3=128, ldo=64)
        a.update(kw)
        assert bwd(a["qkv"], a["out"], a["dout"], a["lse"], a["work"], a["dqkv"], a["B"], a["H"], a["W"], a["heads"], a["ld3"],
                   a["ldo"], None) == -1, kw
        err = lib.ld_last_error()
        assert word in err and b"ld_dn_fa_backward" + suffix.encode() in err, (kw, err)


# ------------------------------------------------------------------------------------------------ 3. the reference
def test_core16_without_rounding_is_the_oracles_core():
    """``core16`` with the identity as its rounding, in fp64: the oracle's formulas and autograd through them."""
    B, heads, H, W = 2, 2, 5, 4
    qkv, dout = R.uniform((B, 96 * heads, H, W), 3, -2.0, 2.0), R.uniform((B, 32 * heads, H, W), 4)
    got, ref = P.core16(qkv, heads, dout, None, F64, P._same), R.core(qkv, heads, dout, F64)
    # (the kernels' constant is the fp32 32^-0.5: 2^-25 relative away from the oracle's)
    assert R.rel_err(got.out, ref["out"]) < 1e-6 and R.rel_err(got.lse, ref["lse"]) < 1e-6
    assert R.rel_err(got.dqkv, ref["dqkv"]) < 1e-6
    for i in range(3):
        sl = slice(64 * i, 64 * (i + 1))
        assert R.rel_err(got.dqkv[:, sl], ref["dqkv"][:, sl]) < 1e-6, i


def test_core16_rounds_the_operands_the_contract_names_and_reads_what_it_is_given():
    B, heads, H, W = 1, 1, 4, 4
    qkv, dout = R.uniform((B, 96, H, W), 5, -2.0, 2.0), R.uniform((B, 32, H, W), 6)
    r, plain = P.core16(qkv, heads, dout, None, F64), P.core16(qkv, heads, dout, None, F64, P._same)
    for name in ("out", "lse", "dq", "dk", "dv"):
        e = R.rel_err(getattr(r, name), getattr(plain, name))
        assert 1e-5 < e < 2e-2, (name, e)                                             # a few 2^-9
    qq, k, v = P.split(qkv, heads, F64)
    a = torch.einsum("bhci,bhcj->bhij", P.q(qq.float()).double(), P.q(k.float()).double()) * P.SCALE
    pu = (a - a.amax(-1, keepdim=True)).exp()
    assert torch.equal(r.lse, a.amax(-1) + pu.sum(-1).log())                          # l sums the unrounded p
    want = torch.einsum("bhij,bhcj->bhci", P.q(pu.float()).double(), P.q(v.float()).double()) / pu.sum(-1)[:, :, None, :]
    assert torch.equal(r.out, want.reshape(r.out.shape))
    given = dict(lse=(r.lse + 1.0).float(), out=torch.zeros(B, 32, H, W))             # p / e, delta = 0
    g = P.core16(qkv, heads, dout, given, F64)
    assert torch.equal(g.out, r.out) and torch.equal(g.lse, r.lse)                    # the forward's own results do not move
    assert bool((g.delta == 0).all())
    p = (a - given["lse"].double()[..., None]).exp()
    dO = dout.reshape(B, heads, 32, H * W).double()
    assert torch.equal(g.dv, torch.einsum("bhij,bhci->bhcj", P.q(p.float()).double(), P.q(dO.float()).double()))
    dP = torch.einsum("bhci,bhcj->bhij", P.q(dO.float()).double(), P.q(v.float()).double())
    assert torch.equal(g.dq, P.SCALE * torch.einsum("bhij,bhcj->bhci", P.q((p * dP).float()).double(), P.q(k.float()).double()))


def test_core16_as_an_autograd_function_is_core16():
    B, heads, H, W = 2, 2, 3, 5
    qkv, dout = R.uniform((B, 96 * heads, H, W), 13, -2.0, 2.0).double(), R.uniform((B, 32 * heads, H, W), 14).double()
    leaf = qkv.clone().requires_grad_(True)
    out = P.Core16.apply(leaf, heads)
    (g,) = torch.autograd.grad(out, [leaf], grad_outputs=dout)
    fw = P.core16(qkv, heads, None, None, F64)
    r = P.core16(qkv, heads, dout, dict(lse=fw.lse.float(), out=fw.out.float()), F64)
    assert torch.equal(out.detach(), r.out) and torch.equal(g, r.dqkv)


def test_the_module_on_core16_differs_from_the_oracle_by_the_rounding():
    B, dim, heads, H, W = 2, 32, 2, 5, 4
    sd = R.make_attn(dim, heads, key=7)
    x, dout = R.uniform((B, dim, H, W), 8), R.uniform((B, dim, H, W), 9)
    o16, g16 = P.yardstick16(sd, x, dout, heads, F64)
    o64, g64 = R.yardstick(sd, x, dout, heads, dtype=F64)
    assert set(g16) == set(g64) and 1e-5 < R.rel_err(o16, o64) < 2e-2
    for k in g64:                                                                     # (the bias gradient does not pass the core)
        assert (0.0 if k == "to_out.bias" else 1e-5) <= R.rel_err(g16[k], g64[k]) < 5e-2, k
    o, g = P.yardstick16(sd, x, dout, heads, F64)                                     # (and it is a function of its inputs)
    assert torch.equal(o, o16) and all(torch.equal(g[k], g16[k]) for k in g)


# ------------------------------------------------------------------------------------------------ 4. the probes
def test_the_case_lists_are_the_fp32_tests_plus_a_single_pixel():
    assert P.CORE_CASES[-1] == (1, 1, 1, 1, False) and sorted({c[2] * c[3] for c in P.CORE_CASES}) == [1, 15, 64, 65, 196, 1023]
    assert {c[1] for c in P.CORE_CASES} == {1, 2, 4} and sum(c[4] for c in P.CORE_CASES) == 1


@pytest.mark.parametrize("shape", P.PROBE_SHAPES)
@pytest.mark.parametrize("kind", P.FORWARD_KINDS)
def test_forward_probes(shape, kind):
    """Every precondition is asserted inside the builder: one logit per row, integer sums below 2^24, fp32 == fp64 up to the
    one trailing operation, and a missing or truncating rounding moves what the probed operand feeds by more than 2^-12."""
    B, heads, H, W = shape
    pr = P.forward_probe(shape, kind)
    assert pr.want.out.shape == (B, 32 * heads, H, W) and pr.want.lse.shape == (B, heads, H * W)
    assert pr.want.out.dtype == F64 and pr.want.lse.dtype == F64
    assert bool(pr.want.out.any()) and bool(torch.isfinite(pr.want.lse).all())


@pytest.mark.parametrize("shape", P.PROBE_SHAPES)
@pytest.mark.parametrize("kind", P.BACKWARD_KINDS)
def test_backward_probes(shape, kind):
    """p = 1 on every pair and delta = 0 in fp32, ds = dP an integer, every sum of magnitudes below 2^24, dv an exact integer,
    and a missing or truncating rounding shows on what the probed operand feeds."""
    B, heads, H, W = shape
    pr = P.backward_probe(shape, kind)
    for name in ("dq", "dk", "dv"):
        t = getattr(pr.want, name)
        assert t.shape == (B, heads, 32, H * W) and t.dtype == F64 and bool(t.any()), name
    assert bool((pr.given["out"] == 0).all()) and pr.given["lse"].dtype == F32
