"""The CPU yardstick of the two attention cores on the fp16 matrix cores (``amp_attn="fp16"``: the ``<f16>`` instantiations of
csrc/linattn16.hip and csrc/attention16.hip).  Pure torch, no GPU import.

* The rounding is ``amp_ref.h``: to fp16, nearest even, beyond 65504 inf.
* The full core is ``attention16_ref.core16(..., rnd=h)``: the bf16 contract with the other rounding.
* The linear core is restated here (``la_core``), because one operand pair differs from the bf16 contract: the dv product of
  the apply pass is ``sum_d h(dctx[d, e] iz[d]) h(exp(k[d, n] - m[d]))`` (``fold=True``), the division by Z moved to the dctx
  side, where the bf16 kernel rounds ``ks = exp(k - m) iz``.  ``fold=False`` is the bf16 contract at any rounding, what the
  fold is compared against.
* ``LaCore`` / ``FaCore`` are the cores as ``autograd.Function``s and ``la_yardstick`` / ``fa_yardstick`` the modules around
  them.
* The probes follow ``linattn16_ref.probe`` and ``attention16_ref.forward_probe`` / ``backward_probe``.  The operand under
  test holds ``amp_ref.fp16_ties``: integers in [257, 2047], which fp16 holds and bf16 does not, mixed with odd integers in
  [2049, 4095], exact fp16 ties.  Every builder asserts that every sum is an integer (times one trailing factor) below
  2^24, and that bf16 rounding, truncation (to fp16's and to bf16's bits) and no rounding each give another expectation, by
  more than ``SHOWS`` relative somewhere, which is 8 times what the GPU tests tolerate.  (The single-pixel shape leaves a
  probe one logit or one dP to show that on: the builders' default keys are ones at which it does.)
"""
import math
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

import attention16_ref as FA
import linattn16_ref as LA
from amp_ref import fp16_ties, h, trunc16
from conv16_ref import _same, q, trunc
from exact_probes import ints, is_integer, trits
from oracle import unet_ref

F32, F64 = torch.float32, torch.float64
D = 32
LIMIT = 2.0 ** 24
SHOWS = 2.0 ** -18                       # a wrong rounding moves an expectation by more than this, relative, somewhere
OTHERS = (q, _same, trunc16, trunc)     # what a kernel could do instead of rounding to fp16

LA_CORE_CASES = LA.CORE_CASES
LA_PROBE_SHAPES = LA.PROBE_SHAPES
LA_PROBE_KINDS = LA.PROBE_KINDS
LA_MODULE_CASES = LA.MODULE_CASES
LA_SUBNORMAL_CASE = (1, 1, 128, 128)     # the smallest map at which ks = exp(k - m) / Z reaches fp16's subnormals
FA_CORE_CASES = FA.CORE_CASES
FA_PROBE_SHAPES = FA.PROBE_SHAPES
FA_FORWARD_KINDS = FA.FORWARD_KINDS
FA_BACKWARD_KINDS = FA.BACKWARD_KINDS
FA_MODULE_CASES = FA.MODULE_CASES

_r = LA._r


def shows(a, b):
    """Somewhere ``a`` is off from ``b`` by more than ``SHOWS`` relative."""
    return bool(((a.double() - b.double()).abs() > SHOWS * b.double().abs()).any())


def power_of_two(n):
    return n & (n - 1) == 0


# --------------------------------------------------------------------------------------------- the linear core
def la_core(qkv, heads, dout, given=None, dtype=F32, rnd=h, fold=True):
    """``linattn16_ref.core16`` with ``rnd`` on the same operands, and with ``fold`` the fp16 kernels' dv product:
    ``rnd(dctx iz)`` against ``rnd(exp(k - m))`` (the product ``dctx iz`` is an fp32 multiplication in the kernel; ``_r``
    rounds through fp32).  Without ``fold`` it is that function."""
    r = LA.core16(qkv, heads, dout, given, dtype, rnd)
    if not fold:
        return r
    given = given or {}
    b, _, hh, ww = qkv.shape
    _, k, _ = LA.split(qkv, heads, dtype)
    m, Z = (given.get(name, getattr(r, name)).to(dtype) for name in ("m", "Z"))
    dctx = given.get("dctx", r.dctx).to(dtype)
    iz = (1.0 / Z.float()).to(dtype)
    pk = (k - m[..., None]).exp()
    r.dv = torch.einsum("bhde,bhdn->bhen", _r(rnd, dctx * iz[..., None], dtype), _r(rnd, pk, dtype))
    r.dqkv = torch.cat([t.reshape(b, heads * D, hh, ww) for t in (r.dq, r.dk, r.dv)], dim=1)
    r.parts.pk, r.parts.iz = pk, iz
    return r


class LaCore(torch.autograd.Function):
    """``linattn16_ref.Core16`` on ``la_core`` (fp16 rounding, the folded dv)."""

    @staticmethod
    def forward(c, qkv, heads):
        zero = torch.zeros_like(qkv[:, :heads * D])
        r = la_core(qkv, heads, zero, dtype=qkv.dtype)
        c.heads = heads
        c.save_for_backward(qkv, r.ctx.float(), r.m.float(), r.Z.float())
        return la_core(qkv, heads, zero, dict(ctx=r.ctx.float()), qkv.dtype).out

    @staticmethod
    def backward(c, dout):
        qkv, ctx, m, Z = c.saved_tensors
        r = la_core(qkv, c.heads, dout, dict(ctx=ctx, m=m, Z=Z), qkv.dtype)
        r = la_core(qkv, c.heads, dout, dict(ctx=ctx, m=m, Z=Z, dctx=r.dctx.float(), rk=r.rk.float()), qkv.dtype)
        return r.dqkv, None


class FaCore(torch.autograd.Function):
    """``attention16_ref.Core16`` with fp16 rounding."""

    @staticmethod
    def forward(c, qkv, heads):
        r = FA.core16(qkv, heads, None, dtype=qkv.dtype, rnd=h)
        c.heads = heads
        c.save_for_backward(qkv, r.lse.float(), r.out.float())
        return r.out

    @staticmethod
    def backward(c, dout):
        qkv, lse, out = c.saved_tensors
        return FA.core16(qkv, c.heads, dout, dict(lse=lse, out=out), qkv.dtype, h).dqkv, None


def _leaves(sd, x, dtype):
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    return leaves, x.detach().to(dtype).clone().requires_grad_(True)


def la_yardstick(sd, x, dout, heads, dtype=F64):
    """``linattn16_ref.yardstick16`` with ``LaCore``: out and {"x", parameter name: gradient} of sum(out * dout)."""
    leaves, xin = _leaves(sd, x, dtype)
    y = unet_ref.rms_norm(xin, leaves["norm.g"])
    core = LaCore.apply(F.conv2d(y, leaves["to_qkv.weight"]), heads)
    out = unet_ref.rms_norm(F.conv2d(core, leaves["to_out.0.weight"], leaves["to_out.0.bias"]), leaves["to_out.1.g"])
    grads = torch.autograd.grad(out, [xin] + list(leaves.values()), grad_outputs=dout.to(dtype))
    return out.detach(), dict(zip(["x"] + list(leaves), grads))


def fa_yardstick(sd, x, dout, heads, dtype=F64):
    """``attention16_ref.yardstick16`` with ``FaCore``."""
    leaves, xin = _leaves(sd, x, dtype)
    y = unet_ref.rms_norm(xin, leaves["norm.g"])
    core = FaCore.apply(F.conv2d(y, leaves["to_qkv.weight"]), heads)
    out = F.conv2d(core, leaves["to_out.weight"], leaves["to_out.bias"])
    grads = torch.autograd.grad(out, [xin] + list(leaves.values()), grad_outputs=dout.to(dtype))
    return out.detach(), dict(zip(["x"] + list(leaves), grads))


# --------------------------------------------------------------------------------------------- the linear core's probes
def la_probe(shape, kind, key=18000):
    """``linattn16_ref.probe`` for fp16: k constant per channel (P = 1, Z = n, ks = 1 / n), q constant per pixel (p = 1 / 32);
    ``kind`` names the memory operand (v, dO, ctx, dctx) that holds ``fp16_ties``, the other three hold {-1, 0, 1}.

    The folded dv is ``sum_d h(dctx[d, e] / n)``: where n is a power of two the division is exact and dv has a bit-exact
    expectation (``want.dv``, ``dv_exact``); elsewhere ``dctx / n`` is rounded a second time, and dv is held to
    ``want.dv_bound`` around ``want.dv`` = the fp64 sum of the unrounded ``dctx / n``: one fp16 rounding of a term (2^-11)
    plus the fp32 product in front of it and the fp32 sum of 32 terms (2^-21 together, generously)."""
    B, heads, H, W = shape
    n = H * W
    key += 1000 * LA_PROBE_KINDS.index(kind) + 100 * heads + 10 * H + W
    hs, ms = (B, heads, D, n), (B, heads, D, D)

    def operand(name, shp, k):
        return fp16_ties(shp, k) if kind == name else trits(shp, k)

    v, dO = operand("v", hs, key), operand("dO", hs, key + 10)
    ctx, dctx = operand("ctx", ms, key + 20), operand("dctx", ms, key + 30)
    kc = ints((B, heads, D, 1), key + 40, -3, 3) / 4
    qc = ints((B, heads, 1, n), key + 41, -3, 3) / 4
    rk = ints((B, heads, D), key + 42, -8, 8)
    qkv = torch.cat([t.reshape(B, heads * D, H, W) for t in (qc.expand(hs), kc.expand(hs), v)], dim=1).contiguous()
    dout = dO.reshape(B, heads * D, H, W).contiguous()
    m, Z = kc[..., 0].clone(), torch.full((B, heads, D), float(n))
    given = dict(ctx=ctx, m=m, Z=Z, dctx=dctx, rk=rk)
    qq, kk, _ = LA.split(qkv, heads, F32)
    e = (qq - qq.amax(dim=-2, keepdim=True)).exp()
    assert bool((e == 1).all()) and bool((e.sum(dim=-2) == 32.0).all()) and bool((qq.softmax(dim=-2) == 1 / 32).all())
    assert bool(((kk - m[..., None]).exp() == 1).all())

    def run(rnd, dt):
        return la_core(qkv, heads, dout, given, dt, rnd)

    r32, r64 = run(h, F32), run(h, F64)
    assert torch.equal(r64.Z, Z.double()) and torch.equal(r64.m, m.double())
    assert bool((r32.parts.pk == 1).all()) and torch.equal(r32.parts.iz, 1.0 / Z)
    ones = torch.ones(hs, dtype=F64)
    raw_ctx = torch.einsum("bhdn,bhen->bhde", ones, h(v).double())                                   # ctx Z
    raw_dctx = torch.einsum("bhdn,bhen->bhde", torch.full(hs, 1 / 32, dtype=F64), h(dO).double())    # dctx / 32^-0.5
    mag = [torch.einsum("bhdn,bhen->bhde", ones, h(v).double().abs()),
           torch.einsum("bhdn,bhen->bhde", ones, h(dO).double().abs()),
           torch.einsum("bhde,bhen->bhdn", h(ctx).double().abs(), h(dO).double().abs()),
           torch.einsum("bhde,bhen->bhdn", h(dctx).double().abs(), h(v).double().abs()),
           torch.einsum("bhde,bhdn->bhen", h(dctx).double().abs(), ones),
           32 * (r64.parts.s.abs() / 32).sum(dim=-2)]
    for t in mag:
        assert float(t.max()) < LIMIT, float(t.max())
    assert is_integer(raw_ctx) and is_integer(32 * raw_dctx) and is_integer(r64.parts.s)
    dv_exact = power_of_two(n)
    for name in ("ctx", "out", "dctx", "dq", "dk") + (("dv",) if dv_exact else ()):
        a, b = getattr(r32, name).double(), getattr(r64, name)
        assert float((a - b).abs().max()) <= 2.0 ** -21 * float(b.abs().max()), name
    want = NS(ctx=(raw_ctx / Z.double()[..., None]).float(), kstat=torch.stack([m, Z], dim=-1),
              dctx=(raw_dctx * LA.SCALE).float(), rk32=r32.rk, rk64=r64.rk, out=r64.out, dq=r64.dq, dk=r64.dk, dv_exact=dv_exact)
    assert torch.equal(want.ctx, r64.ctx.float()) and torch.equal(want.dctx, r64.dctx.float())
    if dv_exact:                       # h(dctx / n) = h(dctx) / n: a sum of integers over n
        want.dv = (h(dctx).double().sum(dim=-2) / n)[..., None].expand(hs).contiguous()
        assert torch.equal(r64.dv, want.dv) and torch.equal(r32.dv.double(), want.dv)
        want.dv_bound = torch.zeros_like(want.dv)
    else:
        want.dv = (dctx.double().sum(dim=-2) / n)[..., None].expand(hs).contiguous()
        want.dv_bound = ((2.0 ** -11 + 2.0 ** -21) * dctx.double().abs().sum(dim=-2) / n)[..., None].expand(hs).contiguous()
        assert bool(((r32.dv.double() - want.dv).abs() <= want.dv_bound).all())
    # a kernel that rounds to bf16, does not round, or truncates, shows on what the probed operand feeds
    feeds = {"v": ("ctx", "dk"), "dO": ("dctx", "dq"), "ctx": ("out", "dq"), "dctx": ("dk",) + (("dv",) if dv_exact else ())}[kind]
    rounded = dict(v=v, dO=dO, ctx=ctx, dctx=dctx)[kind]
    assert not torch.equal(h(rounded), rounded) and not torch.equal(q(rounded), h(rounded))
    for other in OTHERS:
        ro = run(other, F64)
        for name in feeds:
            assert shows(getattr(ro, name), getattr(r64, name)), (kind, name, other.__name__)
    return NS(qkv=qkv, dout=dout, given=given, want=want, heads=heads, kind=kind)


# --------------------------------------------------------------------------------------------- the full core's probes
def _nchw(t, B, heads, H, W):
    return t.reshape(B, heads * D, H, W)


def fa_forward_probe(shape, kind, key=19200):
    """``attention16_ref.forward_probe`` for fp16: k constant over the keys, so p = 1, l = n, out = mean_j(h(v_j)) and lse =
    a + log n.  ``kind`` "v": v holds ``fp16_ties`` (seen through out); "q" / "k": that operand does (seen through lse)."""
    B, heads, H, W = shape
    n = H * W
    key = FA._key(shape, kind, FA_FORWARD_KINDS, key)
    hs = (B, heads, D, n)
    qq = fp16_ties(hs, key) if kind == "q" else trits(hs, key)
    kc = fp16_ties((B, heads, D, 1), key + 10) if kind == "k" else ints((B, heads, D, 1), key + 10, -3, 3)
    v = fp16_ties(hs, key + 20) if kind == "v" else ints(hs, key + 20, -8, 8)
    qkv = torch.cat([_nchw(t, B, heads, H, W) for t in (qq, kc.expand(hs), v)], dim=1).contiguous()

    def run(rnd, dt):
        return FA.core16(qkv, heads, None, None, dt, rnd)

    r32, r64 = run(h, F32), run(h, F64)
    s = torch.einsum("bhci,bhcj->bhij", h(qq).double(), h(kc.expand(hs)).double())
    assert is_integer(s) and bool((s == s[..., :1]).all())
    assert float(torch.einsum("bhci,bhc->bhi", h(qq).double().abs(), h(kc[..., 0]).double().abs()).max()) < LIMIT
    raw = h(v).double().sum(dim=-1)
    assert is_integer(raw) and float(h(v).double().abs().sum(dim=-1).max()) < LIMIT
    a32 = s[..., 0].float() * FA.SCALE
    want = NS(out=_nchw((raw / n)[..., None].expand(hs), B, heads, H, W), lse=a32.double() + math.log(n))
    assert torch.equal(r64.out, want.out)
    assert float((r64.lse - want.lse).abs().max()) <= 2.0 ** -22 * max(1.0, float(want.lse.abs().max()))
    assert float((r32.out.double() - want.out).abs().max()) <= 2.0 ** -21 * float(want.out.abs().max())
    rounded = dict(q=qq, k=kc, v=v)[kind]
    assert not torch.equal(h(rounded), rounded) and not torch.equal(q(rounded), h(rounded))
    name = "out" if kind == "v" else "lse"
    for other in OTHERS:
        assert shows(getattr(run(other, F64), name), getattr(r64, name)), (kind, other.__name__)
    return NS(qkv=qkv, want=want, heads=heads, kind=kind, feeds=name)


def fa_backward_probe(shape, kind, key=20300):
    """``attention16_ref.backward_probe`` for fp16: lse_i is the fp32 logit of row i and out = 0, so p = 1, delta = 0 and ds =
    dP, an integer.  ``kind`` names what holds integers that fp16 rounds: "dO" (dense ties, seen through dv; v has one
    non-zero channel per pixel so that dP stays inside fp16's range), "v" (dense ties; dO holds +1 and -1 on two channels
    of a pixel, dP is a difference of two h(v)), "ds" (dO and v representable -- 2048 or 3072 on even channels, 3 or 7 on
    odd ones -- and dP = +-(2051, 2055, 3075 or 3079): ties that round up, so truncation shows on every one), "q" and "k" (dense ties seen through dk and
    dq; dO on two channels keeps |ds| <= 2 and the sums over 1,023 rows below 2^24)."""
    B, heads, H, W = shape
    n = H * W
    key = FA._key(shape, kind, FA_BACKWARD_KINDS, key)
    hs = (B, heads, D, n)
    ch = torch.arange(D).reshape(1, 1, D, 1)
    qq = fp16_ties(hs, key) if kind == "q" else trits(hs, key)
    kc = fp16_ties((B, heads, D, 1), key + 10) if kind == "k" else ints((B, heads, D, 1), key + 10, -3, 3)
    v = fp16_ties(hs, key + 20) if kind == "v" else trits(hs, key + 20)
    if kind == "dO":
        dO = fp16_ties(hs, key + 30)
        v = (2 * ints((B, heads, 1, n), key + 23, 0, 1) - 1) * (ch == ints((B, heads, 1, n), key + 24, 0, 31).long()).float()
    else:                                                        # dO: two channels of every pixel, an even and an odd one
        c1 = 2 * ints((B, heads, 1, n), key + 31, 0, 15).long()
        c2 = 2 * ints((B, heads, 1, n), key + 32, 0, 15).long() + 1
        sg = 2 * ints((B, heads, 1, n), key + 33, 0, 1) - 1
        dO = sg * ((ch == c1).float() + (1.0 if kind == "ds" else -1.0) * (ch == c2).float())
    if kind == "ds":
        v = torch.where(ch % 2 == 0, 1024 * ints(hs, key + 21, 2, 3), 4 * ints(hs, key + 22, 0, 1) + 3)
    k = kc.expand(hs)
    qkv = torch.cat([_nchw(t, B, heads, H, W) for t in (qq, k, v)], dim=1).contiguous()
    dout = _nchw(dO, B, heads, H, W).contiguous()
    s = torch.einsum("bhci,bhcj->bhij", h(qq).double(), h(k).double())
    assert is_integer(s) and bool((s == s[..., :1]).all())
    assert float(torch.einsum("bhci,bhc->bhi", h(qq).double().abs(), h(kc[..., 0]).double().abs()).max()) < LIMIT
    lse = s[..., 0].float() * FA.SCALE
    given = dict(lse=lse, out=torch.zeros(B, heads * D, H, W))

    def run(rnd, dt, g=given):
        return FA.core16(qkv, heads, dout, g, dt, rnd)

    r32 = run(h, F32)
    assert bool((r32.parts.p == 1).all()) and bool((r32.delta == 0).all())
    dP = torch.einsum("bhci,bhcj->bhij", h(dO).double(), h(v).double())
    assert float(dP.abs().max()) < 65504.0
    dsr = h(dP.float()).double()
    mag = [torch.einsum("bhci,bhcj->bhij", h(dO).double().abs(), h(v).double().abs()),
           torch.einsum("bhij,bhcj->bhci", dsr.abs(), h(k).double().abs()),
           torch.einsum("bhij,bhci->bhcj", dsr.abs(), h(qq).double().abs()),
           h(dO).double().abs().sum(dim=-1)]
    for t in mag:
        assert float(t.max()) < LIMIT, float(t.max())
    assert is_integer(dP) and torch.equal(r32.parts.ds.double(), dP)
    want = NS(dq=FA.SCALE * torch.einsum("bhij,bhcj->bhci", dsr, h(k).double()),
              dk=FA.SCALE * torch.einsum("bhij,bhci->bhcj", dsr, h(qq).double()),
              dv=h(dO).double().sum(dim=-1, keepdim=True).expand(hs).contiguous())
    assert is_integer(want.dv) and torch.equal(r32.dv.double(), want.dv)
    for name in ("dq", "dk"):
        a, b = getattr(r32, name).double(), getattr(want, name)
        assert bool(((a - b).abs() <= 2.0 ** -21 * b.abs()).all()), name
    if kind == "ds":
        assert torch.equal(h(dO), dO) and torch.equal(h(v), v) and not torch.equal(dsr, dP)
        assert not torch.equal(q(dP.float()).double(), dsr)
    else:
        rounded = dict(dO=dO, v=v, q=qq, k=kc)[kind]
        assert not torch.equal(h(rounded), rounded) and not torch.equal(q(rounded), h(rounded))
    feeds = {"dO": ("dv",), "v": ("dq", "dk"), "ds": ("dq", "dk"), "q": ("dk",), "k": ("dq",)}[kind]
    for other in OTHERS:
        so = torch.einsum("bhci,bhcj->bhij", _r(other, qq, F64), _r(other, k, F64))
        ro = run(other, F32, dict(given, lse=so[..., 0].float() * FA.SCALE))          # (its own logits: p = 1 there as well)
        assert bool((ro.parts.p == 1).all())
        for name in feeds:
            assert shows(getattr(ro, name), getattr(want, name)), (kind, name, other.__name__)
    return NS(qkv=qkv, dout=dout, given=given, want=want, heads=heads, kind=kind, feeds=feeds)
