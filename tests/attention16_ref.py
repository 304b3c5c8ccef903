"""The CPU yardstick of full Attention's core on the bf16 matrix cores (``full_attn_precision="bf16"``,
csrc/attention16.hip).  Pure torch, no GPU import.

What the three kernels compute: both operands of every product rounded to bf16 (``q``: round-to-nearest-even), exact
products summed in fp32, everything else as the fp32 kernels have it.  ``core16`` restates that pass by pass -- the
backward fed GIVEN ``lse`` and ``out`` where the entry point reads them from its arguments --, ``Core16`` is the same as
an ``autograd.Function`` and ``yardstick16`` the ``Attention`` module around it (the module-level oracle).

The probes are inputs on which the arithmetic is exact in the style of tests/conv16_ref.py and tests/linattn16_ref.py: k
is constant over the keys of a (sample, head), so every logit of a row is the same fp32 number, p = exp2(0) = 1 and
l = n; every product and partial sum is then an integer (times the one trailing 32^-0.5, or over the one trailing n)
below 2^24, and any accumulation order gives the same bits.  The operand under test holds ``ties_and_neighbours``.
Every builder asserts its preconditions, so tests/test_attention16.py proves the probes without a GPU.

What no probe reaches exactly: the rounding of a COMPUTED p.  exp2 of a non-zero argument is not exact, so a probe with
p != 1 has no bit-exact expectation; that rounding (and the one of a ds that is not an integer) is covered by the bounds
of the random-operand tests only.
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

from conv16_ref import _same, q, ties_and_neighbours, trunc
from exact_probes import ints, is_integer, trits
from oracle import unet_ref

F32, F64 = torch.float32, torch.float64
D = 32
SCALE = float(np.float32(32 ** -0.5))       # the kernels' fp32 constant, as a Python float
LIMIT = 2.0 ** 24

# (B, heads, H, W, k x 20 in the last quarter of the pixels): tests/test_hip_attention_grad.py's CORE_CASES + a single pixel
CORE_CASES = [(2, 1, 5, 3, False),         # 15 pixels: fewer than a tile; three waves see no valid key
              (3, 4, 8, 8, False),         # 64: exactly one tile
              (2, 2, 13, 5, False),        # 65: one valid row in the second tile
              (2, 4, 14, 14, False),       # 196: three tiles and a part
              (1, 2, 33, 31, False),       # 1,023: one short of sixteen tiles
              (2, 4, 14, 14, True),        # logits to +-121: a missing or wrongly merged maximum overflows
              (1, 1, 1, 1, False)]         # a single pixel
PROBE_SHAPES = [c[:4] for c in CORE_CASES if not c[4]]
FORWARD_KINDS = ("v", "q", "k")            # which rounded operand holds the unrepresentable integers
BACKWARD_KINDS = ("dO", "v", "ds", "q", "k")
# B, dim, heads, H, W: tests/test_hip_attention_grad.py's MODULE_CASES
MODULE_CASES = [(2, 32, 1, 5, 3), (2, 64, 2, 13, 5), (2, 64, 4, 14, 14), (1, 96, 2, 33, 31), (3, 128, 4, 8, 8)]


def _r(rnd, t, dtype):
    """``rnd`` on the fp32 value (the kernels compute an operand in fp32, then round it), back in ``dtype``; the identity
    (``_same``: no rounding at all) leaves the value as ``dtype`` has it."""
    return t if rnd is _same else rnd(t.float()).to(dtype)


def split(qkv, heads, dtype):
    b, _, hh, ww = qkv.shape
    return [t.reshape(b, heads, D, hh * ww).to(dtype) for t in qkv.chunk(3, dim=1)]


# --------------------------------------------------------------------------------------------- what the kernels compute
def core16(qkv, heads, dout, given=None, dtype=F32, rnd=q):
    """The three passes from qkv [B, 3 hidden, H, W] and dout [B, hidden, H, W] (or None: forward only) with ``rnd`` on the
    operands the contract names, in ``dtype``.  ``given``: dict with ``lse`` [B, heads, n] and ``out`` [B, hidden, H, W] --
    what the backward reads instead of this function's own forward (fp32 tensors, as the kernels find them in memory).
    Returns out, lse, and with dout delta, dq, dk, dv [B, heads, 32, n] and dqkv [B, 3 hidden, H, W]."""
    given = given or {}
    b, _, hh, ww = qkv.shape
    n = hh * ww
    qq, k, v = split(qkv, heads, dtype)
    r = NS()
    # forward: S = q^ k^T; the fp32 constant on the sum; softmax in fp32; l sums the unrounded p; O = p^ v^; out = O / l
    a = torch.einsum("bhci,bhcj->bhij", _r(rnd, qq, dtype), _r(rnd, k, dtype)) * SCALE
    m = a.amax(dim=-1)
    pu = (a - m[..., None]).exp()
    l = pu.sum(dim=-1)
    o = torch.einsum("bhij,bhcj->bhci", _r(rnd, pu, dtype), _r(rnd, v, dtype)) / l[:, :, None, :]
    r.out, r.lse = o.reshape(b, heads * D, hh, ww), m + l.log()
    if dout is None:
        return r
    # backward: p = exp(a - lse), delta from the unrounded dO and out, dP = dO^ v^T, ds = p (dP - delta), three products
    lse = given["lse"].to(dtype) if "lse" in given else r.lse
    out = (given["out"].to(dtype) if "out" in given else r.out).reshape(b, heads, D, n)
    dO = dout.reshape(b, heads, D, n).to(dtype)
    p = (a - lse[..., None]).exp()
    r.delta = (dO * out).sum(dim=2)
    dP = torch.einsum("bhci,bhcj->bhij", _r(rnd, dO, dtype), _r(rnd, v, dtype))
    ds = p * (dP - r.delta[..., None])
    r.dq = SCALE * torch.einsum("bhij,bhcj->bhci", _r(rnd, ds, dtype), _r(rnd, k, dtype))
    r.dk = SCALE * torch.einsum("bhij,bhci->bhcj", _r(rnd, ds, dtype), _r(rnd, qq, dtype))
    r.dv = torch.einsum("bhij,bhci->bhcj", _r(rnd, p, dtype), _r(rnd, dO, dtype))
    r.dqkv = torch.cat([t.reshape(b, heads * D, hh, ww) for t in (r.dq, r.dk, r.dv)], dim=1)
    r.parts = NS(a=a, p=p, dP=dP, ds=ds)
    return r


class Core16(torch.autograd.Function):
    """``apply(qkv, heads)`` -> the core's output [B, hidden, H, W]: ``core16``'s forward, and in backward its two passes on
    the forward's own lse and out, rounded to fp32 where the kernels store them; in the dtype of qkv."""

    @staticmethod
    def forward(c, qkv, heads):
        r = core16(qkv, heads, None, dtype=qkv.dtype)
        c.heads = heads
        c.save_for_backward(qkv, r.lse.float(), r.out.float())
        return r.out

    @staticmethod
    def backward(c, dout):
        qkv, lse, out = c.saved_tensors
        return core16(qkv, c.heads, dout, dict(lse=lse, out=out), qkv.dtype).dqkv, None


def yardstick16(sd, x, dout, heads, dtype=F64):
    """tests/attention_ref.yardstick with ``Core16`` in place of the oracle's two einsums: out and {"x", parameter name:
    gradient} of sum(out * dout), the rest of the module in ``dtype``."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    y = unet_ref.rms_norm(xin, leaves["norm.g"])
    core = Core16.apply(F.conv2d(y, leaves["to_qkv.weight"]), heads)
    out = F.conv2d(core, leaves["to_out.weight"], leaves["to_out.bias"])
    grads = torch.autograd.grad(out, [xin] + list(leaves.values()), grad_outputs=dout.to(dtype))
    return out.detach(), dict(zip(["x"] + list(leaves), grads))


# --------------------------------------------------------------------------------------------- the exact probes
def _nchw(t, B, heads, H, W):
    return t.reshape(B, heads * D, H, W)


def _shows(a, b):
    """Somewhere ``a`` is off from ``b`` by more than 2^-12 relative."""
    return bool(((a - b).abs() > 2.0 ** -12 * b.abs()).any())


def _key(shape, kind, kinds, key):
    B, heads, H, W = shape
    return key + 1000 * kinds.index(kind) + 100 * heads + 10 * H + W


def forward_probe(shape, kind, key=9000):
    """qkv and the expected out and lse (fp64) of one forward probe.  k is constant over the keys and varies over the
    channels, so a row's logits are one fp32 number a, p = 1, l = n: out = mean_j(v^_j), lse = a + log n.  ``kind`` "v":
    v holds ``ties_and_neighbours`` (seen through out); "q" / "k": that operand does (seen through lse, where a wrong
    rounding moves a by multiples of 32^-0.5)."""
    B, heads, H, W = shape
    n = H * W
    key = _key(shape, kind, FORWARD_KINDS, key)
    hs = (B, heads, D, n)
    qq = ties_and_neighbours(hs, key) if kind == "q" else trits(hs, key)
    kc = ties_and_neighbours((B, heads, D, 1), key + 10) if kind == "k" else ints((B, heads, D, 1), key + 10, -3, 3)
    v = ties_and_neighbours(hs, key + 20) if kind == "v" else ints(hs, key + 20, -8, 8)
    qkv = torch.cat([_nchw(t, B, heads, H, W) for t in (qq, kc.expand(hs), v)], dim=1).contiguous()

    def run(rnd, dt):
        return core16(qkv, heads, None, None, dt, rnd)

    r32, r64 = run(q, F32), run(q, F64)
    # the preconditions: the logits' sums and the sums over the keys are integers below 2^24 whatever the order
    s = torch.einsum("bhci,bhcj->bhij", q(qq).double(), q(kc.expand(hs)).double())
    assert is_integer(s) and bool((s == s[..., :1]).all())
    assert float(torch.einsum("bhci,bhc->bhi", q(qq).double().abs(), q(kc[..., 0]).double().abs()).max()) < LIMIT
    raw = q(v).double().sum(dim=-1)                              # out n
    assert is_integer(raw) and float(q(v).double().abs().sum(dim=-1).max()) < LIMIT
    a32 = s[..., 0].float() * SCALE                              # fp32 x fp32, as the kernel multiplies
    want = NS(out=_nchw((raw / n)[..., None].expand(hs), B, heads, H, W), lse=a32.double() + math.log(n))
    assert torch.equal(r64.out, want.out)
    assert float((r64.lse - want.lse).abs().max()) <= 2.0 ** -22 * max(1.0, float(want.lse.abs().max()))   # fp64 a, not fp32 a
    assert float((r32.out.double() - want.out).abs().max()) <= 2.0 ** -21 * float(want.out.abs().max()) + 0.0
    # a kernel that does not round, or truncates, shows
    rounded = dict(q=qq, k=kc, v=v)[kind]
    assert not torch.equal(q(rounded), rounded)
    name = "out" if kind == "v" else "lse"
    for other in (_same, trunc):
        assert _shows(getattr(run(other, F64), name), getattr(r64, name)), (kind, other.__name__)
    return NS(qkv=qkv, want=want, heads=heads, kind=kind, feeds=name)


def backward_probe(shape, kind, key=9500):
    """qkv, dout, the given lse and out, and the expected dq, dk, dv (fp64, [B, heads, 32, n]) of one backward probe.  k is
    constant over the keys and lse_i is exactly the fp32 logit of row i, so p = 1 on every valid pair; out = 0, so delta = 0
    and ds = dP, an integer: dv_j = sum_i dO^_i, dq_i = 32^-0.5 sum_j ds^_ij k^_j, dk_j = 32^-0.5 sum_i ds^_ij q^_i.  ``kind``
    names what holds integers that bf16 does not: "dO" (seen through dv), "v" (dO holds +1 and -1 on two channels of a
    pixel, so dP is a difference of two v^ and small enough to survive its own rounding), "ds" (dO and v representable,
    dP = +-(256 m + e) is not), "q" (through dk), "k" (through dq)."""
    B, heads, H, W = shape
    n = H * W
    key = _key(shape, kind, BACKWARD_KINDS, key)
    hs = (B, heads, D, n)
    ch = torch.arange(D).reshape(1, 1, D, 1)
    qq = ties_and_neighbours(hs, key) if kind == "q" else trits(hs, key)
    kc = ties_and_neighbours((B, heads, D, 1), key + 10) if kind == "k" else ints((B, heads, D, 1), key + 10, -3, 3)
    v = ties_and_neighbours(hs, key + 20) if kind == "v" else trits(hs, key + 20)
    dO = ties_and_neighbours(hs, key + 30) if kind == "dO" else trits(hs, key + 30)
    if kind in ("v", "ds"):                                      # dO: two channels of every pixel, an even and an odd one
        c1 = 2 * ints((B, heads, 1, n), key + 31, 0, 15).long()
        c2 = 2 * ints((B, heads, 1, n), key + 32, 0, 15).long() + 1
        sg = 2 * ints((B, heads, 1, n), key + 33, 0, 1) - 1
        dO = sg * ((ch == c1).float() + (1.0 if kind == "ds" else -1.0) * (ch == c2).float())
    if kind == "ds":     # v: 512 or 768 on even channels, -1 or 3 on odd ones: 511, 515, 767, 771 round up, and truncate down
        v = torch.where(ch % 2 == 0, 256 * ints(hs, key + 21, 2, 3), 4 * ints(hs, key + 22, 0, 1) - 1)
    k = kc.expand(hs)
    qkv = torch.cat([_nchw(t, B, heads, H, W) for t in (qq, k, v)], dim=1).contiguous()
    dout = _nchw(dO, B, heads, H, W).contiguous()
    s = torch.einsum("bhci,bhcj->bhij", q(qq).double(), q(k).double())
    assert is_integer(s) and bool((s == s[..., :1]).all())
    assert float(torch.einsum("bhci,bhc->bhi", q(qq).double().abs(), q(kc[..., 0]).double().abs()).max()) < LIMIT
    lse = s[..., 0].float() * SCALE                              # fp32 x fp32: the kernel's logit, bit for bit
    given = dict(lse=lse, out=torch.zeros(B, heads * D, H, W))

    def run(rnd, dt, g=given):
        return core16(qkv, heads, dout, g, dt, rnd)

    r32 = run(q, F32)
    # fp32: p is exactly 1.  (fp64 forms the logit without fp32's rounding of the product: there p is 1 up to 2^-24 |a|,
    # and the expectation below is written down from p = 1 instead)
    assert bool((r32.parts.p == 1).all()) and bool((r32.delta == 0).all())
    dP = torch.einsum("bhci,bhcj->bhij", q(dO).double(), q(v).double())
    mag = [torch.einsum("bhci,bhcj->bhij", q(dO).double().abs(), q(v).double().abs()),
           torch.einsum("bhij,bhcj->bhci", q(dP.float()).double().abs(), q(k).double().abs()),
           torch.einsum("bhij,bhci->bhcj", q(dP.float()).double().abs(), q(qq).double().abs()),
           q(dO).double().abs().sum(dim=-1)]
    for t in mag:
        assert float(t.max()) < LIMIT, float(t.max())
    assert is_integer(dP) and torch.equal(r32.parts.ds.double(), dP)
    dsr = q(dP.float()).double()
    want = NS(dq=SCALE * torch.einsum("bhij,bhcj->bhci", dsr, q(k).double()),
              dk=SCALE * torch.einsum("bhij,bhci->bhcj", dsr, q(qq).double()),
              dv=q(dO).double().sum(dim=-1, keepdim=True).expand(hs).contiguous())
    assert is_integer(want.dv) and torch.equal(r32.dv.double(), want.dv)
    for name in ("dq", "dk"):                                    # fp32 torch agrees up to the trailing multiplication
        a, b = getattr(r32, name).double(), getattr(want, name)
        assert bool(((a - b).abs() <= 2.0 ** -21 * b.abs()).all()), name
    # a kernel that does not round, or truncates, shows on what the probed operand feeds (with p = 1 given to both)
    if kind == "ds":
        assert torch.equal(q(dO), dO) and torch.equal(q(v), v) and not torch.equal(q(dP.float()).double(), dP)
    else:
        rounded = dict(dO=dO, v=v, q=qq, k=kc)[kind]
        assert not torch.equal(q(rounded), rounded)
    feeds = {"dO": ("dv",), "v": ("dq", "dk"), "ds": ("dq", "dk"), "q": ("dk",), "k": ("dq",)}[kind]
    for other in (_same, trunc):
        so = torch.einsum("bhci,bhcj->bhij", _r(other, qq, F64), _r(other, k, F64))
        ro = run(other, F32, dict(given, lse=so[..., 0].float() * SCALE))          # (its own logits: p = 1 there as well)
        assert bool((ro.parts.p == 1).all())
        for name in feeds:
            assert _shows(getattr(ro, name).double(), getattr(want, name)), (kind, name, other.__name__)
    return NS(qkv=qkv, dout=dout, given=given, want=want, heads=heads, kind=kind, feeds=feeds)
