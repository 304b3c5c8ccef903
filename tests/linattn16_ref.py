"""The CPU yardstick of LinearAttention's core on the bf16 matrix cores (``attn_precision="bf16"``, csrc/linattn16.hip).
Pure torch, no GPU import.

What the four kernels compute: both operands of every 32 x 32 product of a head rounded to bf16 (``q``:
round-to-nearest-even), exact products summed in fp32, everything else as the fp32 kernels have it.  ``core16`` restates
that pass by pass, each pass fed GIVEN ctx / (m, Z) / dctx / rk where it reads them, so that a pass is checked by itself;
``Core16`` is the same as an ``autograd.Function`` and ``yardstick16`` the module around it (the module-level oracle).
The probes are inputs on which the arithmetic is exact in the style of tests/conv16_ref.py: k is constant per channel
(P = exp(0) = 1, Z = n, ks = 1 / n), q is constant per pixel (p = 1 / 32), and v, dO, ctx and dctx hold
``ties_and_neighbours`` integers and {-1, 0, 1} in turn, so every product and partial sum is an integer (or one fixed
multiple of integers) below 2^24: any accumulation order gives the same bits.  Every builder asserts its preconditions, so
tests/test_linattn16.py proves the probes without a GPU.
"""
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from conv16_ref import _same, q, ties_and_neighbours, trunc
from exact_probes import ints, is_integer, trits
from oracle import unet_ref

F32, F64 = torch.float32, torch.float64
D = 32
SCALE = 0.17677669529663687          # 32^-0.5, the kernels' constant (fp64; the element-wise passes use its fp32 value)
LIMIT = 2.0 ** 24

# (B, heads, H, W, shifted): tests/test_hip_linattn_grad.py's CORE_CASES
CORE_CASES = [(2, 1, 5, 3, False),         # 15 pixels: fewer than one 32-pixel tile; padding in out and dqkv
              (2, 4, 14, 14, False),       # 196 = 6 x 32 + 4 pixels, four parts
              (1, 2, 33, 31, False),       # 1,023 pixels, 16 parts, ragged last tile
              (3, 4, 8, 8, False),         # exactly two tiles
              (2, 4, 14, 14, True)]        # k near +100 in the last quarter of the pixels only
PROBE_SHAPES = [c[:4] for c in CORE_CASES if not c[4]] + [(1, 2, 16, 32)]     # + 512 pixels, a power of two, several parts
PROBE_KINDS = ("v", "dO", "ctx", "dctx")   # which rounded memory operand holds the unrepresentable integers
MODULE_CASES = [(2, 32, 1, 5, 3), (2, 64, 4, 14, 14), (1, 96, 2, 33, 31), (3, 128, 4, 8, 8)]     # B, dim, heads, H, W


def _r(rnd, t, dtype):
    """``rnd`` on the fp32 value (the kernels compute an operand in fp32, then round it), back in ``dtype``; the identity
    (``_same``: no rounding at all) leaves the value as ``dtype`` has it."""
    return t if rnd is _same else rnd(t.float()).to(dtype)


def split(qkv, heads, dtype):
    b, _, hh, ww = qkv.shape
    return [t.reshape(b, heads, D, hh * ww).to(dtype) for t in qkv.chunk(3, dim=1)]


# --------------------------------------------------------------------------------------------- what the kernels compute
def core16(qkv, heads, dout, given=None, dtype=F32, rnd=q):
    """The four passes from qkv [B, 3 hidden, H, W] and dout [B, hidden, H, W] with ``rnd`` on the operands the contract
    names, in ``dtype``.  ``given``: dict with any of ``ctx`` [B, heads, 32, 32], ``m``, ``Z`` [B, heads, 32], ``dctx``,
    ``rk`` [B, heads, 32] -- what the LATER passes read instead of this function's own results (fp32 tensors, as the
    kernels find them in memory).  Returns dict(m, Z, ctx, out, dctx, rk, dq, dk, dv, dqkv) plus the terms' magnitudes
    that ``bounds`` wants."""
    given = given or {}
    b, _, hh, ww = qkv.shape
    qq, k, v = split(qkv, heads, dtype)
    dO = dout.reshape(b, heads, D, hh * ww).to(dtype)
    r = NS()
    # context: P = exp(k - m) in fp32, then rounded; v rounded; Z sums the unrounded P
    r.m = k.amax(dim=-1)
    P = (k - r.m[..., None]).exp()
    r.Z = P.sum(dim=-1)
    r.ctx = torch.einsum("bhdn,bhen->bhde", _r(rnd, P, dtype), _r(rnd, v, dtype)) / r.Z[..., None]
    ctx, m, Z = (given.get(name, getattr(r, name)).to(dtype) for name in ("ctx", "m", "Z"))
    # out: p = softmax_d(q) in fp32, then rounded; ctx rounded; the product times 32^-0.5
    p = qq.softmax(dim=-2)
    r.out = (torch.einsum("bhde,bhdn->bhen", _r(rnd, ctx, dtype), _r(rnd, p, dtype)) * SCALE).reshape(b, heads * D, hh, ww)
    # reduce: p and dO rounded; 32^-0.5 and rk (from the stored fp32 dctx and ctx) in the fp64 merge
    r.dctx = torch.einsum("bhdn,bhen->bhde", _r(rnd, p, dtype), _r(rnd, dO, dtype)) * SCALE
    r.rk = (r.dctx.float().to(dtype) * ctx).sum(dim=-1)
    dctx, rk = (given.get(name, getattr(r, name)).to(dtype) for name in ("dctx", "rk"))
    # apply: ks = exp(k - m) (1 / Z) as la_apply_kernel writes it (the reciprocal is an fp32 value); six rounded operands
    iz = (1.0 / Z.float()).to(dtype)
    ks = (k - m[..., None]).exp() * iz[..., None]
    s = torch.einsum("bhde,bhen->bhdn", _r(rnd, ctx, dtype), _r(rnd, dO, dtype))
    dot = (p * s).sum(dim=-2, keepdim=True)
    tk = torch.einsum("bhde,bhen->bhdn", _r(rnd, dctx, dtype), _r(rnd, v, dtype))
    r.dq = SCALE * p * (s - dot)
    r.dk = ks * (tk - rk[..., None])
    r.dv = torch.einsum("bhde,bhdn->bhen", _r(rnd, dctx, dtype), _r(rnd, ks, dtype))
    r.dqkv = torch.cat([t.reshape(b, heads * D, hh, ww) for t in (r.dq, r.dk, r.dv)], dim=1)
    r.parts = NS(P=P, v=v, p=p, dO=dO, ctx=ctx, dctx=dctx, ks=ks, s=s, tk=tk, rk=rk, Z=r.Z)
    return r


class Core16(torch.autograd.Function):
    """``apply(qkv, heads)`` -> the core's output [B, hidden, H, W]: ``core16``'s forward, and in backward its reduce and
    apply passes on the forward's own ctx and (m, Z), rounded to fp32 where the kernels store them; in the dtype of qkv."""

    @staticmethod
    def forward(c, qkv, heads):
        r = core16(qkv, heads, torch.zeros_like(qkv[:, :heads * D]), dtype=qkv.dtype)
        c.heads = heads
        c.save_for_backward(qkv, r.ctx.float(), r.m.float(), r.Z.float())
        given = dict(ctx=r.ctx.float())
        return core16(qkv, heads, torch.zeros_like(qkv[:, :heads * D]), given, qkv.dtype).out

    @staticmethod
    def backward(c, dout):
        qkv, ctx, m, Z = c.saved_tensors
        r = core16(qkv, c.heads, dout, dict(ctx=ctx, m=m, Z=Z), qkv.dtype)
        r = core16(qkv, c.heads, dout, dict(ctx=ctx, m=m, Z=Z, dctx=r.dctx.float(), rk=r.rk.float()), qkv.dtype)
        return r.dqkv, None


def yardstick16(sd, x, dout, heads, dtype=F64):
    """tests/linattn_ref.yardstick with ``Core16`` in place of the oracle's two einsums: out and {"x", parameter name:
    gradient} of sum(out * dout), the rest of the module in ``dtype``."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    y = unet_ref.rms_norm(xin, leaves["norm.g"])
    core = Core16.apply(F.conv2d(y, leaves["to_qkv.weight"]), heads)
    out = unet_ref.rms_norm(F.conv2d(core, leaves["to_out.0.weight"], leaves["to_out.0.bias"]), leaves["to_out.1.g"])
    grads = torch.autograd.grad(out, [xin] + list(leaves.values()), grad_outputs=dout.to(dtype))
    return out.detach(), dict(zip(["x"] + list(leaves), grads))


# --------------------------------------------------------------------------------------------- the exact probes
def probe(shape, kind, key=8000):
    """qkv, dout and the given ctx / m / Z / dctx / rk of one probe, with its expected results (fp32 tensors that hold the
    exact values: ``ctx``, ``dctx`` and ``kstat`` through the merge's fp64 arithmetic restated and cast, ``out`` / ``dq`` /
    ``dk`` / ``dv`` as fp64).  ``kind`` names the operand that holds ``ties_and_neighbours``; the other three hold
    {-1, 0, 1}.  k is constant per channel, q constant per pixel."""
    B, heads, H, W = shape
    n = H * W
    key += 1000 * PROBE_KINDS.index(kind) + 100 * heads + 10 * H + W
    hs, ms = (B, heads, D, n), (B, heads, D, D)

    def operand(name, shp, k):
        return ties_and_neighbours(shp, k) if kind == name else trits(shp, k)

    v, dO = operand("v", hs, key), operand("dO", hs, key + 10)
    ctx, dctx = operand("ctx", ms, key + 20), operand("dctx", ms, key + 30)
    kc = ints((B, heads, D, 1), key + 40, -3, 3) / 4            # k: one value per channel
    qc = ints((B, heads, 1, n), key + 41, -3, 3) / 4            # q: one value per pixel
    rk = ints((B, heads, D), key + 42, -8, 8)
    qkv = torch.cat([t.reshape(B, heads * D, H, W) for t in (qc.expand(hs), kc.expand(hs), v)], dim=1).contiguous()
    dout = dO.reshape(B, heads * D, H, W).contiguous()
    m, Z = kc[..., 0].clone(), torch.full((B, heads, D), float(n))
    given = dict(ctx=ctx, m=m, Z=Z, dctx=dctx, rk=rk)
    # the preconditions, in fp32: exp(0) = 1 and the sum of 32 of them is 32.0, so P = 1, Z = n, p = 1 / 32, ks = 1 / n
    qq, kk, _ = split(qkv, heads, F32)
    e = (qq - qq.amax(dim=-2, keepdim=True)).exp()
    assert bool((e == 1).all()) and bool((e.sum(dim=-2) == 32.0).all()) and bool((qq.softmax(dim=-2) == 1 / 32).all())
    assert bool(((kk - m[..., None]).exp() == 1).all())

    def run(rnd, dt):
        return core16(qkv, heads, dout, given, dt, rnd)

    r32, r64 = run(q, F32), run(q, F64)
    assert torch.equal(r64.Z, Z.double()) and torch.equal(r64.m, m.double())
    iz = 1.0 / Z                                               # fp32, as the kernel divides
    assert torch.equal(r32.parts.ks, iz[..., None].expand(hs)) and torch.equal(r64.parts.ks, r32.parts.ks.double())
    # every sum is exact: fp32 == fp64 bit for bit, integers (times one power of two or one 8-bit factor) below 2^24
    raw_ctx = torch.einsum("bhdn,bhen->bhde", torch.ones(hs, dtype=F64), q(v).double())            # ctx Z
    raw_dctx = torch.einsum("bhdn,bhen->bhde", torch.full(hs, 1 / 32, dtype=F64), q(dO).double())   # dctx / 32^-0.5
    mag = [torch.einsum("bhdn,bhen->bhde", torch.ones(hs, dtype=F64), q(v).double().abs()),
           torch.einsum("bhdn,bhen->bhde", torch.ones(hs, dtype=F64), q(dO).double().abs()),             # (x 32 of the real terms)
           torch.einsum("bhde,bhen->bhdn", q(ctx).double().abs(), q(dO).double().abs()),
           torch.einsum("bhde,bhen->bhdn", q(dctx).double().abs(), q(v).double().abs()),
           torch.einsum("bhde,bhdn->bhen", q(dctx).double().abs(), torch.ones(hs, dtype=F64)),
           32 * (r64.parts.s.abs() / 32).sum(dim=-2)]                                                    # dot, in units of 1 / 32
    for t in mag:
        assert float(t.max()) < LIMIT, float(t.max())
    assert is_integer(raw_ctx) and is_integer(32 * raw_dctx) and is_integer(r64.parts.s)
    for name in ("ctx", "out", "dctx", "dq", "dk", "dv"):
        a, b = getattr(r32, name).double(), getattr(r64, name)
        assert float((a - b).abs().max()) <= 2.0 ** -21 * float(b.abs().max()), name      # fp32 torch agrees up to the trailing multiplications
    want = NS(ctx=(raw_ctx / Z.double()[..., None]).float(), kstat=torch.stack([m, Z], dim=-1),
              dctx=(raw_dctx * SCALE).float(), rk32=r32.rk, rk64=r64.rk, out=r64.out, dq=r64.dq, dk=r64.dk, dv=r64.dv)
    assert torch.equal(want.ctx, r64.ctx.float()) and torch.equal(want.dctx, r64.dctx.float())
    # a kernel that does not round, or truncates, shows: on what the probed operand feeds, by more than 2^-12 relative
    feeds = {"v": ("ctx", "dk"), "dO": ("dctx", "dq"), "ctx": ("out", "dq"), "dctx": ("dk", "dv")}[kind]
    rounded = dict(v=v, dO=dO, ctx=ctx, dctx=dctx)[kind]
    assert not torch.equal(q(rounded), rounded)
    for other in (_same, trunc):
        ro = run(other, F64)
        for name in feeds:
            a, b = getattr(ro, name), getattr(r64, name)
            assert float((a - b).abs().max()) > 2.0 ** -12 * float(b.abs().max()), (kind, name, other.__name__)
    return NS(qkv=qkv, dout=dout, given=given, want=want, heads=heads, kind=kind)


# --------------------------------------------------------------------------------------------- the random tests' bound
U = 2.0 ** -23


def term_bound(K, magnitude, other_max):
    """The worst case of a K-term product sum with both operands rounded to bf16 and an fp32 accumulator, against the
    unrounded fp64 sum: (2 2^-8 + 2^-16) of the sum of the terms' absolute values for the two roundings ((1 + 2^-8)^2 - 1;
    bf16's unit roundoff is 2^-9, so half of it is room for the fp32 roundings in front of the conversion: v_exp_f32, the
    softmax's normalisation, Z), (K + 4) 2^-23 for the fp32 sum in any order and the epilogue, and K 2^-126 max|other
    operand| for operands below bf16's normal range, which the conversion or the matrix core may flush."""
    return (2 * 2.0 ** -8 + 2.0 ** -16 + (K + 4) * U) * magnitude.double() + K * 2.0 ** -126 * float(other_max)


def bounds(ref):
    """Per-element bounds of the six outputs of ``core16(..., rnd=identity, dtype=float64)`` (``ref``), every pass on given
    inputs: ctx, out, dctx, dq, dk, dv.  dq and dk carry the bounds of s, dot and tk through their fp32 formulas: four more
    fp32 roundings on dq's terms, and for dk the fp32 ks itself below the normal range -- the same 2^-126 as bf16's, since the
    two formats share the exponent -- where v_exp_f32 returns zero (the fp32 kernels' ks as well): 2^-126 |tk - rk|."""
    t = ref.parts
    n = t.P.shape[-1]
    b, heads = t.P.shape[:2]
    amax = lambda x: float(x.abs().max())                                                      # noqa: E731
    ctx = term_bound(n, torch.einsum("bhdn,bhen->bhde", t.P.abs(), t.v.abs()), max(amax(t.v), amax(t.P))) / t.Z[..., None]
    out = SCALE * term_bound(D, torch.einsum("bhde,bhdn->bhen", t.ctx.abs(), t.p), max(amax(t.ctx), 1.0))
    dctx = SCALE * term_bound(n, torch.einsum("bhdn,bhen->bhde", t.p, t.dO.abs()), max(amax(t.dO), 1.0))
    s = term_bound(D, torch.einsum("bhde,bhen->bhdn", t.ctx.abs(), t.dO.abs()), max(amax(t.ctx), amax(t.dO)))
    dot = (t.p * s).sum(dim=-2, keepdim=True)
    dq = SCALE * t.p * (s + dot) + 4 * U * SCALE * t.p * (t.s.abs() + (t.p * t.s.abs()).sum(dim=-2, keepdim=True))
    tk = term_bound(D, torch.einsum("bhde,bhen->bhdn", t.dctx.abs(), t.v.abs()), max(amax(t.dctx), amax(t.v)))
    dk = t.ks * tk + 2.0 ** -126 * (t.tk.abs() + t.rk.abs()[..., None])
    dv = term_bound(D, torch.einsum("bhde,bhdn->bhen", t.dctx.abs(), t.ks), max(amax(t.dctx), amax(t.ks)))
    return NS(ctx=ctx, out=out.reshape(ref.out.shape), dctx=dctx, dq=dq, dk=dk, dv=dv)
