"""The CPU yardstick of the bf16 convolutions (``conv_precision="bf16"``, csrc/conv16.hip).  Pure torch, no GPU import.

What the three kernels compute: both operands of every product rounded to bf16 (``q``: round-to-nearest-even), the
products summed in fp32, everything else as in the fp32 path.  ``conv_ref`` / ``wgrad_ref`` / ``dgrad_ref`` restate that in
fp32 or fp64, ``Bf16Conv`` is the same as an ``autograd.Function`` (the module-level oracle), and the probes are inputs on
which the arithmetic is EXACT in the style of tests/exact_probes.py: every product and partial sum is an integer below
2^24, so any accumulation order and MFMA shape gives the same bits and the GPU comparison is ``torch.equal``.  Each builder
asserts its own preconditions, so tests/test_conv16_ref.py proves the probes without a GPU.
"""
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from exact_probes import check_exact, ints, is_integer, trits

LIMIT = 2.0 ** 24

# ---- the shapes of tests/test_hip_conv16.py: (B, Cin, Cout, H, W, k)
CONV_SHAPES = [(1, 32, 64, 5, 3, 3),       # one partial pixel tile, one chunk per tap
               (2, 96, 128, 9, 7, 3),      # two tiles with a remainder, three chunks, two column blocks, the seam between two images
               (2, 64, 64, 8, 8, 1),       # exactly full tiles, ksize 1
               (1, 128, 64, 7, 7, 3)]      # with residual and a non-zero shift
CONV_WITH_EPILOGUE = (1, 128, 64, 7, 7, 3)
DGRAD_SHAPE = (2, 64, 32, 6, 5, 3)         # the forward convolution's (Cin, Cout): Cout 32 padded to 64
WGRAD_CASES = [((1, 64, 64, 5, 3, 3), None), ((2, 64, 128, 9, 7, 3), None), ((2, 64, 128, 9, 7, 3), 3),
               ((2, 128, 64, 9, 7, 1), None), ((2, 128, 64, 9, 7, 1), 3)]     # (shape, splits: None = ld_seg_wgrad_splits')
WGRAD_SHAPES = sorted({s for s, _ in WGRAD_CASES})
PACK_SHAPES = [(32, 32, 3), (64, 96, 1), (20, 3, 3)]                          # (co, ci, k)


def q(t):
    """Round to bf16 (nearest even) and back: for fp32 tensors ``t.bfloat16().float()``."""
    return t.to(torch.bfloat16).to(t.dtype)


def trunc(t):
    """Chop an fp32 tensor to bf16 (what a kernel does that drops the low 16 bits instead of rounding)."""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _same(t):
    return t


# --------------------------------------------------------------------------------------------- what the kernels compute
def conv_ref(x, w, shift=None, residual=None, dt=torch.float32, rnd=q):
    """x [B, Cin, H, W], w [Cout, Cin, k, k] -> conv2d(q(x), q(w), padding = k // 2) + shift (+ residual) in ``dt``."""
    y = F.conv2d(rnd(x).to(dt), rnd(w).to(dt), padding=w.shape[-1] // 2)
    if shift is not None:
        y = y + shift.to(dt)[None, :, None, None]
    if residual is not None:
        y = y + residual.to(dt)
    return y


def dgrad_ref(dy, w, dt=torch.float32, rnd=q):
    """The data gradient of the same convolution: dy [B, Cout, H, W], w [Cout, Cin, k, k] -> [B, Cin, H, W]."""
    return F.conv_transpose2d(rnd(dy).to(dt), rnd(w).to(dt), padding=w.shape[-1] // 2)


def wgrad_ref(dy, a, k, dt=torch.float32, rnd=q):
    """The weight gradient dw [Cout, Cin, k, k] = sum over (b, y, x) of q(dy)[b, o, y, x] q(a)[b, c, y + i - p, x + j - p]."""
    out = F.conv2d(rnd(a).to(dt).transpose(0, 1), rnd(dy).to(dt).transpose(0, 1), padding=k // 2)       # [Cin, Cout, k, k]
    return out.transpose(0, 1).contiguous()


class Bf16Conv(torch.autograd.Function):
    """``apply(x, w, b)``: conv_ref forward; backward gives dx from q(dout) and q(w), dw from q(dout) and q(x) and db as the
    plain sum of dout -- exactly the three kernels' arithmetic, in the dtype of its inputs."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return conv_ref(x, w, b, dt=x.dtype)

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        return dgrad_ref(dout, w, dt=x.dtype), wgrad_ref(dout, x, w.shape[-1], dt=x.dtype), dout.sum(dim=(0, 2, 3))


# --------------------------------------------------------------------------------------------- the probes' operands
def small_ints(shape, key):
    """Integers in [-8, 8]: bf16 values."""
    return ints(shape, key, -8, 8)


def ties_and_neighbours(shape, key):
    """+- integers that bf16 does not hold: odd ones in [257, 511], each an exact tie between its two bf16 neighbours (the
    even one wins), and integers in [513, 1023] (spacing 4: residue 1 rounds down, 3 rounds up, 2 is a tie, 0 is exact)."""
    odd = 2 * ints(shape, key, 128, 255) + 1
    wide = ints(shape, key + 1, 513, 1023)
    v = torch.where(ints(shape, key + 2, 0, 1) == 0, odd, wide)
    return v * (2 * ints(shape, key + 3, 0, 1) - 1)


def _check_identity(*operands):
    for t in operands:
        assert torch.equal(q(t), t)


def _check_rounding(fn, rounded):
    """``fn(rnd)``: the probe's result in fp32 with ``rnd`` as the rounding.  The preconditions of a rounding probe."""
    ref32, ref64 = fn(q, torch.float32), fn(q, torch.float64)
    check_exact(ref32, ref64, limit=LIMIT)
    assert not torch.equal(q(rounded), rounded)
    assert not torch.equal(ref32, fn(_same, torch.float32))           # ... a kernel that does not round shows
    assert not torch.equal(ref32, fn(trunc, torch.float32))           # ... and so does one that truncates
    return ref32


def _epilogue(shape, key, on):
    B, cin, cout, H, W, k = shape
    if not on:
        return torch.zeros(cout), None
    return ints((cout,), key + 20, -4, 4), ints((B, cout, H, W), key + 21, -4, 4)


def conv_probe(shape, kind, epilogue=False, key=7000):
    """``kind`` "identity": x in {-1, 0, 1}, w in [-8, 8]; "rounding": x = ties_and_neighbours (the activations are what
    the kernel rounds), w in {-1, 0, 1}.  With K <= 9 * 128 every sum stays below 2^24."""
    B, cin, cout, H, W, k = shape
    assert k * k * cin <= 9 * 128
    key += 100 * cin + 10 * H + k
    shift, res = _epilogue(shape, key, epilogue)
    if kind == "identity":
        x, w = trits((B, cin, H, W), key), small_ints((cout, cin, k, k), key + 1)
        _check_identity(x, w)
        ref = conv_ref(x, w, shift, res)
        check_exact(ref, conv_ref(x, w, shift, res, torch.float64), limit=LIMIT)
    else:
        x, w = ties_and_neighbours((B, cin, H, W), key), trits((cout, cin, k, k), key + 1)
        ref = _check_rounding(lambda rnd, dt: conv_ref(x, w, shift, res, dt, rnd), x)
    return NS(x=x, w=w, shift=shift, res=res, ref=ref)


def dgrad_probe(shape, kind, key=7300):
    """The data gradient: dy [B, Cout, H, W] and the OIHW weight.  "rounding" puts the unrepresentable integers into the
    WEIGHT (ld_dn_pack_conv16 rounds it) and into dy in turn (``kind`` "rounding_w" / "rounding_dy")."""
    B, cin, cout, H, W, k = shape
    assert k * k * cout <= 9 * 128
    key += 100 * cin + 10 * H + k
    if kind == "identity":
        dy, w = trits((B, cout, H, W), key), small_ints((cout, cin, k, k), key + 1)
        _check_identity(dy, w)
        ref = dgrad_ref(dy, w)
        check_exact(ref, dgrad_ref(dy, w, torch.float64), limit=LIMIT)
    elif kind == "rounding_w":
        dy, w = trits((B, cout, H, W), key), ties_and_neighbours((cout, cin, k, k), key + 1)
        ref = _check_rounding(lambda rnd, dt: dgrad_ref(dy, w, dt, rnd), w)
    else:
        dy, w = ties_and_neighbours((B, cout, H, W), key), trits((cout, cin, k, k), key + 1)
        ref = _check_rounding(lambda rnd, dt: dgrad_ref(dy, w, dt, rnd), dy)
    return NS(dy=dy, w=w, ref=ref)


def wgrad_probe(shape, kind, key=7600):
    """``kind`` "identity", "rounding_dy" or "rounding_a" (which operand holds the unrepresentable integers)."""
    B, cin, cout, H, W, k = shape
    assert B * H * W <= 9 * 128
    key += 100 * cin + 10 * H + k
    ds, as_ = (B, cout, H, W), (B, cin, H, W)
    if kind == "identity":
        dy, a = trits(ds, key), small_ints(as_, key + 1)
        _check_identity(dy, a)
        ref = wgrad_ref(dy, a, k)
        check_exact(ref, wgrad_ref(dy, a, k, torch.float64), limit=LIMIT)
    elif kind == "rounding_dy":
        dy, a = ties_and_neighbours(ds, key), trits(as_, key + 1)
        ref = _check_rounding(lambda rnd, dt: wgrad_ref(dy, a, k, dt, rnd), dy)
    else:
        dy, a = trits(ds, key), ties_and_neighbours(as_, key + 1)
        ref = _check_rounding(lambda rnd, dt: wgrad_ref(dy, a, k, dt, rnd), a)
    return NS(dy=dy, a=a, ref=ref)


def pack_probe(shape, key=7900):
    """An OIHW weight of unrepresentable integers and its two padded kernel layouts, rounded: fwd [cop][k k][cip] and dgr
    [cip][k k, flipped][cop] as fp32 tensors holding bf16 values, zero in the padded channels."""
    co, ci, k = shape
    cop, cip = (co + 63) // 64 * 64, (ci + 63) // 64 * 64
    w = ties_and_neighbours((co, ci, k, k), key + 10 * co + ci)
    assert not torch.equal(q(w), w) and not torch.equal(q(w), trunc(w)) and is_integer(q(w))
    fwd, dgr = pack_ref(q(w), cop, cip)
    return NS(w=w, cop=cop, cip=cip, fwd=fwd, dgr=dgr)


def pack_ref(w, cop, cip):
    """The two kernel layouts of an OIHW weight (``trainable.pack_conv``'s), flat, zero in the padded channels."""
    co, ci, k, _ = w.shape
    fwd = torch.zeros(cop, k * k, cip, dtype=w.dtype)
    fwd[:co, :, :ci] = w.permute(0, 2, 3, 1).reshape(co, k * k, ci)
    dgr = torch.zeros(cip, k * k, cop, dtype=w.dtype)
    dgr[:ci, :, :co] = w.flip(2, 3).permute(1, 2, 3, 0).reshape(ci, k * k, co)
    return fwd.reshape(-1), dgr.reshape(-1)


# --------------------------------------------------------------------------------------------- the random tests' bound
U = 2.0 ** -23


def sum_bound(K, magnitude):
    """(K + 4) u times the sum of the terms' absolute values (fp64): K u is the worst case of a K-term fp32 sum in any
    order, whether the adds round to nearest or truncate; + 4 for the epilogue's multiply and adds."""
    return (K + 4) * U * magnitude.double()


# --------------------------------------------------------------------------------------------- ResnetBlock on Bf16Conv
def resnet_block(sd, x, temb, groups=8):
    """oracle.unet_ref.resnet_block (ddpm.py:188-212) with ``Bf16Conv`` in place of its three convolutions, in the dtype of
    its arguments; ``sd`` has the block's state_dict names."""
    film = None
    if temb is not None:
        e = F.linear(F.silu(temb), sd["mlp.1.weight"], sd["mlp.1.bias"])[:, :, None, None]
        film = e.chunk(2, dim=1)

    def conv_gn_act(p, h, film):
        y = Bf16Conv.apply(h, sd[p + ".proj.weight"], sd[p + ".proj.bias"])
        y = F.group_norm(y, groups, sd[p + ".norm.weight"], sd[p + ".norm.bias"], eps=1e-5)
        if film is not None:
            y = y * (film[0] + 1) + film[1]
        return F.silu(y)

    h = conv_gn_act("block2", conv_gn_act("block1", x, film), None)
    if "res_conv.weight" in sd:
        x = Bf16Conv.apply(x, sd["res_conv.weight"], sd["res_conv.bias"])
    return h + x


def block_yardstick(sd, x, temb, dout, dtype, groups=8):
    """out and {"x", "time_emb", parameter name: gradient of sum(out * dout)} of ``resnet_block`` with ``dtype`` intermediates."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    tin = None if temb is None else temb.detach().to(dtype).clone().requires_grad_(True)
    out = resnet_block(leaves, xin, tin, groups)
    names = ["x"] + ([] if tin is None else ["time_emb"]) + list(leaves)
    inputs = [xin] + ([] if tin is None else [tin]) + list(leaves.values())
    grads = torch.autograd.grad(out, inputs, grad_outputs=dout.to(dtype))
    return out.detach(), dict(zip(names, grads))
