"""Inputs for which the arithmetic of a kernel is EXACT, with their expected values (pure torch on the CPU).

A norm-wise tolerance of a few storage half-ulps of the largest output lets a mis-read channel, a key counted twice or
a pixel lost at a chunk edge through: those move a long reduction by far less than one rounding of its result.  On
the probes below every product and every partial sum is a small integer (or a multiple of 2^-10 / 2^-8 well inside 24
bits), so ANY accumulation order, chunk width and MFMA shape gives the same bits, and the comparison is torch.equal.
Each builder asserts its own preconditions against fp32 and fp64 torch, so tests/test_exact_probes.py proves the
probes on a machine without a GPU and tests/test_hip_exact.py only has to compare.

Draws come from the package's counter-based generator (rng.uniform, seed 1234, one stream per tensor), rounded.
"""
import functools
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

from localdiffusion_hallucination_amd import rng

SEED = 1234
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
LIMIT = 256.0               # |integer| <= 256 is exact in bf16 (8 significant bits), fp16 and fp32

# ---- the shapes of tests/test_hip_exact.py (tests/test_exact_probes.py proves every one of them on the CPU)
CONV3_SHAPES = [(2, 32, 32, 16, 16), (1, 64, 32, 20, 28), (1, 128, 64, 7, 7), (1, 256, 256, 8, 8), (2, 64, 32, 17, 23)]
CONV3_SK_SHAPES = [(1, 96, 32, 13, 18), (2, 256, 64, 16, 16)]
S32_SIZES = [(48, 32), (40, 24)]
S32_CASES = {"plain32": 32, "one64": 64, "two32": 64}          # case -> input channels
BIG64_SHAPE = (2, 64, 128, 40, 24)
C32_SHAPE = (2, 32, 32, 32, 32)                                # the smallest map conv3x3_c32.hip's router accepts
CONV1_SHAPES = [(1, 384, 256, 8, 8), (1, 96, 64, 14, 14), (1, 32, 384, 28, 28)]
IMAGE_CASES = [(cin, ks, H, W) for cin in (1, 3) for ks in (3, 7) for (H, W) in ((20, 12), (28, 28))]
STEM_SHAPES = [(3, 40, 33), (1, 28, 28)]                       # cin, H, W
FINAL_CASES = [(32, 1), (32, 3), (64, 1), (64, 3),             # cin, cout at 9 x 11
               (8, 2), (8, 4), (24, 4), (40, 3)]               # ... a partial pass of the 4 x 16 B channel loop, cout 2 and 4
ATTN_SIZES = [49, 324, 400, 1024, 4096]
LINATTN_SHAPES = [(32, 28, 28), (64, 14, 14), (32, 64, 96)]    # C, H, W
# ---- the shapes of tests/test_hip_conv_tiles.py (every tile variant of ld_conv3x3 / ld_conv1x1, forced through the routing table)
TILE3_RAGGED32 = [(2, 64, 32, 40, 24), (1, 32, 96, 33, 20)]    # ragged in both axes for 8- and 16-row tiles; Cout % 64 != 0, one row past two 16-row tiles
TILE3_RAGGED64 = [BIG64_SHAPE, (2, 64, 64, 17, 23)]
TILE3_WHOLE = {32: (1, 128, 32, 32, 48), 64: (1, 128, 64, 32, 48)}   # whole tiles only: every workgroup takes the FULL emit path
TILE3_SK_SHAPES = [(1, 256, 64, 16, 16), (1, 96, 32, 13, 18)]    # eight chunks; an odd chunk count on a ragged map
TILE3_CAT = (2, 64, 32, 40, 24)                                  # B, c1 (half resolution), c2, H, W of conv3x3_concat_upsample
TILE3_CAT_COUTS = [32, 96, 128]
TILE3_ADDEND_SHAPES = [(2, 64, 32, 40, 24), (2, 64, 128, 40, 24), (2, 64, 32, 17, 23)]
TILE1_SHAPES = [(2, 64, 64, 17, 23), (2, 96, 128, 17, 23), (2, 64, 96, 17, 23)]   # 391 pixels: one 256-pixel tile + 135, the last 16-pixel group holds 7
TILE1_GROUP_SHAPES = [(1, 160, 32, 20, 28), (1, 416, 64, 17, 23), (2, 128, 64, 9, 11)]   # 5 and 13 chunks (partial groups); below one tile
TILE1_CAT = (2, 64, 32, 17, 23)                                  # B, c1, c2, H, W of conv1x1_concat
TILE1_UNSHUFFLE = (2, 32, 17, 23)                                # B, c, H, W of conv1x1_unshuffle
TILE1_VARIANT_COUTS = [64, 128]
# ---- the shapes of tests/test_hip_attention_heads.py (head counts other than the model's default of 4)
OTHER_HEADS = [1, 2, 8]
ATTN_HEADS_SIZES = [49, 324]                                   # one ragged key tile; three tiles, two key groups
KVCTX_HEADS_SHAPES = [(32, 28, 28), (64, 14, 14), (128, 7, 7)] # C, H, W: 3 pixel chunks; one ragged tile; 49 pixels, four K-chunks


def tile_groups(cout):
    """Statistics groups of the tile tests: the model's 8, but 12 at Cout = 96 -- ld_conv3x3 takes group widths that divide
    32 (a workgroup's channel tile holds whole groups), and 96 / 8 = 12 does not (docs/findings.md 142)."""
    return 8 if 32 % (cout // 8) == 0 else 12


def ints(shape, key, lo, hi):
    """Integers lo..hi with equal weights, fp32: the seeded uniform draw on [lo - 1/2, hi + 1/2), rounded."""
    u = rng.uniform(shape, SEED, key, lo - 0.5, hi + 0.5)
    return torch.from_numpy(np.clip(np.rint(u), lo, hi).astype(np.float32))


def trits(shape, key):
    """{-1, 0, 1} in equal thirds."""
    return ints(shape, key, -1, 1)


def odd_1024ths(shape, key):
    """odd / 1024 in (-1/2, 1/2): what makes a result unrepresentable in 16 bits while fp32 still holds it exactly."""
    return (2 * ints(shape, key, -255, 255) + 1) / 1024


def bias_for(cout, key, frac=False):
    """Integers in [-4, 4]; the rounding variant adds odd / 1024."""
    b = ints((cout,), key, -4, 4)
    return b + odd_1024ths((cout,), key + 5000) if frac else b


def gn_stats_ref(y, groups):
    """[B, groups, 2] fp64 (sum, sumsq) of an NCHW tensor (hip_helpers.gn_stats_ref, without the device import)."""
    g = y.double().reshape(y.shape[0], groups, -1)
    return torch.stack([g.sum(-1), (g * g).sum(-1)], dim=-1)


def is_integer(t):
    return bool((t == t.round()).all())


def check_exact(ref32, ref64, integer=True, limit=LIMIT):
    """The preconditions of every probe: fp32 torch == fp64 torch bit for bit, the result within the exact range."""
    assert torch.equal(ref32.double(), ref64), float((ref32.double() - ref64).abs().max())
    assert float(ref64.abs().max()) <= limit, float(ref64.abs().max())
    if integer:
        assert is_integer(ref64)


def stored(ref32, dtype):
    """What a kernel must leave in ``dtype`` storage for the exact fp32 value: one round-to-nearest-even (torch's .to)."""
    return ref32.to(TDT[dtype]).float()


def check_representable(t, dtype):
    assert torch.equal(t.to(TDT[dtype]).float(), t)


def _conv(x, w, b, padding, residual=None, frac=False, groups=None):
    """fp32 and fp64 F.conv2d of the same operands -> (ref fp32, fp64 statistics or None), preconditions asserted."""
    ref64 = F.conv2d(x.double(), w.double(), b.double(), padding=padding)
    ref32 = F.conv2d(x, w, b, padding=padding)
    if residual is not None:
        ref64, ref32 = ref64 + residual.double(), ref32 + residual
    check_exact(ref32, ref64, integer=not frac)
    stats = None
    if groups:
        stats = gn_stats_ref(ref64, groups)
        if not frac:
            assert is_integer(stats) and float(stats.abs().max()) < 2.0 ** 53
    if frac:          # not representable in 16 bits somewhere: the stored value is a genuine rounding
        for dt in ("bf16", "fp16"):
            assert not torch.equal(stored(ref32, dt), ref32)
    return ref32, stats


# --------------------------------------------------------------------------------------------- convolutions (1a, 1b)
def conv3x3(B, cin, cout, H, W, key=1000, frac=False, groups=8):
    x, w, b = trits((B, cin, H, W), key), trits((cout, cin, 3, 3), key + 1), bias_for(cout, key + 2, frac)
    ref, stats = _conv(x, w, b, 1, frac=frac, groups=groups)
    return NS(x=x, w=w, b=b, ref=ref, stats=stats)


def conv3x3_addend(B, cin, cout, H, W, key=1300, groups=8):
    """conv3x3 plus ``add``, an integer tensor in [-4, 4] of the output's shape (ld_conv3x3_args.addend): the addend
    enters BEFORE the statistics, so ``stats`` are those of conv + bias + add."""
    x, w, b = trits((B, cin, H, W), key), trits((cout, cin, 3, 3), key + 1), bias_for(cout, key + 2)
    add = ints((B, cout, H, W), key + 3, -4, 4)
    ref, stats = _conv(x, w, b, 1, residual=add, groups=groups)
    plain, plain_stats = _conv(x, w, b, 1, groups=groups)
    assert not torch.equal(ref, plain) and not torch.equal(stats, plain_stats)      # a dropped addend shows in both
    return NS(x=x, w=w, b=b, add=add, ref=ref, stats=stats)


def conv3x3_concat_upsample(B=2, c1=64, c2=32, cout=32, H=12, W=12, key=1100, groups=8):
    """Two sources: c1 channels at half resolution (nearest x2 on load) ++ c2 channels."""
    x1, x2 = trits((B, c1, H // 2, W // 2), key), trits((B, c2, H, W), key + 1)
    w, b = trits((cout, c1 + c2, 3, 3), key + 2), bias_for(cout, key + 3)
    xc = torch.cat([F.interpolate(x1, scale_factor=2, mode="nearest"), x2], 1)
    ref, stats = _conv(xc, w, b, 1, groups=groups)
    return NS(x1=x1, x2=x2, w=w, b=b, ref=ref, stats=stats)


def conv3x3_side(B=2, c1=64, c2=32, cout=64, H=17, W=23, key=1200):
    """A 3x3 convolution of a concatenation and a 1x1 convolution of the same input (the res_conv side output)."""
    x1, x2 = trits((B, c1, H, W), key), trits((B, c2, H, W), key + 1)
    w, b = trits((cout, c1 + c2, 3, 3), key + 2), bias_for(cout, key + 3)
    wr, br = trits((cout, c1 + c2, 1, 1), key + 4), bias_for(cout, key + 5)
    xc = torch.cat([x1, x2], 1)
    ref, stats = _conv(xc, w, b, 1, groups=8)
    ref_side, _ = _conv(xc, wr, br, 0)
    return NS(x1=x1, x2=x2, w=w, b=b, wr=wr, br=br, ref=ref, ref_side=ref_side, stats=stats)


def conv1x1(B, cin, cout, H, W, key=2000, frac=False, residual=False, per_batch=False):
    """Plain / + integer residual / a weight per batch element (w [B, cout, cin, 1, 1])."""
    x, b = trits((B, cin, H, W), key), bias_for(cout, key + 2, frac)
    res = ints((B, cout, H, W), key + 3, -4, 4) if residual else None
    if per_batch:
        w = trits((B, cout, cin, 1, 1), key + 1)
        parts = [_conv(x[i:i + 1], w[i], b, 0, residual=None if res is None else res[i:i + 1], frac=frac)[0] for i in range(B)]
        ref = torch.cat(parts)
    else:
        w = trits((cout, cin, 1, 1), key + 1)
        ref, _ = _conv(x, w, b, 0, residual=res, frac=frac)
    return NS(x=x, w=w, b=b, res=res, ref=ref)


def conv1x1_concat(B=1, c1=64, c2=32, cout=64, H=12, W=10, key=2100):
    x1, x2 = trits((B, c1, H, W), key), trits((B, c2, H, W), key + 1)
    w, b = trits((cout, c1 + c2, 1, 1), key + 2), bias_for(cout, key + 3)
    ref, _ = _conv(torch.cat([x1, x2], 1), w, b, 0)
    return NS(x1=x1, x2=x2, w=w, b=b, ref=ref)


def unshuffle(x):
    """'b c (h p1) (w p2) -> b (c p1 p2) h w' (Downsample's rearrangement)."""
    B, c, H2, W2 = x.shape
    return x.reshape(B, c, H2 // 2, 2, W2 // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(B, 4 * c, H2 // 2, W2 // 2)


def conv1x1_unshuffle(B=1, c=32, cout=64, H=12, W=10, key=2200):
    """Pixel-unshuffle of a [B, c, 2H, 2W] map, then a 1x1 convolution over its 4c channels."""
    x = trits((B, c, 2 * H, 2 * W), key)
    w, b = trits((cout, 4 * c, 1, 1), key + 1), bias_for(cout, key + 2)
    ref, _ = _conv(unshuffle(x), w, b, 0)
    return NS(x=x, w=w, b=b, ref=ref)


def conv_image(cin, ks, H, W, B=2, key=3000):
    """ld_conv_image: a small-Cin direct convolution from the fp32 image, 32 output channels, 16 statistics groups."""
    x, w, b = trits((B, cin, H, W), key), trits((32, cin, ks, ks), key + 1), bias_for(32, key + 2)
    ref, stats = _conv(x, w, b, ks // 2, groups=16)
    return NS(x=x, w=w, b=b, ref=ref, stats=stats)


def stem(cin, H, W, variant="int", B=2, key=3100):
    """The 7x7 MFMA stem.  ``int``: integer operands; ``frac``: + odd/1024 in the bias (1b); ``split``: image values
    k/256 with |k| <= 383, which need the lo term of the kernel's bf16 hi/lo split, weights in {-1, 0, 1}; ``mirror``:
    the weights take the k/256 values and the image the {-1, 0, 1} (1c).  A sum of at most 147 such terms is a multiple
    of 1/256 below 2^8: exact in fp32 in any order; the stored value is its one rounding."""
    xs, ws = (B, cin, H, W), (32, cin, 7, 7)
    if variant == "split":
        x, w = ints(xs, key, -383, 383) / 256, trits(ws, key + 1)
    elif variant == "mirror":
        x, w = trits(xs, key), ints(ws, key + 1, -383, 383) / 256
    else:
        x, w = trits(xs, key), trits(ws, key + 1)
    b = bias_for(32, key + 2, variant == "frac")
    integer = variant == "int"
    ref64 = F.conv2d(x.double(), w.double(), b.double(), padding=3)
    ref32 = F.conv2d(x, w, b, padding=3)
    check_exact(ref32, ref64, integer=integer)
    if variant in ("split", "mirror"):       # the lo term is exercised: some operand is not a bf16 value
        t = x if variant == "split" else w
        assert not torch.equal(t.to(torch.bfloat16).float(), t)
        lo = t - t.to(torch.bfloat16).float()
        assert torch.equal(lo.to(torch.bfloat16).float(), lo)          # ... and hi + lo holds it exactly
    return NS(x=x, w=w, b=b, ref=ref32)


def final_conv(cin, cout, H=9, W=11, B=2, key=3200, frac=False):
    x, w, b = trits((B, cin, H, W), key), trits((cout, cin, 1, 1), key + 1), bias_for(cout, key + 2, frac)
    ref, _ = _conv(x, w, b, 0, frac=frac)
    return NS(x=x, w=w, b=b, ref=ref)


def two_term_scale(dtype):
    """Weights k / scale with |k| < 1.5 scale: one significant bit more than the storage type's hi part holds (bf16:
    8 bits -> k/256, |k| <= 383; fp16 holds k/256 exactly, so its probe uses k/4096, |k| <= 6143, 13 bits)."""
    return 256 if dtype == "bf16" else 4096


def two_term(kind, dtype, key=3300):
    """Weights that need hi + lo in ``dtype`` (two_term_scale), activations in {-1, 0, 1}: with weight_terms = 2 the
    kernel's result is the exact one, stored once; with one term the weights themselves are rounded and it is not."""
    s = two_term_scale(dtype)
    kmax = s + s // 2 - 1
    B, c1, c2, cout, H, W = 2, 64, 32, 64, 16, 16
    if kind == "3x3":                         # concat + nearest x2 on the first source
        x1, x2 = trits((B, c1, H // 2, W // 2), key), trits((B, c2, H, W), key + 1)
        w = ints((cout, c1 + c2, 3, 3), key + 2, -kmax, kmax) / s
        xc, pad = torch.cat([F.interpolate(x1, scale_factor=2, mode="nearest"), x2], 1), 1
    else:
        x1, x2 = trits((B, c1, H, W), key + 10), trits((B, c2, H, W), key + 11)
        w = ints((cout, c1 + c2, 1, 1), key + 12, -kmax, kmax) / s
        xc, pad = torch.cat([x1, x2], 1), 0
    b = bias_for(cout, key + 3)
    ref64 = F.conv2d(xc.double(), w.double(), b.double(), padding=pad)
    ref32 = F.conv2d(xc, w, b, padding=pad)
    check_exact(ref32, ref64, integer=False, limit=4096.0)              # multiples of 1/s below 2^12: at most 24 bits
    hi = w.to(TDT[dtype]).float()
    lo = w - hi
    assert not torch.equal(hi, w) and torch.equal(lo.to(TDT[dtype]).float(), lo)      # one term rounds, two are exact
    ref1 = F.conv2d(xc.double(), hi.double(), b.double(), padding=pad).float()          # what one term computes
    assert not torch.equal(stored(ref1, dtype), stored(ref32, dtype))
    return NS(x1=x1, x2=x2, w=w, b=b, ref=ref32)


# --------------------------------------------------------------------------------------------- full attention (1d, 1e)
HEADS, DH = 4, 32
HID = HEADS * DH


def _pack_qkv(q, k, v):
    """[B, heads, n, 32] x 3 -> the kernels' NHWC qkv tensor [B, n, 3 * hidden] (q | k | v, head-major channels)."""
    B, heads, n, _ = q.shape
    return torch.cat([t.permute(0, 2, 1, 3).reshape(B, n, heads * DH) for t in (q, k, v)], dim=-1).contiguous()


def _unpack_out(o):
    """[B, heads, n, 32] -> [B, n, hidden]."""
    B, heads, n, _ = o.shape
    return o.permute(0, 2, 1, 3).reshape(B, n, heads * DH).contiguous()


def attention_torch(qkv, dtype=torch.float32):
    """softmax(q k^T) v per (batch, head) in plain torch (q pre-scaled), qkv and result in the kernels' layout (the head
    count is the tensor's: 3 * heads * 32 channels)."""
    B, n, c3 = qkv.shape
    heads = c3 // (3 * DH)
    q, k, v = [t.reshape(B, n, heads, DH).permute(0, 2, 1, 3).to(dtype) for t in qkv.chunk(3, dim=-1)]
    return _unpack_out((q @ k.transpose(-1, -2)).softmax(dim=-1) @ v)


@functools.lru_cache(maxsize=None)
def attention_onehot(n, B=2, key=4000, heads=HEADS):
    """n distinct keys in {-1, +1}^32 per (batch, head), q_i = 64 k_pi(i) for a permutation pi, v integers in [-8, 8].
    The winning logit is 64 * 32 = 2048 and every other one at least 128 lower (2 * 64 per differing sign), so every
    other exp() is zero in fp32 and the result is the gather v[pi(i)], exactly, whatever the tiling of the keys.  Every
    (batch, head) has its own keys, permutation and values: a head that reads another head's slice gathers other rows."""
    for attempt in range(8):
        k = torch.from_numpy(np.where(rng.uniform((B, heads, n, DH), SEED, key + 10 * attempt) < 0.5, -1.0, 1.0).astype(np.float32))
        top2 = (k @ k.transpose(-1, -2)).topk(2, dim=-1).values          # [.., 0] = 32 (itself), [.., 1] = the nearest other key
        if float(top2[..., 1].max()) < DH:
            break
    else:
        raise AssertionError("no draw of distinct keys")
    pi = torch.from_numpy(np.argsort(rng.uniform((B, heads, n), SEED, key + 1), axis=-1))
    q = 64.0 * torch.gather(k, 2, pi[..., None].expand(-1, -1, -1, DH))
    v = ints((B, heads, n, DH), key + 2, -8, 8)
    gap = 64.0 * (DH - float(top2[..., 1].max()))
    assert gap >= 128.0, gap
    assert float(np.exp(np.float32(-gap))) == 0.0                         # exp of every losing logit is zero in fp32
    for t in (q, k, v):
        for dt in ("bf16", "fp16"):
            check_representable(t, dt)
    ref = _unpack_out(torch.gather(v, 2, pi[..., None].expand(-1, -1, -1, DH)))
    qkv = _pack_qkv(q, k, v)
    assert torch.equal(attention_torch(qkv), ref)                         # fp32 torch reproduces the gather bit for bit
    if heads > 1:                                                         # no two heads of an image gather the same rows
        per_head = ref.reshape(B, n, heads, DH)
        assert all(not torch.equal(per_head[:, :, a], per_head[:, :, b]) for a in range(heads) for b in range(a))
    return NS(qkv=qkv, ref=ref, gap=gap)


@functools.lru_cache(maxsize=None)
def attention_uniform(n, B=2, key=4100, heads=HEADS):
    """q = 0: every key weighs 1/n.  Even channels of v hold +-m pairs (4 <= m <= 8, one zero row if n is odd) in a
    shuffled order, so they sum to exactly zero over the keys; odd channels are the constant 1.  Expected: 0 on even
    channels, 1 on odd ones, for every query.  ``d_even`` (relative to max |v| = 8) and ``d_odd`` are fp32 torch's own
    distances from that fp64 value on this probe (it normalises P before the product)."""
    k = torch.from_numpy(np.where(rng.uniform((B, heads, n, DH), SEED, key) < 0.5, -1.0, 1.0).astype(np.float32))
    q = torch.zeros(B, heads, n, DH)
    m = ints((B, heads, n // 2, DH), key + 1, 4, 8)
    col = torch.cat([m, -m] + ([torch.zeros(B, heads, 1, DH)] if n % 2 else []), dim=2)
    order = torch.from_numpy(np.argsort(rng.uniform((B, heads, n, DH), SEED, key + 2), axis=2))
    v = torch.gather(col, 2, order)
    v[..., 1::2] = 1.0
    assert bool((v[..., 0::2].double().sum(2) == 0).all())
    nz = v[..., 0::2].abs()
    assert float(nz.max()) == 8.0 and float(nz[nz > 0].min()) == 4.0 and int((nz == 0).sum()) == (n % 2) * B * heads * (DH // 2)
    for dt in ("bf16", "fp16"):
        check_representable(v, dt)
    ref = torch.zeros(B, n, heads * DH, dtype=torch.float64)
    ref[..., 1::2] = 1.0
    qkv = _pack_qkv(q, k, v)
    assert float((attention_torch(qkv, torch.float64) - ref).abs().max()) < 1e-13     # (1/n) * (a sum that is exactly 0 or n)
    t32 = attention_torch(qkv).double()
    d_even = float(t32[..., 0::2].abs().max()) / 8.0
    d_odd = float((t32[..., 1::2] - 1.0).abs().max())
    return NS(qkv=qkv, ref=ref, d_even=d_even, d_odd=d_odd)


# --------------------------------------------------------------------------------------------- fused linear attention (1f)
@functools.lru_cache(maxsize=None)
def linattn_uniform(C, H, W, B=2, key=5000, heads=HEADS):
    """to_qkv with all k rows zero (the k softmax over the pixels is uniform, its maximum and any Cauchy-Schwarz
    shift are 0) and v rows that each select ONE input channel.  x is +-1 on ``nnz`` channels per pixel (64 of them for
    C >= 64 -- all of C = 64, the even ones of C = 128 -- and the 16 even ones for C = 32) and 0 elsewhere, so the
    pixel norm is sqrt(nnz) = 8 or 4, and with g * sqrt(C) = ``scale`` = that power of two the RMS-normalised value,
    hence v, is +-1 up to the error of the reciprocal norm.  Non-zero channel j is balanced for even j (sums to zero
    over an even number of pixels, to +1 over an odd one: ceil(n / 2) pixels hold +1) and constant (+1 for j = 1 mod 4,
    -1 for j = 3 mod 4) for odd j; v row (h, e) selects non-zero channel (32 h + e) mod nnz, so even e are balanced and
    odd e constant.  Expected: ctxn[b, h, d, e] = mean_n v_e, the same for every d: 0 (1 / n for odd n) or +-1."""
    n = H * W
    hid = heads * DH
    nnz = 64 if C >= 64 else 16
    chans = torch.arange(0, C, C // nnz)
    half = torch.cat([torch.ones(n - n // 2), -torch.ones(n // 2)])
    xs = torch.empty(B, nnz, n)
    order = torch.from_numpy(np.argsort(rng.uniform((B, nnz, n), SEED, key), axis=-1))
    xs[:] = half[order]
    xs[:, 1::4] = 1.0
    xs[:, 3::4] = -1.0
    x = torch.zeros(B, C, n)
    x[:, chans] = xs
    x = x.reshape(B, C, H, W)
    assert bool((x.double().pow(2).sum(1) == nnz).all())
    scale = float(nnz) ** 0.5                                              # g * sqrt(C): 8 or 4
    w = torch.zeros(3 * hid, C)
    sel = torch.tensor([[(DH * h + e) % nnz for e in range(DH)] for h in range(heads)])
    for h in range(heads):
        for e in range(DH):
            w[2 * hid + DH * h + e, chans[sel[h, e]]] = 1.0
    v64 = xs.double()[:, sel.flatten()].reshape(B, heads, DH, n)           # exact v: +-1
    total = v64.sum(-1)                                                    # [B, heads, e]: an exact integer
    assert bool((total[..., 0::2] == n % 2).all()) and bool((total[..., 1::2].abs() == n).all())
    mean = total / n
    ref = mean[:, :, None, :].expand(B, heads, DH, DH).contiguous()
    # fp32 torch on the same probe: F.normalize * scale, the 1x1 projection, softmax over the pixels, the context
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12) * scale
    kv = F.conv2d(xn, w[:, :, None, None]).reshape(B, 3, heads, DH, n)
    t32 = torch.einsum("bhdn,bhen->bhde", kv[:, 1].softmax(dim=-1), kv[:, 2]).double()
    d = float((t32 - ref).abs().max())                                     # relative to |v| = 1
    return NS(x=x, w=w[:, :, None, None].contiguous(), scale=torch.full((C,), scale), ref=ref, d=d)


# --------------------------------------------------------------------------------------------- fused linear attention, output half (1g)
LINOUT_CHANNELS = [32, 64, 128]
LINOUT_SIZES = [49, 196, 784, 1024]         # one partial 128-pixel tile; a tile + a tail whose last 16-group holds 4 pixels;
                                            # six tiles + a 16-pixel tail; full tiles only
QWIN = 128.0                                # the winning q logit: exp(-128) is zero in fp32 (and exp2(-128 log2 e) on the device)


def linout_contract(x, wq, ctxn, wout, bias, g2, q_scale=1.0, dtype=None):
    """What ld_linattn_out computes, in fp64: out = RMSNorm(M_b (softmax_d(W_q x / |x|) * q_scale) + bias) * g2 + x with
    M_b[c, 32 h + d] = sum_e W_out[c, 32 h + e] ctxn[b, h, d, e] (ld_linattn_fold).  x [B, C, n]; wq [128, C] with
    g sqrt(C) folded in (the sum of the stored terms, or the unrounded product); ctxn [B, 4, 32, 32]; wout [C, 128]; g2 =
    to_out.1.g * sqrt(C).  ``dtype``: the kernel's two internal rounding points -- M_b and the scaled softmax as storage
    holds them (both are operands of the second matrix product) -- and the stored output; None: no rounding at all."""
    B, C, n = x.shape
    rnd = (lambda t: t) if dtype is None else (lambda t: t.float().to(TDT[dtype]).double())
    x, wq, ctxn, wout, bias, g2 = (t.double() for t in (x, wq, ctxn, wout, bias, g2))
    M = rnd(torch.einsum("che,bhde->bchd", wout.reshape(C, HEADS, DH), ctxn).reshape(B, C, HID))
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    q = torch.einsum("kc,bcn->bkn", wq, xn).reshape(B, HEADS, DH, n)
    q = rnd(q.softmax(dim=2) * q_scale).reshape(B, HID, n)
    y = torch.einsum("bck,bkn->bcn", M, q) + bias[None, :, None]
    return rnd(y / y.norm(dim=1, keepdim=True).clamp_min(1e-12) * g2[None, :, None] + x)


def _linout_tail(C, key):
    """The part both probes share: bias +-2, a target y in {-1, +1} per (channel, k-slot) reached by W_out = y - bias in
    {-3, -1, 1, 3}, and the gain g2 = k_c sqrt(C) with k_c in +-{1..4}.  Every |y_c| is 1, so RMSNorm gives +-1 / sqrt(C)
    and the block's value is y_c k_c + x: an integer, |.| <= 36, which 16-bit storage holds exactly although
    fl(1 / sqrt(C)) * fl(k sqrt(C)) is only k (1 + 1e-7) for C = 32 and 128 -- as long as the sum does not cancel to 0,
    where that 1e-7 would be all that is left: the probes' x is 0 or a multiple of 8, |k_c| <= 4."""
    sign = lambda shape, k: torch.from_numpy(np.where(rng.uniform(shape, SEED, k) < 0.5, -1.0, 1.0).astype(np.float32))
    bias = 2.0 * sign((C,), key)
    target = sign((C, HID), key + 1)
    gain = ints((C,), key + 2, 1, 4) * sign((C,), key + 3)
    g2 = (gain.double() * float(C) ** 0.5).float()
    return bias, target, gain, g2


def _linout_check(p, integer_limit=36.0):
    """Preconditions of a linout probe: the fp64 contract gives the stated integers (to 1e-12), with the kernel's
    rounding points too, for both storage types; and an fp32 evaluation, stored once, gives them bit for bit."""
    assert is_integer(p.ref) and 1.0 <= float(p.ref.abs().min()) and float(p.ref.abs().max()) <= integer_limit
    for dt in ("bf16", "fp16"):
        for t in (p.x, p.wq, p.wout, p.bias, p.ctxn):
            check_representable(t, dt)
        assert float((linout_contract(p.x, p.wq, p.ctxn, p.wout, p.bias, p.g2) - p.ref.double()).abs().max()) < 1e-6     # g2 is an fp32 value
        assert torch.equal(linout_contract(p.x, p.wq, p.ctxn, p.wout, p.bias, p.g2, dtype=dt), p.ref.double())
    B, C, n = p.x.shape
    M = torch.einsum("che,bhde->bchd", p.wout.reshape(C, HEADS, DH), p.ctxn).reshape(B, C, HID)          # fp32 throughout
    q = torch.einsum("kc,bcn->bkn", p.wq, p.x / p.x.norm(dim=1, keepdim=True).clamp_min(1e-12)).reshape(B, HEADS, DH, n)
    y = torch.einsum("bck,bkn->bcn", M, q.softmax(dim=2).reshape(B, HID, n)) + p.bias[None, :, None]
    out32 = y * torch.rsqrt((y * y).sum(1, keepdim=True)) * p.g2[None, :, None] + p.x
    for dt in ("bf16", "fp16"):
        assert torch.equal(stored(out32, dt), p.ref)


def linout_sel(h, j):
    """The q channel (within head h) that input channel j selects in the one-hot probe: all 32 for every head."""
    return (j + 8 * h + j // DH) % DH


@functools.lru_cache(maxsize=None)
def linout_onehot(C, n, key=6000):
    """ld_linattn_out with B = 4.  Every pixel of x has ONE non-zero channel j (a draw per pixel) holding 8, 16 or 32, so
    the normalised pixel is the unit vector e_j whatever the reciprocal norm's last bit is; W_q[32 h + sel(h, j), j] =
    128 and 0 elsewhere (scale = 1), so in every head the winning logit is 128 and the 31 others 0: every other exp is
    zero and softmax_d(q) is exactly one-hot at d = sel(h, j) -- with the per-pixel maximum and with qshift = 128 alike.
    ctxn[b] is the identity for head b mod 4 and zero for the others, so M_b is the head's block of W_out and
    y_c = W_out[c, 32 (b mod 4) + sel(b mod 4, j)] + bias_c = +-1 (``_linout_tail``).  Expected: y_c k_c + x, integers.
    A q channel in another k-slot or a head taken twice picks another column of W_out (another sign pattern over c), a
    wrong M_b batch offset another head's block, a residual from the wrong fragment moves the one non-zero x."""
    B = 4
    bias, target, gain, g2 = _linout_tail(C, key)
    j = ints((B, n), key + 10, 0, C - 1).long()
    a = 2.0 ** ints((B, n), key + 11, 3, 5)
    x = torch.zeros(B, C, n)
    x.scatter_(1, j[:, None, :], a[:, None, :])
    wq = torch.zeros(HID, C)
    for h in range(HEADS):
        for c in range(C):
            wq[DH * h + linout_sel(h, c), c] = QWIN
    ctxn = torch.zeros(B, HEADS, DH, DH)
    for b in range(B):
        ctxn[b, b % HEADS] = torch.eye(DH)
    wout = target - bias[:, None]
    hb = torch.arange(B) % HEADS
    col = DH * hb[:, None] + linout_sel(hb[:, None], j)                     # [B, n]: the one k-slot that is switched on
    ref = target[:, col].permute(1, 0, 2) * gain[None, :, None] + x       # [B, C, n]
    assert all(len({linout_sel(h, c) for c in range(DH)}) == DH for h in range(HEADS))
    assert len(set(j.flatten().tolist())) == C or n < 4 * C               # every channel is some pixel's (at the larger sizes)
    p = NS(x=x, wq=wq, scale=torch.ones(C), ctxn=ctxn, wout=wout, bias=bias, g2=g2, ref=ref, qshift=torch.full((HEADS,), QWIN))
    _linout_check(p)
    return p


@functools.lru_cache(maxsize=None)
def linout_uniform(C, n, key=6100):
    """ld_linattn_out with W_q = 0 (B = 2): q is 0, softmax_d(q) is 1 / 32 for every d -- with the per-pixel maximum and
    with qshift = 0 -- and the second product is the row sum of M_b over all 128 k-slots / 32.  ctxn[b, h] is a
    permutation matrix (a draw per batch and head), so M_b is W_out with the columns of each head permuted: entries +-1,
    row c holding (128 + S_c) / 2 ones with S_c = 32 (y_c - bias_c) in {+-32, +-96}; every partial sum is a multiple of
    1 / 32 below 4, exact in any order.  x: multiples of 8 in [-16, 16].  Expected: y_c k_c + x (``_linout_tail``)."""
    B = 2
    bias, target, gain, g2 = _linout_tail(C, key)
    t = target[:, 0]                                                       # y_c
    S = (32 * (t - bias)).long()
    assert set(S.tolist()) <= {-96, -32, 32, 96}
    wout = torch.empty(C, HID)
    order = torch.from_numpy(np.argsort(rng.uniform((C, HID), SEED, key + 10), axis=-1))
    for c in range(C):
        plus = (HID + int(S[c])) // 2
        row = torch.cat([torch.ones(plus), -torch.ones(HID - plus)])
        wout[c] = row[order[c]]
    assert torch.equal(wout.sum(1).long(), S)
    perm = torch.from_numpy(np.argsort(rng.uniform((B, HEADS, DH), SEED, key + 11), axis=-1))
    ctxn = torch.zeros(B, HEADS, DH, DH)
    ctxn.scatter_(3, perm[..., None], 1.0)
    assert bool((ctxn.sum(2) == 1).all()) and bool((ctxn.sum(3) == 1).all())
    x = 8.0 * ints((B, C, n), key + 12, -2, 2)
    ref = (t * gain)[None, :, None] + x
    p = NS(x=x, wq=torch.zeros(HID, C), scale=torch.ones(C), ctxn=ctxn, wout=wout, bias=bias, g2=g2, ref=ref, qshift=torch.zeros(HEADS))
    _linout_check(p)
    return p


def linout_swapped_slots(p, dtype="bf16"):
    """The mutation the one-hot probe is for, in torch: k-slots 4 and 20 of every head's M_b exchanged (two channel slots
    of the chained-operand order of ld_linattn_fold(perm = 1) swapped).  Returns the block's stored value."""
    idx = torch.arange(HID)
    d = idx % DH
    idx = torch.where(d == 4, idx + 16, torch.where(d == 20, idx - 16, idx))
    return linout_contract(p.x, p.wq[idx], p.ctxn, p.wout, p.bias, p.g2, dtype=dtype).float()


@functools.lru_cache(maxsize=None)
def linout_random(C, n, dtype, sharp=False, key=6200):
    """Random operands for ld_linattn_out (B = 2): x in [-1, 1] (as storage holds it: it is the kernel's input, not one of
    its roundings), to_qkv's q rows in [-0.3, 0.3] with norm.g in [0.5, 1.5], to_out.0 in [-0.3, 0.3], its bias in
    [-1, 1], to_out.1.g in [2, 4] -- the attention branch is at least as large as the residual --, and a context of
    the magnitude a softmax context has: ctxn = softmax_n(k) v^T of random k, v in [-1.5, 1.5] over 64 pixels.  ``ref``:
    the fp64 value of the UNROUNDED operands; ``rest[terms]``: linout_contract with W_q as one or two stored terms and
    the kernel's rounding points; ``d[terms]``: its distance from ref (max |.| / max |ref|).  ``sharp``: the q rows times
    16 -- logits of +-20, where the rounding of W_q moves softmax_d(q) by more than its own rounding to storage does, so
    that the second weight term shows in the output (with the plain draw it disappears behind the roundings of q and of
    the output: d[2] / d[1] is 1 to three digits)."""
    B = 2
    u = lambda shape, k, lo=-1.0, hi=1.0: torch.from_numpy(rng.uniform(shape, SEED, key + k, lo, hi))
    x = u((B, C, n), 0).to(TDT[dtype]).float()
    g = u((C,), 1, 0.5, 1.5)
    scale = (g * float(C) ** 0.5).contiguous()
    wq = u((HID, C), 2, -0.3, 0.3) * (16.0 if sharp else 1.0)
    wout, bias = u((C, HID), 3, -0.3, 0.3), u((C,), 4)
    g2 = (u((C,), 5, 2.0, 4.0) * float(C) ** 0.5).contiguous()
    k, v = u((B, HEADS, DH, 64), 6, -1.5, 1.5), u((B, HEADS, DH, 64), 7, -1.5, 1.5)
    ctxn = torch.einsum("bhdn,bhen->bhde", k.double().softmax(dim=-1), v.double()).float()
    q_scale = DH ** -0.5
    ws = wq * scale[None, :]                                               # fp32, as ld_pack_conv_weight_terms forms it
    hi = ws.to(TDT[dtype]).float()
    lo = (ws - hi).to(TDT[dtype]).float()
    ref = linout_contract(x, wq.double() * scale.double()[None, :], ctxn, wout, bias, g2, q_scale)
    rest = {1: linout_contract(x, hi, ctxn, wout, bias, g2, q_scale, dtype=dtype),
            2: linout_contract(x, hi.double() + lo.double(), ctxn, wout, bias, g2, q_scale, dtype=dtype)}
    top = float(ref.abs().max())
    d = {t: float((r - ref).abs().max()) / top for t, r in rest.items()}
    d_rms = {t: float((r - ref).pow(2).mean().sqrt()) / top for t, r in rest.items()}
    branch = float((ref - x.double()).abs().max())
    assert branch >= float(x.abs().max())                                  # the attention branch is not hidden behind the residual
    qb = (hi.norm(dim=1) * 1.01).reshape(HEADS, DH).amax(dim=1)            # the Cauchy-Schwarz bound of q per head (unet.py)
    return NS(x=x, wq=wq, scale=scale, ctxn=ctxn, wout=wout, bias=bias, g2=g2, q_scale=q_scale, qshift=qb.contiguous(), ref=ref,
              rest=rest, d=d, d_rms=d_rms, top=top)


# --------------------------------------------------------------------------------------------- the motivating mutation
def misread_last_channel(x, w, b, tap=(1, 1)):
    """A 3x3 convolution whose LAST input channel reads its neighbour channel at ONE tap (fp32 torch)."""
    cin = x.shape[1]
    xa = torch.cat([x, x[:, cin - 2:cin - 1]], 1)
    wa = torch.cat([w, torch.zeros_like(w[:, :1])], 1)
    wa[:, cin, tap[0], tap[1]] = w[:, cin - 1, tap[0], tap[1]]
    wa[:, cin - 1, tap[0], tap[1]] = 0.0
    return F.conv2d(xa, wa, b, padding=1)
