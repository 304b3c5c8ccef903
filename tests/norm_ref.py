"""References of the GroupNorm / FiLM path (build_gn_coef + affine_act_n of csrc/common.hip.h and the copy of that
arithmetic in csrc/conv3x3_s32.hip) in pure torch on the CPU, the input builders, the case lists and the comparison the
GPU tests use.  No device import (as tests/exact_probes.py and tests/pointwise_ref.py).

Three evaluations of act(GN(x) * (scale + 1) + shift) (+ second operand, final activation, 2x2 max-pool), all of the
STORED input (x already rounded to the storage type):

* ``ref64``: the direct fp64 form act(((x - mean) * rstd * gamma + beta) * (scale + 1) + shift), biased variance, eps
  1e-5, statistics = the fp64 sums of the stored x.  The yardstick.
* ``restate32`` (``fast=None``): the kernels' operation order with PRECISE = true: stripe sums, 1/n, mean, the clamped
  variance and rstd in fp64, mean and rstd rounded to fp32, a = rstd * gamma, s = beta - mean * a, a *= sc,
  s = s * sc + sh in fp32 (the library is built with -ffp-contract=off: every product and sum rounds on its own),
  fmaf(x, a, s) as the fp32 rounding of the fp64 x * a + s, SiLU as v / (1 + expf(-v)) with expf the correctly rounded
  exponential (the fp64 exp rounded once, as silu_f<true> evaluates it).  ``d`` = its largest distance
  from ref64, per (sample, group).
* ``restate_fast`` (``fast`` = five signs): the 16-bit-storage path, whose five approximated results -- v_rcp_f32 for
  1/n, v_rsq_f32 for rstd, the -log2(e) * v product, v_exp_f32 and v_rcp_f32 of the sigmoid -- are each moved by one fp32
  ulp up or down.  ``d_fast`` = the largest distance from ref64 over the 32 sign combinations, per (sample, group): the
  allowance for the fast path, derived here and never from a GPU value.

``compare`` is the rule of the GPU tests, per (sample, group) because the planted groups differ by orders of magnitude
in conditioning (see its docstring).  tests/test_norm_ref.py pins ref64 to oracle/unet_ref.py, proves the builders'
preconditions for every case below and shows that ``compare`` rejects a set of subtly wrong kernels (``mut``), without
a GPU.

Draws come from the package's counter generator (rng.uniform, seed 1234, one stream per tensor).
"""
import functools
import itertools
from types import SimpleNamespace as NS

import numpy as np
import torch

from localdiffusion_hallucination_amd import rng

SEED = 1234
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DTYPES = ["fp32", "bf16", "fp16"]
LOWP = ["bf16", "fp16"]
ELEMS = {"fp32": 4, "bf16": 8, "fp16": 8}          # DT<T>::E: elements of one 16-byte fragment
MANT = {"bf16": 7, "fp16": 10}                     # stored fraction bits
EMIN = {"bf16": -126, "fp16": -14}                 # exponent of the smallest normal
STRIPES = 16                                        # LD_STAT_STRIPES
EPS = 1e-5
ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2
T_ROWS = 5                                          # rows of the FiLM table in table mode
SIGNS = list(itertools.product((-1, 1), repeat=5))  # (1/n, rstd, -log2(e) * v, exp, reciprocal)
# planted channels (every C here is >= 32): gamma = 0, FiLM scale = -1 exactly, FiLM shift = -90 / +90
CH_GAMMA0, CH_SCALE, CH_NEG, CH_POS = 5, 9, 14, 19
CONST_VALUE = 16.0                                  # the constant group: representable in every storage type


def uni(shape, key, lo=-1.0, hi=1.0):
    return torch.from_numpy(rng.uniform(shape, SEED, key, lo, hi))


def stored(x, dtype):
    """One round-to-nearest-even to ``dtype`` storage, widened again."""
    return x.to(TDT[dtype]).float()


def nudge(v, k):
    """fp32 ``v`` moved by ``k`` (-1, 0, +1) fp32 ulps."""
    if k == 0:
        return v
    return torch.nextafter(v, torch.full_like(v, float("inf") if k > 0 else float("-inf")))


# ------------------------------------------------------------------------------------------------ input builders
def planted_moments(B, G):
    """mu, sigma [B, G]: neighbouring (b, g) are >= 0.5 apart in mu and >= 1.5x apart in sigma (x = mu + sigma * u, u
    uniform on [-1, 1)); then the constant group (sigma = 0) and, in ONE sample, the group with |mean| / std ~ 30."""
    b, g = torch.meshgrid(torch.arange(B), torch.arange(G), indexing="ij")
    mu = 0.5 * (((3 * g + 5 * b) % 7) - 3).double()             # steps of 3 (mod 7) along g, 5 (mod 7) along b: >= 1.0 apart
    sigma = 0.25 * 2.0 ** ((g + 2 * b) % 4).double()            # 2x / 8x along g, 4x along b
    cb, hb = const_group(B, G), high_group(B, G)
    mu[cb], sigma[cb] = CONST_VALUE, 0.0
    mu[hb], sigma[hb] = 2.125, 0.125                             # std = 0.125 / sqrt(3): ratio 29.4; 16 bf16 levels across
    return mu, sigma


def const_group(B, G):
    return (min(1, B - 1), 1)


def high_group(B, G):
    return (B - 1, G - 1)


def make_x(B, C, H, W, G, dtype, key):
    """Stored NCHW activations with the planted per-(sample, group) moments."""
    mu, sigma = planted_moments(B, G)
    gi = torch.arange(C) // (C // G)
    u = uni((B, C, H, W), key).double()
    x = mu[:, gi][:, :, None, None] + sigma[:, gi][:, :, None, None] * u
    return stored(x.float(), dtype)


def make_params(C, key, film, B):
    """gamma / beta distinct per channel, one gamma = 0.  ``film``: None | 'shared' ([1, 2C]) | 'batch' ([B, 2C]) |
    'table' ([T_ROWS, 2C]); rows are [scale C | shift C], distinct per row, with scale = -1 and shift = -90 / +90 planted
    in every row."""
    gamma, beta = uni((C,), key, 0.5, 1.5), uni((C,), key + 1, -0.3, 0.3)
    gamma[CH_GAMMA0] = 0.0
    rows = None
    if film is not None:
        n = {"shared": 1, "batch": B, "table": T_ROWS}[film]
        rows = torch.cat([uni((n, C), key + 2, -0.5, 0.5), uni((n, C), key + 3, -0.3, 0.3)], 1)
        rows[:, CH_SCALE], rows[:, C + CH_NEG], rows[:, C + CH_POS] = -1.0, -90.0, 90.0
    return gamma, beta, rows


def group_sums(x, G):
    """[B, G, 2] fp64 (sum, sum of squares) of a stored NCHW tensor."""
    g = x.double().reshape(x.shape[0], G, -1)
    return torch.stack([g.sum(-1), (g * g).sum(-1)], -1)


def striped(sums, layout):
    """[B, STRIPES, G, 2]: 'spread' puts unequal shares (1 : 2 : ... : 16) into the stripes, 'last' puts everything
    into the last one.  (The shares of 'spread' add up to the sum only to an fp64 rounding: ref64 takes the sums
    themselves, the restatements add the stripes as the kernels do.)"""
    out = torch.zeros(sums.shape[0], STRIPES, *sums.shape[1:], dtype=torch.float64)
    if layout == "last":
        out[:, STRIPES - 1] = sums
    else:
        wgt = torch.arange(1, STRIPES + 1, dtype=torch.float64)
        out[:] = sums[:, None] * (wgt / wgt.sum())[None, :, None, None]
    return out


def operand(x, G, gamma, beta, act=ACT_NONE, film=None, film_kind=None, t=0, layout="spread"):
    """One normalised operand: x [B, C, h, w] stored, statistics over its own h * w pixels."""
    return NS(x=x, G=G, gamma=gamma, beta=beta, act=act, film=film, film_kind=film_kind, t=t,
              stats=striped(group_sums(x, G), layout), npix=x.shape[2] * x.shape[3])


def film_rows(op, B, mut=None):
    """(scale, shift) [B, C] as the kernels address them: film + t * tstride + b * bstride, shift at + C."""
    if op.film is None:
        return None
    C = op.x.shape[1]
    if op.film_kind == "batch":
        idx = torch.zeros(B, dtype=torch.long) if mut == "film_row0" else torch.arange(B)
    elif op.film_kind == "table":
        idx = torch.full((B,), op.t + (1 if mut == "t_off" else 0))
    else:
        idx = torch.zeros(B, dtype=torch.long)
    rows = op.film[idx]
    off = 32 if mut == "film_plus32" else C
    return rows[:, :C], rows[:, off:off + C]


# ------------------------------------------------------------------------------------------------ references
def act64(v, act):
    if act == ACT_SILU:
        return v / (1.0 + torch.exp(-v))
    return torch.clamp(v, min=0.0) if act == ACT_RELU else v


def value64(op):
    """act(((x - mean) * rstd * gamma + beta) * (scale + 1) + shift) in fp64, [B, C, h, w]."""
    B, C = op.x.shape[:2]
    x = op.x.double().reshape(B, op.G, -1)
    mean = x.mean(-1, keepdim=True)
    var = ((x * x).sum(-1, keepdim=True) / x.shape[-1] - mean * mean).clamp(min=0.0)       # biased, from the two sums
    y = ((x - mean) / torch.sqrt(var + EPS)).reshape(op.x.shape)
    y = y * op.gamma.double()[None, :, None, None] + op.beta.double()[None, :, None, None]
    fr = film_rows(op, B)
    if fr is not None:
        y = y * (fr[0].double()[:, :, None, None] + 1.0) + fr[1].double()[:, :, None, None]
    return act64(y, op.act)


def pool2(v):
    return torch.nn.functional.max_pool2d(v, 2)


def tail64(a, b=None, b_op=None, final_act=ACT_NONE, pool=False):
    """ld_gn_apply / the GN_TAIL epilogue in fp64: a normalised; ``b`` raw (stored tensor) or ``b_op`` normalised."""
    v = value64(a)
    if b is not None:
        v = v + b.double()
    if b_op is not None:
        v = v + value64(b_op)
    v = act64(v, final_act)
    return pool2(v) if pool else v


def coef32(op, fast=None, mut=None):
    """(a, s) [B, C] fp32 of y = x * a + s, in build_gn_coef's order.  ``fast``: None = PRECISE, else the five signs."""
    B, C = op.x.shape[:2]
    G, gs = op.G, C // op.G
    st = op.stats
    if mut == "stripe0":
        sums = st[:, 0]
    elif mut == "drop_last":
        sums = st[:, :STRIPES - 1].sum(1)
    else:
        sums = st.sum(1)
    s1, s2 = sums[..., 0], sums[..., 1]
    npix = op.npix * 4 if mut == "npix_full" else op.npix          # (the full map of a nearest-x2 source)
    n = float(npix * gs)
    if fast is None:
        inv_n = torch.tensor(1.0 / n, dtype=torch.float64)
    else:
        inv_n = nudge(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(n, dtype=torch.float32), fast[0]).double()
    mean = s1 * inv_n
    var = s2 * inv_n - mean * mean
    if mut == "unbiased":
        var = var * (n / max(n - 1.0, 1.0))
    if mut != "no_clamp":
        var = torch.where(var > 0.0, var, torch.zeros_like(var))
    ve = var + (0.0 if mut == "no_eps" else EPS)
    if fast is None:
        rstd = (1.0 / torch.sqrt(ve)).float()
    else:
        rstd = nudge((1.0 / torch.sqrt(ve.float().double())).float(), fast[1])
    mean32 = mean.float()
    Go = (16 if G == 8 else 8) if mut == "other_groups" else G
    gi = (torch.arange(C) // (C // Go)) % G
    gamma, beta = op.gamma, op.beta
    if mut == "gamma_wrap":                                          # channels >= 256 read the first trip's registers
        ci = torch.arange(C)
        ci = torch.where(ci >= 256, ci - 256, ci)
        gamma, beta = gamma[ci], beta[ci]
    a = rstd[:, gi] * gamma[None]
    s = beta[None] - mean32[:, gi] * a
    fr = film_rows(op, B, mut)
    if fr is not None:
        sc = fr[0] + 1.0
        a = a * sc
        s = s * sc + fr[1]
    return a, s


def act32(v, act, fast=None):
    if act == ACT_RELU:
        return torch.clamp(v, min=0.0)
    if act != ACT_SILU:
        return v
    if fast is None:
        return v / (1.0 + torch.exp(-v.double()).float())          # silu_f<true>: the fp64 exponential, rounded once
    p = nudge(torch.tensor(-1.4426950408889634, dtype=torch.float32) * v, fast[2])
    e = nudge(torch.exp2(p.double()).float(), fast[3])
    r = nudge((1.0 / (1.0 + e).double()).float(), fast[4])
    return v * r


def value32(op, fast=None, mut=None, coef=None):
    a, s = coef32(op, fast, mut) if coef is None else coef
    v = (op.x.double() * a.double()[:, :, None, None] + s.double()[:, :, None, None]).float()
    return act32(v, op.act, fast)


def tail32(a, b=None, b_op=None, final_act=ACT_NONE, pool=False, fast=None, mut=None):
    """The fp32 value BEFORE storage rounding (finish_pixel + the pool's fmaxf)."""
    v = value32(a, fast, mut)
    if b is not None:
        v = v + b
    if b_op is not None:
        coef = coef32(a, fast, mut) if mut == "b_with_a_coef" else None
        v = v + value32(b_op, fast, mut, coef=coef)
    v = act32(v, final_act, fast)
    if pool:
        if mut == "pool3":
            v = torch.stack([v[:, :, 0::2, 0::2], v[:, :, 0::2, 1::2], v[:, :, 1::2, 0::2]]).amax(0)
        else:
            v = pool2(v)
    return v


# ------------------------------------------------------------------------------------------------ the comparison
def floor_log2(v):
    """floor(log2 |v|) of an fp64 tensor (0 -> -1075)."""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.full_like(e, -1075), e - 1)


def ulp32(v):
    return torch.ldexp(torch.ones_like(v), (floor_log2(v) - 23).clamp(min=-149))


def half_spacing(v, dtype):
    """Half the distance between neighbouring ``dtype`` values at |v|."""
    e = floor_log2(v).clamp(min=EMIN[dtype])
    return torch.ldexp(torch.ones_like(v), e - MANT[dtype] - 1)


def group_max(v, gid, NG):
    """[B, C, ...] -> [B, NG]: max over each channel group's elements."""
    B, C = v.shape[:2]
    flat = v.reshape(B, C, -1).amax(-1)
    out = torch.zeros(B, NG, dtype=v.dtype)
    return out.scatter_reduce(1, gid[None].expand(B, C), flat, "amax", include_self=True)


def distance(pre32, ref64, gid, NG):
    """d or d_fast of one evaluation: per (sample, group) max |pre32 - ref64| (NaN counts as inf)."""
    diff = (pre32.double() - ref64).abs()
    return group_max(torch.nan_to_num(diff, nan=float("inf")), gid, NG)


def compare(got, ref64, d, d_fast, dtype, gid):
    """The rule of the GPU tests.  got: what storage holds, widened to fp32, NCHW; gid [C]: the (sample-independent)
    group of every output channel; d, d_fast [B, NG].  Per (sample, group), with m = max |ref64| of the group:

      fp32 storage:   max |got - ref64| <= max(4 d, ulp32(m))
      16-bit storage: |got_i - ref64_i| <= h_i + max(4 d, 4 d_fast, ulp32(m)), h_i = half the storage spacing at
                      |ref64_i| -- taken at |ref64_i| + the allowance, so that a value the allowance carries over a
                      binade edge gets the wider neighbour's spacing.

    -> (ok [B, NG] bool, worst [B, NG] = the largest |got - ref64| - h_i, allow [B, NG])."""
    NG = d.shape[1]
    m = group_max(ref64.abs(), gid, NG)
    allow = torch.maximum(4.0 * d, ulp32(m))
    if dtype != "fp32":
        allow = torch.maximum(allow, 4.0 * d_fast)
    err = (got.double() - ref64).abs()
    err = torch.nan_to_num(err, nan=float("inf"))
    if dtype != "fp32":
        al = allow[:, gid].reshape(allow.shape[0], -1, *([1] * (ref64.dim() - 2)))
        err = err - half_spacing(ref64.abs() + al, dtype)
    worst = group_max(err, gid, NG)
    return worst <= allow, worst, allow


def evaluate(fn, ref64, gid, NG, act_used):
    """(pre32, d, d_fast) of ``fn(fast)``: the restatement and the largest distance over the sign combinations (the three
    SiLU signs only where a SiLU is evaluated)."""
    pre = fn(None)
    d = distance(pre, ref64, gid, NG)
    d_fast = torch.zeros_like(d)
    signs = SIGNS if act_used else [s for s in SIGNS if s[2:] == (1, 1, 1)]
    for sg in signs:
        d_fast = torch.maximum(d_fast, distance(fn(sg), ref64, gid, NG))
    return pre, d, d_fast


# ------------------------------------------------------------------------------------------------ host-side routing
def gn_lead(C, dtype, pool, film_kind, b_norm, lead_args=1):
    """The predicate of gn_apply.hip's run<T>() for the preloaded-argument kernel (C < 1024, groups < 64 and the pixel
    count hold for every case here)."""
    return bool(lead_args) and not pool and film_kind not in ("batch", "table") and not b_norm and 256 % (C // ELEMS[dtype]) == 0


def gn_fragment_loop(C, dtype):
    return 256 % (C // ELEMS[dtype]) != 0


def gn_second_trip(C):
    """build_gn_coef's `for (c = tid; c < C; c += 256)` runs twice for a thread."""
    return C > 256


def gn_branches(C, dtype, H, W, pool, fpb=512):
    """Branches of gn_apply_tile a launch reaches: 'frag' (fragment loop), else of the register path 'pair' (the
    prefetched pair), 'reload' (a later trip of the pair loop), 'single' (one prefetched pixel, no pool), 'tail' (one()
    behind the loop)."""
    E = ELEMS[dtype]
    fpp = C // E
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    npix = Ho * Wo
    if 256 % fpp:
        return {"frag"}
    blocks = max(1, min(2048, (npix * fpp + fpb - 1) // fpb))
    ppb = 256 // fpp
    step = blocks * ppb
    out = set()
    for o in range(min(step, npix)):
        cnt = (npix - o + step - 1) // step
        if cnt >= 2:
            out.add("pair")
        if cnt >= 4:
            out.add("reload")
        if cnt % 2:
            out.add("single" if cnt == 1 and not pool else "tail")
    return out


def gn_instance(has_b, pool):
    return f"generic<{'b' if has_b else '-'},{'pool' if pool else '-'}>"


GN_BRANCHES = {"lead<b>", "lead<->", "generic<b,pool>", "generic<b,->", "generic<-,pool>", "generic<-,->", "pair", "reload",
               "single", "tail", "frag", "trip2-frag", "trip2-reg"}


def gn_reached(dtype, lead_args=1):
    """What GN_CASES reaches in ``dtype`` according to the mirrors above: the lead kernel with and without b, the four
    generic instantiations, the register path's branches, the fragment loop, the second coefficient trip on either path."""
    seen = set()
    for c in GN_CASES:
        if gn_lead(c.C, dtype, c.pool, c.film, c.mode == "basic", lead_args):
            seen.add("lead<b>" if c.mode != "a" else "lead<->")
        else:
            seen.add(gn_instance(c.mode != "a", c.pool))
        br = gn_branches(c.C, dtype, c.H, c.W, c.pool, c.fpb)
        seen |= br
        if gn_second_trip(c.C):
            seen.add("trip2-frag" if "frag" in br else "trip2-reg")
    return seen


# ------------------------------------------------------------------------------------------------ ld_gn_apply cases
def _gn(C, G, H, W, mode="a", film=None, pool=False, fpb=512, layout="spread", B=3):
    return NS(C=C, G=G, H=H, W=W, mode=mode, film=film, pool=pool, fpb=fpb, layout=layout, B=B,
              id=f"{C}g{G}-{H}x{W}-{mode}-{film or 'nofilm'}{'-pool' if pool else ''}{'-last' if layout == 'last' else ''}")


# mode: 'a' (a alone, SiLU), 'res' (ResnetBlock tail: a GN + SiLU, b raw), 'basic' (BasicBlock tail: both normalised, ReLU)
GN_CASES = [
    _gn(32, 8, 1, 1, "a"),                                     # npix_out = 1: the single prefetched pixel, clamped pair
    _gn(32, 16, 3, 5, "res", "shared", layout="last"),
    _gn(32, 16, 12, 10, "basic"),
    _gn(64, 8, 12, 10, "res"),                                 # the sampler's launch: lead kernel
    _gn(64, 8, 3, 5, "a", "table"),
    _gn(64, 16, 12, 10, "basic", layout="last"),
    _gn(64, 16, 1, 1, "res", "batch"),
    _gn(96, 8, 3, 5, "a", "batch"),                            # 256 % (C / E) != 0: the fragment loop
    _gn(96, 8, 12, 10, "res", "shared", layout="last"),
    _gn(128, 8, 3, 5, "res", "table"),
    _gn(128, 8, 12, 10, "a", "shared"),
    _gn(256, 8, 1, 1, "a", "shared"),
    _gn(256, 8, 3, 5, "basic", "batch"),
    _gn(320, 16, 3, 5, "res", "batch", layout="last"),         # fragment loop AND the second coefficient trip
    _gn(320, 16, 1, 1, "a"),
    _gn(512, 16, 3, 5, "a", "table"),                          # second coefficient trip on the register path
    _gn(512, 16, 1, 1, "res", "shared"),
    _gn(32, 8, 37, 29, "res", "shared", fpb=2048),             # several trips of the pair loop, ragged last one
    _gn(64, 8, 37, 29, "a", fpb=2048, layout="last"),
    _gn(96, 8, 37, 29, "basic", fpb=2048),
    _gn(32, 8, 2, 2, "basic", pool=True),                      # pooled: npix_out = 1
    _gn(64, 16, 4, 6, "a", "batch", pool=True),
    _gn(96, 8, 12, 10, "basic", "shared", pool=True),
    _gn(64, 16, 12, 10, "res", "table", pool=True, layout="last"),
    _gn(32, 16, 38, 30, "basic", pool=True, fpb=2048),
    _gn(320, 16, 4, 6, "a", pool=True),
]
T_VALUES = (0, 3)                                              # what t_ptr holds in table mode


def _key(site, case_id):
    """First of the ten generator streams of one case."""
    return int(rng.fnv1a64(site + ":" + case_id) % (1 << 40)) * 10


@functools.lru_cache(maxsize=None)
def gn_case(idx, dtype, t=0):
    """Inputs, ref64, restatement and allowances of GN_CASES[idx]."""
    c = GN_CASES[idx]
    key = _key("gn", c.id)
    x = make_x(c.B, c.C, c.H, c.W, c.G, dtype, key)
    gamma, beta, rows = make_params(c.C, key + 1, c.film, c.B)
    a = operand(x, c.G, gamma, beta, act=ACT_NONE if c.mode == "basic" else ACT_SILU, film=rows, film_kind=c.film, t=t,
                layout=c.layout)
    b = b_op = None
    final = ACT_NONE
    if c.mode == "res":
        b = stored(uni((c.B, c.C, c.H, c.W), key + 5, -2.0, 2.0), dtype)
    elif c.mode == "basic":
        xb = stored(uni((c.B, c.C, c.H, c.W), key + 6, -1.0, 3.0), dtype)
        gb, bb, _ = make_params(c.C, key + 7, None, c.B)
        b_op = operand(xb, c.G, gb, bb, layout=c.layout)
        final = ACT_RELU
    kw = dict(b=b, b_op=b_op, final_act=final, pool=c.pool)
    ref = tail64(a, **kw)
    gid = torch.arange(c.C) // (c.C // c.G)
    pre, d, d_fast = evaluate(lambda f: tail32(a, fast=f, **kw), ref, gid, c.G, a.act == ACT_SILU)
    return NS(c=c, a=a, kw=kw, ref=ref, pre=pre, d=d, d_fast=d_fast, gid=gid, NG=c.G)


# ------------------------------------------------------------------------------------------------ one-hot convolutions
def onehot_map(cin, cout):
    """Output channel o reads input channel (7 o + 3) mod cin at tap o mod 9 (tap = 3 ky + kx)."""
    o = torch.arange(cout)
    return (7 * o + 3) % cin, o % 9


def onehot_weight(cin, cout):
    w = torch.zeros(cout, cin, 3, 3)
    ci, tap = onehot_map(cin, cout)
    w[torch.arange(cout), ci, tap // 3, tap % 3] = 1.0
    return w


def onehot_gather(p, cout, pad=None):
    """The 3x3 'same' convolution with onehot_weight as a gather of p [B, cin, H, W]: out[b, o, y, x] =
    p[b, ci, y + ky - 1, x + kx - 1], ``pad`` [B, cin] (default 0) outside the map.  -> (out, inside mask [cout, H, W])."""
    B, cin, H, W = p.shape
    ci, tap = onehot_map(cin, cout)
    big = torch.zeros(B, cin, H + 2, W + 2, dtype=p.dtype)
    if pad is not None:
        big[:] = pad.to(p.dtype)[:, :, None, None]
    big[:, :, 1:H + 1, 1:W + 1] = p
    ins = torch.zeros(cin, H + 2, W + 2, dtype=torch.bool)
    ins[:, 1:H + 1, 1:W + 1] = True
    out = torch.empty(B, cout, H, W, dtype=p.dtype)
    inside = torch.empty(cout, H, W, dtype=torch.bool)
    for o in range(cout):
        ky, kx = int(tap[o]) // 3, int(tap[o]) % 3
        out[:, o] = big[:, ci[o], ky:ky + H, kx:kx + W]
        inside[o] = ins[ci[o], ky:ky + H, kx:kx + W]
    return out, inside


def _cv(cin, cout, H, W, B=2, act=ACT_SILU, G=8, film=None, route="generic", src="one", layout="spread"):
    return NS(cin=cin, cout=cout, H=H, W=W, B=B, act=act, G=G, film=film, route=route, src=src, layout=layout,
              id=f"{route}-{src}-{cin}to{cout}-{H}x{W}-g{G}-{'silu' if act == ACT_SILU else 'relu'}-{film or 'nofilm'}")


# the shapes of tests/exact_probes.py for these routes (equality asserted in tests/test_norm_ref.py)
BIG64_SHAPE = (2, 64, 128, 40, 24)
CONV3_SK_SHAPES = [(1, 96, 32, 13, 18), (2, 256, 64, 16, 16)]
C32_SHAPE = (2, 32, 32, 32, 32)
# src: 'one' | 'ups' (normalised source at half resolution) | 'gn+raw' / 'raw+gn' (two sources, cin split in halves) |
#      'slice' (the normalised source is the first cin channels of a tensor twice as wide)
CONV_CASES = [
    _cv(32, 32, 5, 7, film="shared"),
    _cv(64, 64, 5, 7, act=ACT_RELU, G=16, layout="last"),
    _cv(128, 32, 16, 16, film="batch"),
    _cv(256, 64, 16, 16, G=16, film="table"),
    _cv(64, 32, 17, 23, film="table"),
    _cv(256, 32, 5, 7, act=ACT_RELU),
    _cv(128, 64, 17, 23, G=16, film="shared", layout="last"),
    _cv(32, 64, 16, 16, act=ACT_RELU, film="batch"),
    _cv(64, 32, 16, 16, src="ups", film="shared"),
    _cv(64, 32, 17, 23, src="gn+raw", film="batch"),
    _cv(64, 64, 5, 7, src="raw+gn", G=16, film="table"),
    _cv(32, 32, 17, 23, src="slice", film="shared"),
    _cv(BIG64_SHAPE[1], BIG64_SHAPE[2], BIG64_SHAPE[3], BIG64_SHAPE[4], B=BIG64_SHAPE[0], route="big64", film="batch"),
    _cv(96, 32, 13, 18, B=1, route="sk", film="shared"),
    _cv(256, 64, 16, 16, B=2, route="sk", G=16, film="batch", layout="last"),
    # the general (GroupNorm-prologue) instantiations of the 32-channel x 16-row tile <2,4> ("big32") and of the 64-channel x
    # 8-row tile <4,2> ("rows8x64"), which no default threshold reaches at these sizes: ragged maps with H >= 16
    _cv(64, 32, 17, 23, route="big32", src="gn+raw", film="shared"),
    _cv(64, 96, 18, 22, route="big32", src="ups", film="table"),
    _cv(32, 32, 20, 28, route="big32", film="batch", layout="last"),
    _cv(64, 64, 17, 23, route="rows8x64", src="raw+gn", film="batch"),
    _cv(128, 64, 20, 28, B=1, route="rows8x64", src="ups", G=16, film="shared", layout="last"),
    _cv(32, 32, 32, 32, B=2, route="c32", film="shared"),
    _cv(32, 32, 48, 32, route="s32", film=None),
    _cv(32, 32, 48, 32, route="s32", film="shared", layout="last"),
    _cv(32, 32, 48, 32, route="s32", film="batch"),
]


def conv_route_dtypes(c):
    """Split-K halves, the persistent and the lean kernel exist for 16-bit storage only."""
    return LOWP if c.route in ("sk", "c32", "s32") else DTYPES


@functools.lru_cache(maxsize=None)
def conv_case(idx, dtype, t=0):
    """conv3x3 with the one-hot weight over act(GN(x) * (scale + 1) + shift): the output is the STORED prologue value
    of one shifted pixel, or 0 on padding.  ref64 / pre are those gathers; the groups of the comparison are the source
    groups (one more, with d = 0, for the channels of a raw source)."""
    c = CONV_CASES[idx]
    key = _key("cv", c.id)
    two = c.src in ("gn+raw", "raw+gn")
    cn = c.cin // 2 if two else c.cin                  # channels of the normalised source
    h, w = (c.H // 2, c.W // 2) if c.src == "ups" else (c.H, c.W)
    x = make_x(c.B, cn, h, w, c.G, dtype, key)
    gamma, beta, rows = make_params(cn, key + 1, c.film, c.B)
    a = operand(x, c.G, gamma, beta, act=c.act, film=rows, film_kind=c.film, t=t, layout=c.layout)
    raw = stored(uni((c.B, c.cin - cn, c.H, c.W), key + 5, -2.0, 2.0), dtype) if two else None
    up = (lambda v: v.repeat_interleave(2, 2).repeat_interleave(2, 3)) if c.src == "ups" else (lambda v: v)
    NG = c.G + 1

    def full(v, raw_v):
        v = up(v)
        if not two:
            return v
        return torch.cat([v, raw_v], 1) if c.src == "gn+raw" else torch.cat([raw_v, v], 1)

    gin = torch.arange(cn) // (cn // c.G)                                   # group of every INPUT channel
    graw = torch.full((c.cin - cn,), c.G)
    gin = gin if not two else (torch.cat([gin, graw]) if c.src == "gn+raw" else torch.cat([graw, gin]))
    ci, _ = onehot_map(c.cin, c.cout)
    gid = gin[ci]
    ref, inside = onehot_gather(full(value64(a), None if raw is None else raw.double()), c.cout)

    def pre_fn(fast):                                                       # the prologue's fp32 value, gathered
        return onehot_gather(full(value32(a, fast), raw), c.cout)[0]
    pre, d, d_fast = evaluate(pre_fn, ref, gid, NG, c.act == ACT_SILU)
    return NS(c=c, a=a, raw=raw, cn=cn, ref=ref, pre=pre, d=d, d_fast=d_fast, gid=gid, NG=NG, inside=inside, full=full, gin=gin)


# ------------------------------------------------------------------------------------------------ GN_TAIL epilogue cases
def _tl(cout, H, W, residual, layout="spread", B=2):
    return NS(cout=cout, H=H, W=W, residual=residual, layout=layout, B=B, G=8, id=f"{cout}-{H}x{W}-{'res' if residual else 'nores'}")


TAIL_CASES = [_tl(32, 3, 5, False), _tl(32, 16, 16, True, "last"), _tl(64, 9, 11, True), _tl(64, 3, 5, False, "last"),
              _tl(128, 16, 16, False), _tl(128, 9, 11, True, "last"), _tl(256, 3, 5, True), _tl(256, 9, 11, False)]
TAIL_CIN = 32                                    # input channels of the (all-zero) 1x1 weight


@functools.lru_cache(maxsize=None)
def tail_case(idx, dtype):
    """ld_conv1x1 + LD_EPI_GN_TAIL with zero weights and bias: out = 0 + SiLU(GN(tail)) (+ a residual of small integers)."""
    c = TAIL_CASES[idx]
    key = _key("tl", c.id)
    x = make_x(c.B, c.cout, c.H, c.W, c.G, dtype, key)
    gamma, beta, _ = make_params(c.cout, key + 1, None, c.B)
    a = operand(x, c.G, gamma, beta, act=ACT_SILU, layout=c.layout)
    res = None
    if c.residual:
        res = torch.from_numpy(np.rint(rng.uniform((c.B, c.cout, c.H, c.W), SEED, key + 5, -4.5, 4.5)).astype(np.float32))
    ref = tail64(a, b=res)
    gid = torch.arange(c.cout) // (c.cout // c.G)
    pre, d, d_fast = evaluate(lambda f: tail32(a, b=res, fast=f), ref, gid, c.G, True)
    return NS(c=c, a=a, res=res, ref=ref, pre=pre, d=d, d_fast=d_fast, gid=gid, NG=c.G)
