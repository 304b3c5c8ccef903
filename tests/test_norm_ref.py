"""tests/norm_ref.py proved without a GPU: its fp64 forms are pinned to oracle/unet_ref.py, every case of
tests/test_hip_norm.py meets the preconditions the comparison relies on, and the comparison rejects a set of subtly
wrong kernels in every (sample, group) they touch."""
import pytest
import torch
import torch.nn.functional as F

import exact_probes
import norm_ref as R
from oracle import unet_ref

GN_IDS = [c.id for c in R.GN_CASES]
CONV_IDS = [c.id for c in R.CONV_CASES]
TAIL_IDS = [c.id for c in R.TAIL_CASES]


def as_stored(pre, dtype):
    return pre if dtype == "fp32" else R.stored(pre, dtype)


def cases(site):
    n = {"gn": len(R.GN_CASES), "conv": len(R.CONV_CASES), "tail": len(R.TAIL_CASES)}[site]
    for i in range(n):
        c = getattr(R, {"gn": "GN_CASES", "conv": "CONV_CASES", "tail": "TAIL_CASES"}[site])[i]
        for dt in (R.conv_route_dtypes(c) if site == "conv" else R.DTYPES):
            yield i, c, dt, getattr(R, site + "_case")(i, dt)


# ------------------------------------------------------------------------------------------------ pins to the oracle
def identity_conv(C):
    w = torch.zeros(C, C, 3, 3, dtype=torch.float64)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    return w


def op64(x, G, gamma, beta, act, film=None, kind=None):
    return R.operand(x, G, gamma, beta, act=act, film=film, film_kind=kind)


@pytest.mark.parametrize("with_time", [False, True])
def test_resnet_block_tail_is_the_oracles(with_time):
    """oracle resnet_block with identity convolutions = SiLU(GN2(SiLU(GN1(x) * (scale + 1) + shift))) + x, in fp64:
    the FiLM form of value64 (per-sample rows) feeding the ResnetBlock tail of tail64."""
    B, C, H, W, G = 3, 32, 6, 5, 8
    x = R.make_x(B, C, H, W, G, "fp32", 11)
    g1, b1, _ = R.make_params(C, 12, None, B)
    g2, b2, _ = R.make_params(C, 14, None, B)
    sd = {"r.block1.proj.weight": identity_conv(C), "r.block1.proj.bias": torch.zeros(C, dtype=torch.float64),
          "r.block2.proj.weight": identity_conv(C), "r.block2.proj.bias": torch.zeros(C, dtype=torch.float64),
          "r.block1.norm.weight": g1.double(), "r.block1.norm.bias": b1.double(),
          "r.block2.norm.weight": g2.double(), "r.block2.norm.bias": b2.double()}
    temb, film = None, None
    if with_time:
        temb = R.uni((B, 16), 16).double()
        sd["r.mlp.1.weight"], sd["r.mlp.1.bias"] = R.uni((2 * C, 16), 17).double(), R.uni((2 * C,), 18, -0.3, 0.3).double()
        film = F.linear(F.silu(temb), sd["r.mlp.1.weight"], sd["r.mlp.1.bias"])
    want = unet_ref.resnet_block(sd, "r", x.double(), temb, groups=G)
    h = R.value64(op64(x.double(), G, g1.double(), b1.double(), R.ACT_SILU, film, "batch" if with_time else None))
    got = R.tail64(op64(h, G, g2.double(), b2.double(), R.ACT_SILU), b=x)
    assert float((got - want).abs().max()) <= 1e-12


def test_basic_block_tail_with_pool_is_the_oracles():
    """oracle basic_block with identity convolutions, then max_pool2d: ReLU(GN(ReLU(GN(x))) + GN_id(x)), pooled."""
    B, C, H, W, G = 3, 32, 6, 8, 16
    x = R.make_x(B, C, H, W, G, "fp32", 21)
    p = [R.make_params(C, 22 + 2 * i, None, B) for i in range(3)]
    sd = {}
    for name, (g, b, _) in zip(("convblock.1", "convblock.4", "identity.1"), p):
        sd["e." + name + ".weight"], sd["e." + name + ".bias"] = g.double(), b.double()
    for name in ("convblock.0", "convblock.3", "identity.0"):
        sd["e." + name + ".weight"], sd["e." + name + ".bias"] = identity_conv(C), torch.zeros(C, dtype=torch.float64)
    want = F.max_pool2d(unet_ref.basic_block(sd, "e", x.double(), groups=G), 2)
    h = R.value64(op64(x.double(), G, p[0][0].double(), p[0][1].double(), R.ACT_RELU))
    got = R.tail64(op64(h, G, p[1][0].double(), p[1][1].double(), R.ACT_NONE),
                   b_op=op64(x.double(), G, p[2][0].double(), p[2][1].double(), R.ACT_NONE), final_act=R.ACT_RELU, pool=True)
    assert float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("act", [R.ACT_SILU, R.ACT_RELU])
def test_prologue_then_onehot_conv_is_the_oracles(act):
    """conv(act(GN(x) * (scale + 1) + shift)): the oracle's Block with an identity convolution (SiLU) / F.group_norm +
    relu gives the prologue, F.conv2d with the one-hot weight the convolution; norm_ref gathers value64."""
    B, C, cout, H, W, G = 2, 32, 64, 5, 7, 8
    x = R.make_x(B, C, H, W, G, "fp32", 31).double()
    g, b, rows = R.make_params(C, 32, "batch", B)
    if act == R.ACT_SILU:
        sd = {"b.proj.weight": identity_conv(C), "b.proj.bias": torch.zeros(C, dtype=torch.float64),
              "b.norm.weight": g.double(), "b.norm.bias": b.double()}
        film = (rows[:, :C, None, None].double(), rows[:, C:, None, None].double())
        y = unet_ref.conv_gn_act(sd, "b", x, G, film)
        a = op64(x, G, g.double(), b.double(), act, rows.double(), "batch")
    else:
        y = F.relu(F.group_norm(x, G, g.double(), b.double(), eps=1e-5))
        a = op64(x, G, g.double(), b.double(), act)
    want = F.conv2d(y, R.onehot_weight(C, cout).double(), padding=1)
    got, _ = R.onehot_gather(R.value64(a), cout)
    assert float((got - want).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ preconditions
def test_shapes_shared_with_the_exact_probes():
    assert R.BIG64_SHAPE == exact_probes.BIG64_SHAPE and R.CONV3_SK_SHAPES == exact_probes.CONV3_SK_SHAPES
    assert R.C32_SHAPE == exact_probes.C32_SHAPE and R.STRIPES == 16
    sk = [(c.B, c.cin, c.cout, c.H, c.W) for c in R.CONV_CASES if c.route == "sk"]
    assert sk == R.CONV3_SK_SHAPES


@pytest.mark.parametrize("idx", range(len(R.CONV_CASES)), ids=CONV_IDS)
def test_onehot_convolution_equals_the_gather_bit_for_bit(idx):
    """F.conv2d with the one-hot weight, in fp32 and in fp64, of the STORED prologue values = the gather (every other
    product is 0 * finite), and 0 exactly where the tap falls on padding."""
    c = R.CONV_CASES[idx]
    for dt in R.conv_route_dtypes(c):
        k = R.conv_case(idx, dt)
        p = as_stored(k.full(R.value32(k.a), k.raw), dt)
        assert bool(torch.isfinite(p).all())
        want, inside = R.onehot_gather(p, c.cout)
        w = R.onehot_weight(c.cin, c.cout)
        assert torch.equal(F.conv2d(p, w, padding=1), want)
        assert torch.equal(F.conv2d(p.double(), w.double(), padding=1), want.double())
        assert bool((want[:, ~inside] == 0).all()) and int((~inside).sum()) > 0
        assert torch.equal(want, as_stored(k.pre, dt))


def _planted(a, B, dtype, has_film):
    C, G = a.x.shape[1], a.G
    x = a.x.double().reshape(B, G, -1)
    mean, std = x.mean(-1), x.var(-1, unbiased=False).sqrt()
    assert torch.equal(R.stored(a.x, dtype), a.x)                              # the inputs ARE stored values
    mu, sigma = R.planted_moments(B, G)
    for dim in (0, 1):                                                          # the plan: neighbours apart
        lo, hi = (mu[:-1], mu[1:]) if dim == 0 else (mu[:, :-1], mu[:, 1:])
        assert bool(((hi - lo).abs() >= 0.5).all())
        lo, hi = (sigma[:-1], sigma[1:]) if dim == 0 else (sigma[:, :-1], sigma[:, 1:])
        assert bool((torch.maximum(lo, hi) >= 1.5 * torch.minimum(lo, hi)).all())
    cb, hb = R.const_group(B, G), R.high_group(B, G)
    assert cb != hb
    assert float(std[cb]) == 0.0 and float(mean[cb]) == R.CONST_VALUE         # constant after rounding: the clamp's group
    n = x.shape[-1]
    if n >= 16:                                                                 # (a handful of draws has no stable ratio)
        assert 20.0 <= float(mean[hb].abs() / std[hb]) <= 45.0, float(mean[hb].abs() / std[hb])
        others = torch.ones(B, G, dtype=torch.bool)
        others[hb] = others[cb] = False
        assert float((mean.abs() / std)[others].max()) < 20.0                  # ... in one sample only
    assert float(a.gamma[R.CH_GAMMA0]) == 0.0 and int((a.gamma == 0).sum()) == 1
    assert len(set(a.gamma.tolist())) == C and len(set(a.beta.tolist())) == C
    if has_film:
        f = a.film
        assert bool((f[:, R.CH_SCALE] == -1.0).all()) and bool((f[:, C + R.CH_NEG] == -90.0).all()) and bool((f[:, C + R.CH_POS] == 90.0).all())
        free = [i for i in range(2 * C) if i not in (R.CH_SCALE, C + R.CH_NEG, C + R.CH_POS)]
        assert len(set(f[0, free].tolist())) == len(free)                      # distinct per channel
        for i in range(f.shape[0]):
            for j in range(i + 1, f.shape[0]):
                assert int((f[i, free] != f[j, free]).sum()) == len(free)      # distinct per batch / timestep row
        a_, s_ = R.coef32(a)
        assert bool((a_[:, R.CH_SCALE] == 0).all())                            # scale = -1: a = 0 exactly
    # stripes: unequal shares everywhere, or everything in the last stripe
    st = a.stats
    if float(st[:, 0].abs().max()) == 0.0:
        assert float(st[:, :R.STRIPES - 1].abs().max()) == 0.0 and float(st[:, R.STRIPES - 1, :, 1].min()) > 0.0
    else:
        s2 = st[..., 1]
        assert bool((s2[:, 1:] > s2[:, :-1]).all())
    assert float((st.sum(1) - R.group_sums(a.x, G)).abs().max()) <= 1e-12 * float(R.group_sums(a.x, G).abs().max())


def _bounds_hold(k, dtype):
    assert bool(torch.isfinite(k.d).all()) and bool(torch.isfinite(k.d_fast).all()) and bool(torch.isfinite(k.ref).all())
    ok, worst, allow = R.compare(k.pre, k.ref, k.d, k.d_fast, "fp32", k.gid)   # the restatement inside its own bound
    assert bool(ok.all()), (worst - allow).max()
    for dt in R.DTYPES:                                                         # ... and, rounded, inside the storage bounds
        ok, worst, allow = R.compare(as_stored(k.pre, dt), k.ref, k.d, k.d_fast, dt, k.gid)
        assert bool(ok.all()), (dt, float((worst - allow).max()))


@pytest.mark.parametrize("idx", range(len(R.GN_CASES)), ids=GN_IDS)
def test_gn_apply_cases_meet_the_preconditions(idx):
    c = R.GN_CASES[idx]
    for dt in R.DTYPES:
        for t in (R.T_VALUES if c.film == "table" else (0,)):
            k = R.gn_case(idx, dt, t)
            _planted(k.a, c.B, dt, c.film is not None)
            _bounds_hold(k, dt)
            assert k.ref.shape == (c.B, c.C, c.H // 2 if c.pool else c.H, c.W // 2 if c.pool else c.W)
    if c.film == "table":
        assert not torch.equal(R.gn_case(idx, "fp32", 0).ref, R.gn_case(idx, "fp32", 3).ref)


@pytest.mark.parametrize("idx", range(len(R.CONV_CASES)), ids=CONV_IDS)
def test_conv_cases_meet_the_preconditions(idx):
    c = R.CONV_CASES[idx]
    for dt in R.conv_route_dtypes(c):
        k = R.conv_case(idx, dt)
        _planted(k.a, c.B, dt, c.film is not None)
        _bounds_hold(k, dt)
        assert bool((k.d[:, c.G] == 0).all())                                  # raw channels: exact
        if c.src == "ups":
            assert k.a.npix * 4 == c.H * c.W


@pytest.mark.parametrize("idx", range(len(R.TAIL_CASES)), ids=TAIL_IDS)
def test_gn_tail_cases_meet_the_preconditions(idx):
    c = R.TAIL_CASES[idx]
    for dt in R.DTYPES:
        k = R.tail_case(idx, dt)
        _planted(k.a, c.B, dt, False)
        _bounds_hold(k, dt)
        if c.residual:
            assert bool((k.res == k.res.round()).all()) and float(k.res.abs().max()) == 4.0


def test_case_lists_reach_every_branch():
    """The routing mirrors say that GN_CASES reaches every kernel and branch of GN_BRANCHES in every storage type (and,
    with lead_args = 0, the generic kernels instead of the lead kernel)."""
    for dt in R.DTYPES:
        assert R.GN_BRANCHES <= R.gn_reached(dt), (dt, R.GN_BRANCHES - R.gn_reached(dt))
        assert not {"lead<b>", "lead<->"} & R.gn_reached(dt, lead_args=0)
    assert R.gn_fragment_loop(96, "bf16") and R.gn_fragment_loop(320, "fp32") and not R.gn_fragment_loop(512, "fp32")
    for dt in R.DTYPES:                                                         # the one shape of test_hip_ops.py
        assert R.gn_branches(64, dt, 12, 10, False) <= {"pair", "single"}


# ------------------------------------------------------------------------------------------------ mutations
def _all(k):
    return torch.ones(k.d.shape, dtype=torch.bool)


def _not_const(k, B, G):
    m = _all(k)
    m[R.const_group(B, G)] = False
    return m


def _only_const(k, B, G):
    m = ~_all(k)
    m[R.const_group(B, G)] = True
    return m


def _pre(site, k, mut, fast=None):
    """The restatement of one case with wrong kernel ``mut``."""
    if site == "gn":
        return R.tail32(k.a, fast=fast, mut=mut, **k.kw)
    if site == "tail":
        return R.tail32(k.a, b=k.res, fast=fast, mut=mut)
    return R.onehot_gather(k.full(R.value32(k.a, fast, mut), k.raw), k.c.cout)[0]


def _norm_groups(site, k, m):
    """Conv cases: the extra group of the raw channels is never touched; a source group counts only if some output
    channel reads it."""
    if site == "conv":
        m = m.clone()
        m[:, k.c.G] = False
        read = torch.zeros(k.NG, dtype=torch.bool)
        read[k.gid] = True
        m &= read[None]
    return m


def coef_mutants():
    """name -> (applies(site, c, dtype), touched(site, k) -> [B, NG]) for the wrong coefficient builds."""
    def n_of(site, c):
        cn = c.C if site == "gn" else (c.cout if site == "tail" else (c.cin // 2 if "+" in c.src else c.cin))
        npix = c.H * c.W // (4 if site == "conv" and c.src == "ups" else 1)
        return npix * (cn // c.G), cn

    def film_of(site, c):
        return None if site == "tail" else c.film

    def wrap_groups(site, k):
        c = k.c
        n, cn = n_of(site, c)
        gs = cn // c.G
        m = ~_all(k)
        for g in range(c.G):
            if (g + 1) * gs > 256:
                m[:, g] = True
        return m

    def other_groups(site, k):
        m = _all(k)
        if k.c.G == 16:                       # c / (C / 8) = g / 2: group 0 keeps its own statistics
            m[:, 0] = False
        return m

    def not_sample0(site, k):
        m = _all(k)
        m[0] = False
        return m

    return {
        # FiLM addressing
        "film_row0": (lambda s, c, dt: film_of(s, c) == "batch", not_sample0),
        "t_off": (lambda s, c, dt: film_of(s, c) == "table", lambda s, k: _all(k)),
        "film_plus32": (lambda s, c, dt: film_of(s, c) is not None and n_of(s, c)[1] != 32, lambda s, k: _all(k)),
        # group / stripe indexing
        "other_groups": (lambda s, c, dt: True, other_groups),
        "stripe0": (lambda s, c, dt: True, lambda s, k: _all(k)),
        "drop_last": (lambda s, c, dt: True, lambda s, k: _all(k)),
        # the variance.  Unbiased: rstd moves by 1 / (2 n) relative -- visible against half a storage spacing (2^-9 /
        # 2^-12 relative) only for small n; a constant group has var = 0 either way.
        "unbiased": (lambda s, c, dt: n_of(s, c)[0] <= {"fp32": 1024, "bf16": 16, "fp16": 128}[dt],
                     lambda s, k: _not_const(k, k.c.B, k.c.G)),
        # eps missing: 1 / sqrt(0) in the constant group (elsewhere eps / (2 var) relative, which only fp32 storage sees)
        "no_eps": (lambda s, c, dt: True, lambda s, k: _only_const(k, k.c.B, k.c.G)),
        "gamma_wrap": (lambda s, c, dt: n_of(s, c)[1] > 256, wrap_groups),
    }


def _fails(k, got, dtype):
    ok, _, _ = R.compare(got, k.ref, k.d, k.d_fast, dtype, k.gid)
    return ~ok


@pytest.mark.parametrize("site", ["gn", "conv", "tail"])
def test_wrong_coefficients_are_rejected(site):
    muts = coef_mutants()
    applied = {m: 0 for m in muts}
    for idx, c, dt, k in cases(site):
        for name, (applies, touched) in muts.items():
            if not applies(site, c, dt):
                continue
            t = _norm_groups(site, k, touched(site, k))
            if not bool(t.any()):
                continue
            bad = _fails(k, as_stored(_pre(site, k, name), dt), dt)
            assert bool(bad[t].all()), (name, c.id, dt, (t & ~bad).nonzero().tolist())
            applied[name] += 1
    must = set(muts) - ({"film_row0", "t_off", "film_plus32", "gamma_wrap"} if site == "tail" else set())
    if site == "conv":
        must -= {"gamma_wrap"}                # the widest normalised source has 256 channels: one trip of 256 threads
    assert all(applied[m] > 0 for m in must), applied


def test_unclamped_variance_is_rejected():
    """16-bit storage: with 1/n one ulp high the constant group's s2/n - mean^2 is about -CONST^2 * 2^-23, below -eps:
    without the clamp rstd is NaN.  (With PRECISE arithmetic the cancellation leaves ~1e-14: nothing to clamp that the
    result could show.)"""
    fast = (1, 1, 1, 1, 1)
    n = 0
    for site in ("gn", "conv", "tail"):
        for idx, c, dt, k in cases(site):
            if dt == "fp32":
                continue
            t = _norm_groups(site, k, _only_const(k, c.B, c.G))
            if not bool(t.any()):
                continue
            assert bool(torch.isfinite(_pre(site, k, None, fast)).all())
            bad = _fails(k, as_stored(_pre(site, k, "no_clamp", fast), dt), dt)
            assert bool(bad[t].all()), (c.id, dt)
            n += 1
    assert n > 50


def test_second_operand_with_the_first_operands_coefficients_is_rejected():
    n = 0
    for idx, c, dt, k in cases("gn"):
        if c.mode == "basic":
            bad = _fails(k, as_stored(_pre("gn", k, "b_with_a_coef"), dt), dt)
            assert bool(bad.all()), (c.id, dt)
            n += 1
    assert n >= 15


def test_full_map_pixel_count_for_an_upsampled_source_is_rejected():
    n = 0
    for idx, c, dt, k in cases("conv"):
        if c.src == "ups":
            bad = _fails(k, as_stored(_pre("conv", k, "npix_full"), dt), dt)
            assert bool(bad[_norm_groups("conv", k, _all(k))].all()), (c.id, dt)
            n += 1
    assert n == 9                             # three upsampled cases (generic, big32, rows8x64) in three storage types


def test_padding_that_receives_the_activated_shift_is_rejected():
    """Padding = act(s) instead of 0: every source group some border tap reads with |act(s)| > 0.05."""
    n = 0
    for idx, c, dt, k in cases("conv"):
        a_, s_ = R.coef32(k.a)
        pad = as_stored(R.act32(s_, c.act), dt)                                 # [B, cn]
        padf = torch.zeros(c.B, c.cin)
        padf[:, k.gin < c.G] = pad
        got = R.onehot_gather(k.full(as_stored(R.value32(k.a), dt), k.raw), c.cout, pad=padf)[0]
        ci, tap = R.onehot_map(c.cin, c.cout)
        t = torch.zeros(c.B, k.NG, dtype=torch.bool)
        for o in range(c.cout):
            if int(tap[o]) != 4 and int(k.gid[o]) < c.G:
                t[:, k.gid[o]] |= padf[:, ci[o]].abs() > 0.05
        bad = _fails(k, got, dt)
        assert bool(bad[t].all()), (c.id, dt, (t & ~bad).nonzero().tolist())
        assert bool((got[:, ~k.inside] != 0).any())
        n += int(t.sum())
    assert n > 100


def test_pool_over_three_of_four_pixels_is_rejected():
    """Touched: the groups where the dropped pixel is some window's maximum by a clear margin (0.05 (1 + |v|))."""
    n = 0
    for idx, c, dt, k in cases("gn"):
        if not c.pool:
            continue
        kw = dict(k.kw, pool=False)
        v = R.tail32(k.a, **kw)
        v4, v3 = v[:, :, 1::2, 1::2], torch.stack([v[:, :, 0::2, 0::2], v[:, :, 0::2, 1::2], v[:, :, 1::2, 0::2]]).amax(0)
        t = R.group_max(((v4 - v3) > 0.05 * (1 + v4.abs())).float(), k.gid, k.NG) > 0
        bad = _fails(k, as_stored(_pre("gn", k, "pool3"), dt), dt)
        assert bool(bad[t].all()), (c.id, dt)
        n += int(t.sum())
    assert n > 100


@pytest.mark.parametrize("site", ["gn", "conv", "tail"])
def test_an_unwritten_last_pixel_is_rejected(site):
    for idx, c, dt, k in cases(site):
        got = as_stored(k.pre, dt).clone()
        got[:, :, -1, -1] = float("nan")                                        # the NaN fill shows through
        bad = _fails(k, got, dt)
        t = _all(k)
        if site == "conv":                                                      # groups some output channel belongs to
            t = torch.zeros(k.NG, dtype=torch.bool)
            t[k.gid] = True
            t = t[None].expand(c.B, k.NG)
        assert bool(bad[t].all()), (c.id, dt)


def test_pair_loops_second_pixel_equal_to_its_first_is_rejected():
    """Register path of gn_apply: the pair's second pixel (o + step) stores the first one's value.  A group whose output
    does not vary over the pixels (the constant group without a second operand) cannot show it."""
    n = 0
    for idx, c, dt, k in cases("gn"):
        if "pair" not in R.gn_branches(c.C, dt, c.H, c.W, c.pool, c.fpb):
            continue
        E = R.ELEMS[dt]
        fpp = c.C // E
        Ho, Wo = k.ref.shape[2:]
        npix = Ho * Wo
        step = max(1, min(2048, (npix * fpp + c.fpb - 1) // c.fpb)) * (256 // fpp)
        got = as_stored(k.pre, dt).clone().reshape(c.B, c.C, npix)
        hi = min(2 * step, npix)
        got[:, :, step:hi] = got[:, :, 0:hi - step].clone()
        t = _not_const(k, c.B, c.G) if c.mode == "a" else _all(k)
        bad = _fails(k, got.reshape(k.ref.shape), dt)
        assert bool(bad[t].all()), (c.id, dt, (t & ~bad).nonzero().tolist())
        n += 1
    assert n > 20


# ------------------------------------------------------------------------------------------------ report
def test_report_fast_path_allowance_of_the_high_mean_group(capsys):
    """Printed, not asserted (docs/findings.md, finding 137): d_fast / d of the |mean| / std ~ 30 group."""
    rows = []
    for site in ("gn", "conv", "tail"):
        for dt in R.DTYPES:
            r = []
            for idx, c, dt2, k in cases(site):
                if dt2 == dt and c.H * c.W * (k.a.x.shape[1] // c.G) >= 16:
                    hb = R.high_group(c.B, c.G)
                    if site != "conv" or bool((k.gid == hb[1]).any()):
                        r.append((float(k.d[hb]), float(k.d_fast[hb])))
            if r:
                d, df = max(x[0] for x in r), max(x[1] for x in r)
                ratio = sorted(x[1] / x[0] for x in r)
                rows.append(f"{site:5s} {dt}: high-mean group d <= {d:.2e}, d_fast <= {df:.2e}, d_fast / d median {ratio[len(ratio) // 2]:.0f} "
                            f"(min {ratio[0]:.0f}, max {ratio[-1]:.0f}) over {len(r)} cases")
    with capsys.disabled():
        print("\n" + "\n".join(rows))
