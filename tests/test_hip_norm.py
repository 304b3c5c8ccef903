"""Parity of the GroupNorm / FiLM path with its fp64 form (tests/norm_ref.py, proved on the CPU by
tests/test_norm_ref.py) at the five sites that share build_gn_coef / affine_act_n: ld_gn_apply (lead kernel and the four
generic instantiations), the prologue of the generic 3x3 kernel (every tile: 32 x 8 rows by default, 64 x 16, 32 x 16 and
64 x 8 rows forced and confirmed with ld_last_route; split-K halves), the
persistent and the lean 3x3 kernels, and the LD_EPI_GN_TAIL epilogue of ld_conv1x1.

The rule is norm_ref.compare, per (sample, group): fp32 storage within max(4 d, one fp32 ulp of the group's largest
value) of ref64; 16-bit storage element-wise within half a storage spacing plus max(4 d, 4 d_fast, that ulp), d and d_fast
being the CPU restatements' own distances from ref64.  The convolutions carry a one-hot weight, so their output is the
stored prologue value of one shifted pixel and EXACTLY 0 where the tap falls on padding.  Every output holds NaN before
the launch; routes are switched through ld_tuning_set (restored afterwards) and confirmed with the launch counters, or,
where no counter exists, with norm_ref's mirrors of the host-side predicates."""
import contextlib
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from localdiffusion_hallucination_amd import _cabi as cabi       # noqa: E402
from localdiffusion_hallucination_amd.tuning import kernel_table  # noqa: E402
import hip_helpers as hh                                           # noqa: E402
import norm_ref as R                                               # noqa: E402

COUNTERS = (cabi.COUNTER_CONV3X3_C32, cabi.COUNTER_CONV3X3_GENERIC, cabi.COUNTER_CONV3X3_S32)


@contextlib.contextmanager
def routed(**sets):
    """Entries of the library's routing table for the duration of the block (saved, restored in ``finally``)."""
    lib = cabi.lib()
    keep = kernel_table(lib)
    try:
        for k, v in sets.items():
            cabi.check(lib.ld_tuning_set(k.encode(), v), "tuning_set")
        yield lib
    finally:
        for k, v in keep.items():
            cabi.check(lib.ld_tuning_set(k.encode(), v), "tuning_set")


def counters():
    lib = cabi.lib()
    return {w: lib.ld_counter(w) for w in COUNTERS}


def launched(before):
    torch.cuda.synchronize()
    now = counters()
    return tuple(now[w] - before[w] for w in COUNTERS)          # (c32, generic, s32)


def dev(t, dtype=None):
    return None if t is None else t.to(hh.DEV, dtype if dtype is not None else t.dtype).contiguous()


def gn_src(a, dtype, x_dev=None, stride=0, ups=0):
    """norm_ref operand -> ld_src with its statistics, tables and FiLM addressing."""
    Cc = a.x.shape[1]
    film = dev(a.film)
    return hh.make_src(hh.nhwc(a.x, dtype) if x_dev is None else x_dev, Cc, stride=stride, ups=ups,
                       gn=(dev(a.stats), dev(a.gamma), dev(a.beta), a.G), act=a.act, film=film,
                       film_b=2 * Cc if a.film_kind == "batch" else 0, film_t=2 * Cc if a.film_kind == "table" else 0)


def t_tensor(kind, t):
    return torch.tensor([t], dtype=torch.int32, device=hh.DEV) if kind == "table" else None


def check(k, got, dtype, what):
    """norm_ref.compare; the figures of the (sample, group) nearest to its bound are printed before the assertion."""
    ok, worst, allow = R.compare(got, k.ref, k.d, k.d_fast, dtype, k.gid)
    i = int((worst / allow).argmax())
    b, g = divmod(i, k.NG)
    print(f"{what} {dtype}: (b {b}, g {g}) err {float(worst[b, g]):.3e} of {float(allow[b, g]):.3e} allowed, "
          f"d {float(k.d[b, g]):.3e} d_fast {float(k.d_fast[b, g]):.3e}")
    assert bool(ok.all()), (what, dtype, (~ok).nonzero().tolist()[:8], float(worst[b, g]), float(allow[b, g]))


# ------------------------------------------------------------------------------------------------ ld_gn_apply
def run_gn(k, dtype, t=0):
    c = k.c
    A = cabi.GnApplyArgs()
    keep = [gn_src(k.a, dtype)]                # (assigning an ld_src copies the struct, not the tensors it points to)
    A.a = keep[0]
    if k.kw["b"] is not None:
        keep.append(hh.make_src(hh.nhwc(k.kw["b"], dtype), c.C))
    elif k.kw["b_op"] is not None:
        keep.append(gn_src(k.kw["b_op"], dtype))
    if len(keep) > 1:
        A.b = keep[1]
    A.final_act, A.pool = k.kw["final_act"], int(c.pool)
    Ho, Wo = k.ref.shape[2:]
    out = hh.nans(c.B, Ho, Wo, c.C, dtype=hh.TDT[dtype])
    tp = t_tensor(c.film, t)
    A.out, A.B, A.H, A.W, A.dtype, A.t_ptr = out.data_ptr(), c.B, c.H, c.W, cabi.dtype_code(dtype), cabi.ptr(tp)
    cabi.check(cabi.lib().ld_gn_apply(C.byref(A), hh.st()), "gn_apply")
    torch.cuda.synchronize()
    del keep
    return hh.nchw(out)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("idx", range(len(R.GN_CASES)), ids=[c.id for c in R.GN_CASES])
def test_gn_apply(idx, dtype):
    """Every case against ref64; a case the lead kernel accepts also with lead_args = 0 (the generic kernel), and the two
    outputs are the same bits.  Table mode at both values of the step counter.

    (32g8-1x1-a-nofilm in fp32 is the case that missed the rule while silu_f<true> used libm's expf: finding 137.)"""
    c = R.GN_CASES[idx]
    for t in (R.T_VALUES if c.film == "table" else (0,)):
        k = R.gn_case(idx, dtype, t)
        with routed(gn_frags_per_block=c.fpb, lead_args=1):
            got = run_gn(k, dtype, t)
        check(k, got, dtype, f"gn_apply {c.id} t={t}")
        if R.gn_lead(c.C, dtype, c.pool, c.film, c.mode == "basic"):
            with routed(gn_frags_per_block=c.fpb, lead_args=0):
                got0 = run_gn(k, dtype, t)
            assert torch.equal(got, got0), (c.id, int((got != got0).sum()))


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_gn_apply_cases_reach_every_kernel_and_branch(dtype):
    """No launch counter exists for these routes: the mirrors of gn_apply.hip's host predicates and of gn_apply_tile's
    loop bounds say what test_gn_apply reaches."""
    assert kernel_table(cabi.lib())["lead_args"] == 1
    assert R.GN_BRANCHES <= R.gn_reached(dtype), R.GN_BRANCHES - R.gn_reached(dtype)


# ------------------------------------------------------------------------------------------------ conv3x3 prologue
ROUTES = {   # route -> (tuning entries, expected (c32, generic, s32) launches)
    "generic": (dict(conv_s32=0, conv_c32=0, conv_sk=0), (0, 1, 0)),
    "big64": (dict(conv_big4_min=1, conv_mt4_min_wgs=1, conv_sk=0), (0, 1, 0)),
    "sk": (dict(conv_sk=2, conv_s32=0, conv_c32=0), (0, 1, 0)),
    "c32": (dict(conv_c32=1, conv_c32_min_tiles=1, conv_s32=0), (1, 0, 0)),
    "s32": (dict(conv_s32=7, conv_s32_min_tiles=1, conv_c32=0), (0, 0, 1)),
    "big32": (dict(conv_big_min=1, conv_mt4_min_wgs=1 << 40, conv_s32=0, conv_c32=0, conv_sk=0), (0, 1, 0)),
    "rows8x64": (dict(conv_mt4_min_wgs=1, conv_big4_min=1 << 40, conv_s32=0, conv_c32=0, conv_sk=0), (0, 1, 0)),
}
# route -> what ld_last_route must report for it (the routes whose tile does not depend on the case's shape)
TILES = {
    "big64": dict(family="generic", MT=4, NW=4, raw=False, sk=False, side=False),
    "big32": dict(family="generic", MT=2, NW=4, raw=False, sk=False, side=False),
    "rows8x64": dict(family="generic", MT=4, NW=2, raw=False, sk=False, side=False),
}


def conv_sources(k, dtype):
    c = k.c
    if c.src == "slice":                                  # the other channels of the wider tensor hold NaN
        wide = hh.padded(k.a.x, 2 * c.cin).to(hh.TDT[dtype])
        return [gn_src(k.a, dtype, x_dev=wide, stride=2 * c.cin)]
    a = gn_src(k.a, dtype, ups=int(c.src == "ups"))
    if c.src in ("one", "ups"):
        return [a]
    raw = hh.make_src(hh.nhwc(k.raw, dtype), c.cin - k.cn)
    return [a, raw] if c.src == "gn+raw" else [raw, a]


def run_conv(k, dtype, route, t=0):
    c = k.c
    sets, want = ROUTES[route]
    w = hh.pack(R.onehot_weight(c.cin, c.cout), dtype, 3)
    bias = torch.zeros(c.cout, device=hh.DEV)
    with routed(**sets) as lib:
        if route == "sk":
            assert kernel_table(lib)["conv_sk"] == 2
        before = counters()
        out = hh.conv3x3(conv_sources(k, dtype), w, bias, c.B, c.H, c.W, c.cout, dtype, t_ptr=t_tensor(c.film, t))
        assert launched(before) == want, (route, launched(before))
        if route in TILES:
            assert hh.last_route(cabi.ROUTE_CONV3X3) == TILES[route], (route, hh.last_route(cabi.ROUTE_CONV3X3))
    return hh.nchw(out)


def check_conv(k, got, dtype, what):
    pad = got[:, ~k.inside]
    assert bool((pad == 0).all()), (what, int((pad != 0).sum()), float(pad.abs().max()))      # padding: exactly zero
    check(k, got, dtype, what)


@pytest.mark.parametrize("idx", [i for i, c in enumerate(R.CONV_CASES) if c.route != "s32"],
                         ids=[c.id for c in R.CONV_CASES if c.route != "s32"])
def test_conv3x3_prologue(idx):
    c = R.CONV_CASES[idx]
    for dtype in R.conv_route_dtypes(c):
        for t in (R.T_VALUES if c.film == "table" else (0,)):
            k = R.conv_case(idx, dtype, t)
            check_conv(k, run_conv(k, dtype, c.route, t), dtype, f"conv3x3 {c.id} t={t}")


@pytest.mark.parametrize("dtype", R.LOWP)
@pytest.mark.parametrize("idx", [i for i, c in enumerate(R.CONV_CASES) if c.route == "s32"],
                         ids=[c.id for c in R.CONV_CASES if c.route == "s32"])
def test_conv3x3_prologue_lean_and_generic(idx, dtype):
    """conv3x3_s32.hip has its own copy of the coefficient arithmetic: held to ref64, as is the generic kernel on the
    same inputs; between the two, a storage ulp here and there (the relation test_hip_ops.py holds them to)."""
    c = R.CONV_CASES[idx]
    k = R.conv_case(idx, dtype)
    lean, gen = run_conv(k, dtype, "s32"), run_conv(k, dtype, "generic")
    check_conv(k, lean, dtype, f"conv3x3 lean {c.id}")
    check_conv(k, gen, dtype, f"conv3x3 generic {c.id}")
    assert hh.rel_err(lean, gen) < hh.RTOL[dtype] / 2


# ------------------------------------------------------------------------------------------------ ld_conv1x1, GN_TAIL
def run_tail(k, dtype, lead_args):
    c = k.c
    x = hh.nhwc(hh.rand((c.B, R.TAIL_CIN, c.H, c.W), 77), dtype)                # finite inputs, all-zero weight
    w = hh.pack(torch.zeros(c.cout, R.TAIL_CIN, 1, 1), dtype, 1)
    res = None if k.res is None else hh.nhwc(k.res, dtype)
    with routed(lead_args=lead_args):
        out = hh.conv1x1([hh.make_src(x, R.TAIL_CIN)], w, c.B, c.H, c.W, c.cout, dtype, bias=torch.zeros(c.cout, device=hh.DEV),
                         epi=cabi.EPI_GN_TAIL, residual=res, gn_tail=gn_src(k.a, dtype))
        torch.cuda.synchronize()
    return hh.nchw(out)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("idx", range(len(R.TAIL_CASES)), ids=[c.id for c in R.TAIL_CASES])
def test_conv1x1_gn_tail(idx, dtype):
    """out = 0 + SiLU(GN(tail)) (+ residual): the preloaded-tail launch (lead_args = 1) and the plain one, bit-equal."""
    k = R.tail_case(idx, dtype)
    got = run_tail(k, dtype, 1)
    check(k, got, dtype, f"gn_tail {k.c.id}")
    got0 = run_tail(k, dtype, 0)
    assert torch.equal(got, got0), int((got != got0).sum())


# ------------------------------------------------------------------------------------------------ refusals
def _guarded(n, dtype):
    """n output elements between two NaN guard bands of 64 elements."""
    return hh.nans(n + 128, dtype=hh.TDT[dtype])


def _untouched(buf):
    torch.cuda.synchronize()
    return bool(torch.isnan(buf.float()).all())


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("why", ["groups32", "indivisible", "strided", "odd_pool"])
def test_gn_apply_refuses(why, dtype):
    """More than 16 groups (the stripe reduction has 16 lanes per group), C not divisible by the groups, an operand
    that is not dense, a pool on an odd map: an error code, and nothing written."""
    B, Cc, H, W = 2, 64, 5 if why == "odd_pool" else 4, 6
    groups = {"groups32": 32, "indivisible": 12}.get(why, 8)
    x = hh.rand((B, Cc, H, W), 60)
    stats = torch.zeros(B, cabi.STAT_STRIPES, groups, 2, dtype=torch.float64, device=hh.DEV)
    stats[:, 0, :, 1] = 1.0
    A = cabi.GnApplyArgs()
    wide = hh.padded(x, 2 * Cc, fill=0.0).to(hh.TDT[dtype])
    A.a = hh.make_src(wide if why == "strided" else hh.nhwc(x, dtype), Cc, stride=2 * Cc if why == "strided" else 0,
                      gn=(stats, torch.ones(Cc, device=hh.DEV), torch.zeros(Cc, device=hh.DEV), groups), act=cabi.ACT_SILU)
    A.pool = int(why == "odd_pool")
    buf = _guarded(B * H * W * Cc, dtype)
    A.out, A.B, A.H, A.W, A.dtype = buf.data_ptr() + 64 * buf.element_size(), B, H, W, cabi.dtype_code(dtype)
    rc = cabi.lib().ld_gn_apply(C.byref(A), hh.st())
    assert rc != 0 and cabi.lib().ld_last_error()
    assert _untouched(buf)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("groups", [32, 12])
def test_conv_prologue_and_tail_refuse(groups, dtype):
    """The same two group checks in front of ld_conv3x3's prologue and ld_conv1x1's GN_TAIL operand."""
    B, Cc, H, W = 2, 64, 4, 6
    x = hh.nhwc(hh.rand((B, Cc, H, W), 61), dtype)
    stats = torch.zeros(B, cabi.STAT_STRIPES, groups, 2, dtype=torch.float64, device=hh.DEV)
    stats[:, 0, :, 1] = 1.0
    src = hh.make_src(x, Cc, gn=(stats, torch.ones(Cc, device=hh.DEV), torch.zeros(Cc, device=hh.DEV), groups), act=cabi.ACT_SILU)
    bias = torch.zeros(Cc, device=hh.DEV)
    a = cabi.Conv3x3Args()
    a.src[0], a.nsrc = src, 1
    w3 = hh.pack(R.onehot_weight(Cc, Cc), dtype, 3)
    buf = _guarded(B * H * W * Cc, dtype)
    a.weight, a.bias, a.out = w3.data_ptr(), bias.data_ptr(), buf.data_ptr() + 64 * buf.element_size()
    a.B, a.H, a.W, a.Cout, a.dtype = B, H, W, Cc, cabi.dtype_code(dtype)
    assert cabi.lib().ld_conv3x3(C.byref(a), hh.st()) != 0
    assert _untouched(buf)
    a1 = cabi.Conv1x1Args()
    a1.src[0], a1.nsrc = hh.make_src(x, Cc), 1
    w1 = hh.pack(torch.zeros(Cc, Cc, 1, 1), dtype, 1)
    a1.weight, a1.bias, a1.epilogue, a1.hidden, a1.q_scale, a1.gn_tail = w1.data_ptr(), bias.data_ptr(), cabi.EPI_GN_TAIL, 128, 1.0, src
    a1.out = buf.data_ptr() + 64 * buf.element_size()
    a1.B, a1.H, a1.W, a1.Cout, a1.dtype = B, H, W, Cc, cabi.dtype_code(dtype)
    assert cabi.lib().ld_conv1x1(C.byref(a1), hh.st()) != 0
    assert _untouched(buf)
