"""Every tile instantiation of ld_conv3x3's generic kernel and of ld_conv1x1, forced through the routing table and
CONFIRMED with ld_last_route after every launch -- never inferred from a threshold: a test that relies on default
thresholds silently tests another tile the day a threshold moves.

The small shapes of test_hip_exact.py / test_hip_ops.py / test_hip_norm.py all fall below conv_mt4_min_wgs, conv_big_min,
c1_small_min and c1_big_min and run <MT, NW> = <2, 2>; the other tiles were seen only by whole-model tests under 5e-2.
Here each of <2,2>, <4,2>, <2,4>, <4,4> runs the exact probes of tests/exact_probes.py (torch.equal on the output and on
the fp64 statistics; proved on the CPU by tests/test_exact_probes.py) in all three storage types, on ragged maps and on
maps of whole tiles only, with every output buffer holding NaN before the launch.  The non-linear 1x1 epilogues are held
to the reference and bound of their existing test AND to the <2,2> result on the same inputs, bit for bit: the K order
per output element does not depend on the tile (conv1x1.hip: acc[m][j] takes the chunks in order in mfma_chunk; rs[it]
is a per-lane sum over the chunks joined by kq4_sum; build_gn_coef runs on 256 threads whatever the tile).

The GroupNorm-prologue (non-RAW) instantiations of the 3x3 tiles are also reached with conv_raw = 0 on the exact probes;
their prologue arithmetic is held to fp64 by the big32 / rows8x64 / big64 routes of tests/test_hip_norm.py."""
import contextlib
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from localdiffusion_hallucination_amd import _cabi as cabi       # noqa: E402
from localdiffusion_hallucination_amd.tuning import kernel_table  # noqa: E402
from oracle import unet_ref                                        # noqa: E402
import exact_probes as P                                           # noqa: E402
import hip_helpers as hh                                           # noqa: E402
import norm_ref as R                                               # noqa: E402

DTYPES = ["fp32", "bf16", "fp16"]
LOWP = ["bf16", "fp16"]
NEVER = 1 << 40                                # a threshold no launch reaches
TILES = [(2, 2), (4, 2), (2, 4), (4, 4)]        # <MT, NW>
TILE_ID = {(2, 2): "mt2nw2", (4, 2): "mt4nw2", (2, 4): "mt2nw4", (4, 4): "mt4nw4"}
OBSERVED = set()                                # (op, dtype, decoded route) of every launch of this file
RAN = []


@pytest.fixture(autouse=True)
def _ran(request):
    yield
    RAN.append(request.node.nodeid)


@contextlib.contextmanager
def routed(**sets):
    """Entries of the library's routing table for the duration of the block."""
    lib = cabi.lib()
    keep = kernel_table(lib)
    try:
        for k, v in sets.items():
            cabi.check(lib.ld_tuning_set(k.encode(), v), "tuning_set")
        yield lib
    finally:
        for k, v in keep.items():
            cabi.check(lib.ld_tuning_set(k.encode(), v), "tuning_set")


def tiles_for(cout):
    """The tiles a Cout can run on: 64-channel tiles need Cout % 64 == 0."""
    return [t for t in TILES if t[0] == 2 or cout % 64 == 0]


def pairs(shapes, cout_of=lambda s: s[2], tiles=TILES):
    """(tile, shape) for every one of ``tiles`` the shape's Cout fits, with ids."""
    out = [(t, s) for s in shapes for t in tiles_for(cout_of(s)) if t in tiles]
    return dict(argvalues=out, ids=[TILE_ID[t] + "-" + "x".join(map(str, s if isinstance(s, tuple) else (s,))) for t, s in out])


def want(ref, dtype):
    return P.stored(ref, dtype)


conv3x3_probe = functools.lru_cache(maxsize=None)(P.conv3x3)
conv3x3_addend_probe = functools.lru_cache(maxsize=None)(P.conv3x3_addend)
conv3x3_cat_probe = functools.lru_cache(maxsize=None)(P.conv3x3_concat_upsample)
conv3x3_side_probe = functools.lru_cache(maxsize=None)(P.conv3x3_side)
conv1x1_probe = functools.lru_cache(maxsize=None)(P.conv1x1)
conv1x1_cat_probe = functools.lru_cache(maxsize=None)(P.conv1x1_concat)
conv1x1_unshuffle_probe = functools.lru_cache(maxsize=None)(P.conv1x1_unshuffle)


# ================================================================================================ ld_conv3x3
def sets3(tile, conv_raw=1, sk=0):
    """Routing entries that force <MT, NW> of the generic kernel (conv3x3.hip, dispatch)."""
    MT, NW = tile
    d = dict(conv_s32=0, conv_c32=0, conv_sk=sk, conv_raw=conv_raw, conv_mt4_min_wgs=1 if MT == 4 else NEVER)
    d["conv_big4_min" if MT == 4 else "conv_big_min"] = 1 if NW == 4 else NEVER
    return d


def expect3(dtype, tile, raw=True, sk=False, side=False):
    got = hh.last_route(cabi.ROUTE_CONV3X3)
    exp = dict(family="generic", MT=tile[0], NW=tile[1], raw=raw, sk=sk, side=side)
    assert got == exp, (got, exp)
    OBSERVED.add(("3x3", dtype, tile[0], tile[1], "raw" if raw else "general", "sk" if sk else "-", "side" if side else "-"))


def conv3(tile, srcs, p, B, H, W, cout, dtype, stats=True, conv_raw=1, sk=0, **kw):
    """One launch on ``tile`` (route asserted) -> (out, statistics buffer or None)."""
    groups = P.tile_groups(cout)
    st = hh.stats_buffer(B, groups) if stats else None
    with routed(**sets3(tile, conv_raw, sk)):
        out = hh.conv3x3(srcs, hh.pack(p.w, dtype, 3), p.b.to(hh.DEV), B, H, W, cout, dtype, stats=st, groups=groups, **kw)
        expect3(dtype, tile, raw=bool(conv_raw) and not sk, sk=bool(sk), side="side" in kw)
        torch.cuda.synchronize()
    return out, st


def assert_conv(out, st, p, dtype, what=""):
    got, exp = hh.nchw(out if not isinstance(out, tuple) else out[0]), want(p.ref, dtype)
    assert torch.equal(got, exp), (what, int((got != exp).sum()), float((got - p.ref).abs().max()))
    if st is not None:
        assert torch.equal(st.sum(1).cpu(), p.stats), (what, float((st.sum(1).cpu() - p.stats).abs().max()))


PLAIN3 = ([(t, s) for s in P.TILE3_RAGGED32 + [P.TILE3_WHOLE[32]] for t in TILES if t[0] == 2] +
          [(t, s) for s in P.TILE3_RAGGED64 + [P.TILE3_WHOLE[64]] for t in TILES if t[0] == 4])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,shape", PLAIN3, ids=[TILE_ID[t] + "-" + "x".join(map(str, s)) for t, s in PLAIN3])
def test_conv3x3_plain(tile, shape, dtype):
    """Output and fp64 statistics equal to the integer reference; with odd / 1024 in the bias the stored output is the one
    round-to-nearest-even of the exact value.  On two ragged maps and on a map of whole tiles (every workgroup on the FULL
    emit path) per channel width, in the RAW instantiation and (conv_raw = 0) in the general one."""
    B, cin, cout, H, W = shape
    for frac in (False, True):
        p = conv3x3_probe(B, cin, cout, H, W, frac=frac, groups=P.tile_groups(cout))
        for conv_raw in (1, 0):
            out, st = conv3(tile, [hh.make_src(hh.nhwc(p.x, dtype), cin)], p, B, H, W, cout, dtype, stats=not frac, conv_raw=conv_raw)
            assert_conv(out, st, p, dtype, (frac, conv_raw))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", TILES, ids=[TILE_ID[t] for t in TILES])
def test_conv3x3_channel_slice_and_second_source(tile, dtype):
    """pix_stride: the first 32 channels come from a 64-channel tensor whose other channels hold NaN, the other 32 from a
    second source; ragged 40 x 24."""
    B, cin, cout, H, W = P.TILE3_RAGGED32[0] if tile[0] == 2 else P.BIG64_SHAPE
    p = conv3x3_probe(B, cin, cout, H, W)
    wide = hh.padded(p.x[:, :32], 64).to(hh.TDT[dtype])
    srcs = [hh.make_src(wide, 32, stride=64), hh.make_src(hh.nhwc(p.x[:, 32:].contiguous(), dtype), 32)]
    out, st = conv3(tile, srcs, p, B, H, W, cout, dtype)
    assert_conv(out, st, p, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,cout", **pairs(P.TILE3_CAT_COUTS, cout_of=lambda c: c))
def test_conv3x3_concat_upsample(tile, cout, dtype):
    """Two sources, the first at half resolution (nearest x2 on load), 40 x 24."""
    B, c1, c2, H, W = P.TILE3_CAT
    p = conv3x3_cat_probe(B, c1, c2, cout, H, W, groups=P.tile_groups(cout))
    srcs = [hh.make_src(hh.nhwc(p.x1, dtype), c1, ups=1), hh.make_src(hh.nhwc(p.x2, dtype), c2)]
    out, st = conv3(tile, srcs, p, B, H, W, cout, dtype)
    assert_conv(out, st, p, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,shape", **pairs(P.TILE3_ADDEND_SHAPES))
def test_conv3x3_addend(tile, shape, dtype):
    """ld_conv3x3_args.addend (on by default in the sampler: Tuning.fusion_fold): summed before the statistics, in the
    non-FULL emit path of conv3x3_body.hip.h only -- output and statistics."""
    B, cin, cout, H, W = shape
    p = conv3x3_addend_probe(B, cin, cout, H, W)
    add = hh.nhwc(p.add, dtype)
    out, st = conv3(tile, [hh.make_src(hh.nhwc(p.x, dtype), cin)], p, B, H, W, cout, dtype, addend=add)
    assert_conv(out, st, p, dtype)


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("tile,shape", **pairs(P.TILE3_SK_SHAPES, tiles=[(2, 2), (4, 2)]))
def test_conv3x3_split_k(tile, shape, dtype):
    """conv_sk = 2 on <2,2> and <4,2> (split-K exists on the 8-row tiles only): eight chunks on whole tiles, an odd chunk
    count on a ragged map."""
    B, cin, cout, H, W = shape
    p = conv3x3_probe(B, cin, cout, H, W)
    out, st = conv3(tile, [hh.make_src(hh.nhwc(p.x, dtype), cin)], p, B, H, W, cout, dtype, sk=2)
    assert_conv(out, st, p, dtype)


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("tile", [(2, 2), (4, 2)], ids=["mt2nw2", "mt4nw2"])
def test_conv3x3_side_output(tile, dtype):
    """The res_conv as a second output of the launch on both register tiles that carry it; ragged 17 x 23."""
    p = conv3x3_side_probe()
    B, c1, c2, cout, H, W = 2, 64, 32, 64, 17, 23
    srcs = [hh.make_src(hh.nhwc(p.x1, dtype), c1), hh.make_src(hh.nhwc(p.x2, dtype), c2)]
    out, st = conv3(tile, srcs, p, B, H, W, cout, dtype, side=(hh.pack(p.wr, dtype, 1), p.br.to(hh.DEV)))
    assert_conv(out, st, p, dtype)
    assert torch.equal(hh.nchw(out[1]), p.ref_side)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv3x3_refuses_statistics_groups_that_straddle_a_channel_tile(dtype):
    """Cout = 96 with 8 groups is 12 channels per group: they straddle the 32-channel tile, whose epilogue adds whole
    groups only.  Until finding 142 the call was accepted and the statistics came back wrong (from group 2 on at
    (1, 32, 96, 33, 20); the output itself was right).  Now: LD_EINVAL, nothing launched, nothing written."""
    B, cin, cout, H, W = P.TILE3_RAGGED32[1]
    p = conv3x3_probe(B, cin, cout, H, W, groups=P.tile_groups(cout))
    keep = (hh.nhwc(p.x, dtype), hh.pack(p.w, dtype, 3), p.b.to(hh.DEV), hh.nans(B, H, W, cout, dtype=hh.TDT[dtype]), hh.stats_buffer(B, 8))
    a = cabi.Conv3x3Args()
    a.src[0], a.nsrc = hh.make_src(keep[0], cin), 1
    a.weight, a.bias, a.out, a.out_stats, a.out_groups = keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(), 8
    a.B, a.H, a.W, a.Cout, a.dtype = B, H, W, cout, cabi.dtype_code(dtype)
    lib = cabi.lib()
    before = lib.ld_last_route(cabi.ROUTE_CONV3X3)
    assert lib.ld_conv3x3(C.byref(a), hh.st()) == -1 and b"out_groups" in lib.ld_last_error()
    torch.cuda.synchronize()
    assert lib.ld_last_route(cabi.ROUTE_CONV3X3) == before                   # a refused call leaves the route word alone
    assert bool(torch.isnan(keep[3].float()).all()) and bool((keep[4] == 0).all())


# ================================================================================================ ld_conv1x1
STAGING = [(1, 0), (1, 1), (2, 0), (2, 1), (4, 0), (4, 1)]           # (G, lead_args)


def sets1(tile, G=1, lead=0):
    """Routing entries that force <MT, NW>, the K staging and the argument passing (conv1x1.hip, dispatch)."""
    MT, NW = tile
    d = dict(c1_small_min=0 if MT == 4 else NEVER, c1_big_min=0 if NW == 4 else NEVER, lead_args=lead)
    if G == 4:
        d.update(c1_group=1, c1_group_max_px=NEVER, c1_group_min_ch=1)
    elif G == 2:
        d.update(c1_group=1, c1_group_max_px=0, c1_pair_max_px=NEVER)
    else:
        d.update(c1_group=0)
    return d


def expect1(dtype, tile, epi, G, lead):
    got = hh.last_route(cabi.ROUTE_CONV1X1)
    exp = dict(MT=tile[0], NW=tile[1], epi=epi, G=G, lead=lead)
    assert got == exp, (got, exp)
    OBSERVED.add(("1x1", dtype, tile[0], tile[1], epi, G, lead))


def conv1(tile, G, lead, want_lead, srcs, wp, B, H, W, cout, dtype, epi=cabi.EPI_PLAIN, want_epi=None, **kw):
    """One launch on ``tile`` with G chunks per barrier pair (route asserted) -> NHWC device output."""
    with routed(**sets1(tile, G, lead)):
        out = hh.conv1x1(srcs, wp, B, H, W, cout, dtype, epi=epi, **kw)
        expect1(dtype, tile, epi if want_epi is None else want_epi, G, want_lead)
        torch.cuda.synchronize()
    return out


def klead(G, lead):
    """launch_epi: the preloaded-argument kernel takes grouped launches without per-batch weights."""
    return "klead" if lead and G > 1 else "none"


def tlead(G, lead):
    return "tlead" if lead and G > 1 else "none"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,shape", **pairs(P.TILE1_SHAPES))
def test_conv1x1_plain(tile, shape, dtype):
    """LD_EPI_PLAIN at every combination of G in {1, 2, 4} and lead_args in {0, 1}, integer bias and the rounding variant:
    391 pixels = one 256-pixel tile + 135, the last 16-pixel group holds 7."""
    B, cin, cout, H, W = shape
    for frac in (False, True):
        p = conv1x1_probe(B, cin, cout, H, W, frac=frac)
        x, wp, b = hh.nhwc(p.x, dtype), hh.pack(p.w, dtype, 1), p.b.to(hh.DEV)
        for G, lead in STAGING:
            out = conv1(tile, G, lead, klead(G, lead), [hh.make_src(x, cin)], wp, B, H, W, cout, dtype, bias=b)
            got = hh.nchw(out)
            assert torch.equal(got, want(p.ref, dtype)), (frac, G, lead, int((got != want(p.ref, dtype)).sum()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,shape", **pairs(P.TILE1_GROUP_SHAPES))
def test_conv1x1_partial_groups(tile, shape, dtype):
    """5 and 13 chunks (16-bit; 10 and 26 in fp32): a partial last group of four and of two; and a map below one tile."""
    B, cin, cout, H, W = shape
    p = conv1x1_probe(B, cin, cout, H, W)
    x, wp, b = hh.nhwc(p.x, dtype), hh.pack(p.w, dtype, 1), p.b.to(hh.DEV)
    for G, lead in STAGING:
        out = conv1(tile, G, lead, klead(G, lead), [hh.make_src(x, cin)], wp, B, H, W, cout, dtype, bias=b)
        assert torch.equal(hh.nchw(out), p.ref), (G, lead)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,shape", **pairs(P.TILE1_SHAPES))
def test_conv1x1_residual_and_per_batch_weights(tile, shape, dtype):
    """LD_EPI_RES with an integer residual (the second-operand prefetch and its 16-byte pairing depend on MT and NW); then a
    weight per batch element, which the preloaded-argument kernel must decline (lead = none)."""
    B, cin, cout, H, W = shape
    p = conv1x1_probe(B, cin, cout, H, W, residual=True)
    x, b, res = hh.nhwc(p.x, dtype), p.b.to(hh.DEV), hh.nhwc(p.res, dtype)
    wp = hh.pack(p.w, dtype, 1)
    for G, lead in ((4, 1), (2, 1), (1, 0)):
        out = conv1(tile, G, lead, klead(G, lead), [hh.make_src(x, cin)], wp, B, H, W, cout, dtype, epi=cabi.EPI_RES, bias=b, residual=res)
        assert torch.equal(hh.nchw(out), p.ref), (G, lead)
    p = conv1x1_probe(B, cin, cout, H, W, residual=True, per_batch=True)
    x, b, res = hh.nhwc(p.x, dtype), p.b.to(hh.DEV), hh.nhwc(p.res, dtype)
    wp = torch.stack([hh.pack(p.w[i], dtype, 1) for i in range(B)]).contiguous()
    es = 4 if dtype == "fp32" else 2
    for G in (4, 1):
        out = conv1(tile, G, 1, "none", [hh.make_src(x, cin)], wp, B, H, W, cout, dtype, epi=cabi.EPI_RES, bias=b, residual=res,
                    bstride=cout * cin * es)
        assert torch.equal(hh.nchw(out), p.ref), ("per batch", G)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,cout", **pairs(P.TILE1_VARIANT_COUTS, cout_of=lambda c: c))
def test_conv1x1_two_sources_and_unshuffle(tile, cout, dtype):
    B, c1, c2, H, W = P.TILE1_CAT
    p = conv1x1_cat_probe(B, c1, c2, cout, H, W)
    srcs = [hh.make_src(hh.nhwc(p.x1, dtype), c1), hh.make_src(hh.nhwc(p.x2, dtype), c2)]
    wp, b = hh.pack(p.w, dtype, 1), p.b.to(hh.DEV)
    for G, lead in ((4, 1), (2, 0), (1, 0)):
        out = conv1(tile, G, lead, klead(G, lead), srcs, wp, B, H, W, cout, dtype, bias=b)
        assert torch.equal(hh.nchw(out), p.ref), ("concat", G, lead)
    B, c, H, W = P.TILE1_UNSHUFFLE
    p = conv1x1_unshuffle_probe(B, c, cout, H, W)
    x, wp, b = hh.nhwc(p.x, dtype), hh.pack(p.w, dtype, 1, unshuffle=1), p.b.to(hh.DEV)
    for G, lead in ((4, 1), (2, 0), (1, 0)):
        out = conv1(tile, G, lead, klead(G, lead), [hh.make_src(x, c)], wp, B, H, W, cout, dtype, bias=b, unshuffle=1)
        assert torch.equal(hh.nchw(out), p.ref), ("unshuffle", G, lead)


# ------------------------------------------------------------------------------------------------ non-linear epilogues
def _q(x, dtype):
    return x.to(hh.TDT[dtype]).float()


QKV_SHAPE = (2, 64, 17, 23)             # B, c, H, W: hidden = 128, Cout = 384


@functools.lru_cache(maxsize=None)
def qkv_inputs(dtype):
    """The operands and fp32 references of test_hip_ops.test_qkv_epilogues, on the ragged 17 x 23 map."""
    B, c, H, W = QKV_SHAPE
    hid = 128
    x = _q(hh.rand((B, c, H, W), 30, -2, 2), dtype)
    g = hh.rand((1, c, 1, 1), 31, 0.5, 1.5)
    w = _q(hh.rand((3 * hid, c, 1, 1), 32, -0.3, 0.3), dtype)
    qkv = F.conv2d(unet_ref.rms_norm(x, g), w)
    q, k, v = qkv.chunk(3, dim=1)
    qs = q.reshape(B, 4, 32, H * W).softmax(dim=-2).reshape(B, hid, H, W) * 32 ** -0.5
    return x, g, w, torch.cat([qs, k, v], 1), torch.cat([q * 32 ** -0.5, k, v], 1), k.amax(dim=(2, 3))


def run_qkv(tile, G, lead, dtype):
    """-> (LINEAR output, decoded kmax [B, hidden], FULL output), NCHW fp32 on the CPU."""
    B, c, H, W = QKV_SHAPE
    hid = 128
    x, g, w = qkv_inputs(dtype)[:3]
    xd, wp = hh.nhwc(x, dtype), hh.pack(w, dtype, 1, scale_in=g.flatten() * math.sqrt(c))
    kmax = torch.zeros(B, cabi.STAT_STRIPES, hid, dtype=torch.int32, device=hh.DEV)
    lin = conv1(tile, G, lead, klead(G, lead), [hh.make_src(xd, c)], wp, B, H, W, 3 * hid, dtype, epi=cabi.EPI_QKV_LINEAR, rms_in=1,
                kmax_out=kmax)
    full = conv1(tile, G, lead, klead(G, lead), [hh.make_src(xd, c)], wp, B, H, W, 3 * hid, dtype, epi=cabi.EPI_QKV_FULL, rms_in=1)
    return hh.nchw(lin), hh.dec_max(kmax).amax(dim=1), hh.nchw(full)


@functools.lru_cache(maxsize=None)
def qkv_small_tile(dtype):
    return run_qkv((2, 2), 1, 0, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", TILES, ids=[TILE_ID[t] for t in TILES])
def test_conv1x1_qkv_epilogues(tile, dtype):
    """rms_in + LD_EPI_QKV_LINEAR (with kmax_out) and LD_EPI_QKV_FULL: the reference and bound of
    test_hip_ops.test_qkv_epilogues, and bit-equal to the <2,2> plain-K-loop result on the same inputs.  kmax is the
    maximum of the k channels before they are rounded to storage: held to the fp32 reference's maximum under the same
    bound, and to the <2,2> word."""
    ref_lin, ref_full, ref_kmax = qkv_inputs(dtype)[3:]
    tol = hh.RTOL[dtype] * (3 if dtype != "fp32" else 5)
    base = qkv_small_tile(dtype)
    for G, lead in ((4, 1), (2, 1), (1, 0)):
        lin, kmax, full = run_qkv(tile, G, lead, dtype)
        e = (hh.rel_err(lin, ref_lin), hh.rel_err(full, ref_full), hh.rel_err(kmax, ref_kmax))
        print(f"qkv {TILE_ID[tile]} {dtype} G={G} lead={lead}: linear {e[0]:.2e} full {e[1]:.2e} kmax {e[2]:.2e} (bound {tol:.2e})")
        assert max(e) < tol, (G, lead, e)
        assert torch.equal(lin, base[0]) and torch.equal(kmax, base[1]) and torch.equal(full, base[2]), (G, lead)


TAIL_SHAPE = (2, 64, 32, 64, 17, 23)    # B, c1, c2, cout, H, W


@functools.lru_cache(maxsize=None)
def tail_inputs(dtype):
    """The operands and reference of test_hip_ops.test_conv1x1_gn_tail_epilogue on the ragged 17 x 23 map, plus a residual."""
    B, c1, c2, cout, H, W = TAIL_SHAPE
    x1, x2 = _q(hh.rand((B, c1, H, W), 223), dtype), _q(hh.rand((B, c2, H, W), 224), dtype)
    raw2 = _q(hh.rand((B, cout, H, W), 225, -2, 3), dtype)
    w, b = _q(hh.rand((cout, c1 + c2, 1, 1), 226, -0.2, 0.2), dtype), hh.rand((cout,), 227)
    gamma, beta = hh.rand((cout,), 228, 0.5, 1.5), hh.rand((cout,), 229, -0.3, 0.3)
    res = _q(hh.rand((B, cout, H, W), 230), dtype)
    ref = F.conv2d(torch.cat([x1, x2], 1), w, b) + F.silu(F.group_norm(raw2, 8, gamma, beta))
    return x1, x2, raw2, w, b, gamma, beta, res, ref


def run_tail_random(tile, G, lead, dtype, with_res):
    B, c1, c2, cout, H, W = TAIL_SHAPE
    x1, x2, raw2, w, b, gamma, beta, res, _ = tail_inputs(dtype)
    tail = hh.make_src(hh.nhwc(raw2, dtype), cout, gn=(hh.stats_striped(raw2, 8), gamma.to(hh.DEV), beta.to(hh.DEV), 8), act=cabi.ACT_SILU)
    resd = hh.nhwc(res, dtype) if with_res else None
    out = conv1(tile, G, lead, tlead(G, lead), [hh.make_src(hh.nhwc(x1, dtype), c1), hh.make_src(hh.nhwc(x2, dtype), c2)],
                hh.pack(w, dtype, 1), B, H, W, cout, dtype, epi=cabi.EPI_GN_TAIL, want_epi=hh.EPI_GN_TAIL_RES if with_res else cabi.EPI_GN_TAIL,
                bias=b.to(hh.DEV), gn_tail=tail, residual=resd)
    return hh.nchw(out)


@functools.lru_cache(maxsize=None)
def tail_small_tile(dtype, with_res):
    return run_tail_random((2, 2), 1, 0, dtype, with_res)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("tile", TILES, ids=[TILE_ID[t] for t in TILES])
def test_conv1x1_gn_tail_epilogue(tile, with_res, dtype):
    """LD_EPI_GN_TAIL without and with `residual` (its own instantiation): the reference and bound of
    test_hip_ops.test_conv1x1_gn_tail_epilogue (+ the residual), and bit-equal to the <2,2> result."""
    ref = tail_inputs(dtype)[8] + (tail_inputs(dtype)[7] if with_res else 0)
    for G, lead in ((4, 1), (2, 1), (4, 0), (1, 0)):
        got = run_tail_random(tile, G, lead, dtype, with_res)
        e = hh.rel_err(got, ref)
        print(f"gn_tail {TILE_ID[tile]} {dtype} res={with_res} G={G} lead={lead}: {e:.2e} (bound {hh.RTOL[dtype] * 2:.2e})")
        assert e < hh.RTOL[dtype] * 2, (G, lead, e)
        assert torch.equal(got, tail_small_tile(dtype, with_res)), (G, lead)


def run_tail_case(tile, k, dtype, lead):
    """test_hip_norm.run_tail on ``tile``: an all-zero weight, so the output is SiLU(GN(tail)) (+ residual).  One 16-bit
    K-chunk: c1_group_min_ch = 1 (sets1) makes it a grouped launch, which the preloaded-tail kernel requires."""
    c = k.c
    x = hh.nhwc(hh.rand((c.B, R.TAIL_CIN, c.H, c.W), 77), dtype)
    w = hh.pack(torch.zeros(c.cout, R.TAIL_CIN, 1, 1), dtype, 1)
    res = None if k.res is None else hh.nhwc(k.res, dtype)
    a = k.a
    tail = hh.make_src(hh.nhwc(a.x, dtype), c.cout, gn=(a.stats.to(hh.DEV), a.gamma.to(hh.DEV), a.beta.to(hh.DEV), a.G), act=a.act)
    out = conv1(tile, 4, lead, tlead(4, lead), [hh.make_src(x, R.TAIL_CIN)], w, c.B, c.H, c.W, c.cout, dtype, epi=cabi.EPI_GN_TAIL,
                want_epi=cabi.EPI_GN_TAIL if res is None else hh.EPI_GN_TAIL_RES, bias=torch.zeros(c.cout, device=hh.DEV),
                residual=res, gn_tail=tail)
    return hh.nchw(out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", TILES, ids=[TILE_ID[t] for t in TILES])
def test_conv1x1_gn_tail_against_fp64(tile, dtype):
    """The tail cases of test_hip_norm.py (norm_ref.compare against the fp64 form, unchanged) on every tile their Cout fits,
    at both lead_args: bit-equal to each other and to the <2,2> result."""
    for idx, c in enumerate(R.TAIL_CASES):
        if tile not in tiles_for(c.cout):
            continue
        k = R.tail_case(idx, dtype)
        got = run_tail_case(tile, k, dtype, 1)
        ok, worst, allow = R.compare(got, k.ref, k.d, k.d_fast, dtype, k.gid)
        i = int((worst / allow).argmax())
        print(f"gn_tail {c.id} {TILE_ID[tile]} {dtype}: err {float(worst.flatten()[i]):.3e} of {float(allow.flatten()[i]):.3e} allowed")
        assert bool(ok.all()), (c.id, (~ok).nonzero().tolist()[:8], float(worst.flatten()[i]), float(allow.flatten()[i]))
        got0 = run_tail_case(tile, k, dtype, 0)
        assert torch.equal(got, got0), (c.id, int((got != got0).sum()))
        if tile != (2, 2):
            small = run_tail_case((2, 2), k, dtype, 0)
            assert torch.equal(got, small), (c.id, int((got != small).sum()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [32, 64, 128])
def test_conv1x1_rms_res_fixed_tiles(c, dtype):
    """LD_EPI_RMS_RES normalises over ALL output channels, so its tile is fixed by Cout: <2,2>, <4,2>, <8,2>.  The operands,
    reference and bound of test_hip_ops.test_conv1x1_rms_res_epilogue_and_batched_weights on the ragged 17 x 23 map."""
    B, hid, H, W = 2, 128, 17, 23
    x = _q(hh.rand((B, hid, H, W), 33), dtype)
    res = _q(hh.rand((B, c, H, W), 34), dtype)
    w = _q(hh.rand((B, c, hid, 1, 1), 35, -0.3, 0.3), dtype)
    b, g = hh.rand((c,), 36), hh.rand((1, c, 1, 1), 37, 0.5, 1.5)
    ref = torch.cat([unet_ref.rms_norm(F.conv2d(x[i:i + 1], w[i], b), g) for i in range(B)]) + res
    wp = torch.stack([hh.pack(w[i], dtype, 1) for i in range(B)]).contiguous()
    es = 4 if dtype == "fp32" else 2
    with routed(c1_group=1, c1_group_max_px=NEVER, c1_group_min_ch=1, lead_args=1):
        out = hh.conv1x1([hh.make_src(hh.nhwc(x, dtype), hid)], wp, B, H, W, c, dtype, bias=b.to(hh.DEV), epi=cabi.EPI_RMS_RES,
                         bstride=c * hid * es, g2=(g.flatten() * math.sqrt(c)).to(hh.DEV), residual=hh.nhwc(res, dtype))
        expect1(dtype, (c // 16, 2), cabi.EPI_RMS_RES, 4, "none")
    e = hh.rel_err(hh.nchw(out), ref)
    print(f"rms_res c={c} {dtype}: {e:.2e} (bound {hh.RTOL[dtype] * 3:.2e})")
    assert e < hh.RTOL[dtype] * 3


# ================================================================================================ what was reached
def reachable():
    """Every instantiation of the generic 3x3 kernel and of the 1x1 kernel that a production build can launch and this file
    names: 3x3 -- 4 tiles x (RAW, general), and in 16-bit storage split-K (general) and the side output (RAW) on the two 8-row
    tiles; 1x1 -- per tile PLAIN at G 1 / 2 / 4 with and without preloaded arguments, RES, the two QKV epilogues, GN_TAIL and
    GN_TAIL + residual with and without the preloaded tail, and RMS_RES's three fixed tiles."""
    out = set()
    for dt in DTYPES:
        for MT, NW in TILES:
            out |= {("3x3", dt, MT, NW, kind, "-", "-") for kind in ("raw", "general")}
            out |= {("1x1", dt, MT, NW, cabi.EPI_PLAIN, G, lead) for G, lead in ((1, "none"), (2, "none"), (4, "none"), (2, "klead"), (4, "klead"))}
            out |= {("1x1", dt, MT, NW, cabi.EPI_RES, G, lead) for G, lead in ((1, "none"), (4, "none"), (2, "klead"), (4, "klead"))}
            for epi in (cabi.EPI_QKV_LINEAR, cabi.EPI_QKV_FULL):
                out |= {("1x1", dt, MT, NW, epi, G, lead) for G, lead in ((1, "none"), (2, "klead"), (4, "klead"))}
            for epi in (cabi.EPI_GN_TAIL, hh.EPI_GN_TAIL_RES):
                out |= {("1x1", dt, MT, NW, epi, G, lead) for G, lead in ((1, "none"), (4, "none"), (2, "tlead"), (4, "tlead"))}
        out |= {("1x1", dt, MT, 2, cabi.EPI_RMS_RES, 4, "none") for MT in (2, 4, 8)}
        if dt in LOWP:
            out |= {("3x3", dt, MT, 2, "general", "sk", "-") for MT in (2, 4)}
            out |= {("3x3", dt, MT, 2, "raw", "-", "side") for MT in (2, 4)}
    return out


def test_zz_every_reachable_instantiation_was_launched(request):
    """Runs last: the decoded routes this file observed are the set ``reachable`` names -- a subset of it under a partial
    selection (-k), equal to it when the whole file ran."""
    print("observed routes:")
    for r in sorted(OBSERVED, key=str):
        print("  ", r)
    exp = reachable()
    assert OBSERVED <= exp, sorted(OBSERVED - exp, key=str)
    module = request.node.nodeid.split("::")[0]
    mine = {i.nodeid for i in request.session.items if i.nodeid.split("::")[0] == module} - {request.node.nodeid}
    if mine <= set(RAN):
        assert OBSERVED == exp, sorted(exp - OBSERVED, key=str)
