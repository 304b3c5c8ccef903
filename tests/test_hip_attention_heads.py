"""The forward attention kernels at head counts other than the model's default of four.  Unet(attn_heads=h) accepts
any even h, every other forward test fixes heads = 4 / hidden = 128, and the fused 16-bit route (csrc/linattn_fused.hip)
is built for four heads: Unet takes the unfused route for every other count, and this file runs what that route is
made of -- the to_qkv epilogues, the unfused linear-attention chain, ld_attention -- at 1, 2 and 8 heads against fp32
torch and the exact probes of tests/exact_probes.py, the head-generic (workgroup-per-head) kernel of ld_linattn_kvctx,
which four heads never reach, and the whole denoiser at 2 and 8 heads against the oracle.  Tolerances are those of the
four-head tests named in each docstring."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import localdiffusion_hallucination_amd as ldh                   # noqa: E402
from localdiffusion_hallucination_amd import _cabi as cabi       # noqa: E402
from localdiffusion_hallucination_amd import rng                  # noqa: E402
from oracle import unet_ref                                        # noqa: E402
import exact_probes as P                                           # noqa: E402
import hip_helpers as hh                                           # noqa: E402
from test_hip_exact import ATTN_ROUTES, ROUTE_SETS, routed        # noqa: E402
from test_hip_unet import CASES, build, tap_table                 # noqa: E402

DTYPES = ["fp32", "bf16", "fp16"]
LOWP = ["bf16", "fp16"]


def _q(x, dtype):
    return x.to(hh.TDT[dtype]).float()


# ------------------------------------------------------------------------------------------------ to_qkv epilogues
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W", [(7, 7), (14, 14)])
@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("hid", [64, 256])
def test_qkv_epilogues(dtype, hid, c, H, W):
    """test_hip_ops.test_qkv_epilogues at hidden = 64 and 256 (2 and 8 heads), its tolerances: the q part ends after one
    64-channel tile / after four, the softmax over d runs per 32-channel head."""
    B, heads = 2, hid // 32
    x = _q(hh.rand((B, c, H, W), 30, -2, 2), dtype)
    g = hh.rand((1, c, 1, 1), 31, 0.5, 1.5)
    w = _q(hh.rand((3 * hid, c, 1, 1), 32, -0.3, 0.3), dtype)
    q, k, v = F.conv2d(unet_ref.rms_norm(x, g), w).chunk(3, dim=1)
    qs = q.reshape(B, heads, 32, H * W).softmax(dim=-2).reshape(B, hid, H, W) * 32 ** -0.5
    wp = hh.pack(w, dtype, 1, scale_in=g.flatten() * math.sqrt(c))
    tol = hh.RTOL[dtype] * (3 if dtype != "fp32" else 5)
    out = hh.conv1x1([hh.make_src(hh.nhwc(x, dtype), c)], wp, B, H, W, 3 * hid, dtype, epi=cabi.EPI_QKV_LINEAR, rms_in=1, hidden=hid)
    assert hh.rel_err(hh.nchw(out), torch.cat([qs, k, v], 1)) < tol
    out = hh.conv1x1([hh.make_src(hh.nhwc(x, dtype), c)], wp, B, H, W, 3 * hid, dtype, epi=cabi.EPI_QKV_FULL, rms_in=1, hidden=hid)
    assert hh.rel_err(hh.nchw(out), torch.cat([q * 32 ** -0.5, k, v], 1)) < tol


# ------------------------------------------------------------------------------------------------ the unfused block
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,H,W", [(32, 28, 28), (64, 14, 14)])
@pytest.mark.parametrize("heads", [2, 8])
def test_linear_attention_block_unfused(dtype, heads, c, H, W):
    """The route Unet takes for attn_heads != 4 at every storage type: EPI_QKV_LINEAR + kmax_out, ld_linattn_kmax, ctx,
    ctx_reduce, fold, ctxfold, EPI_RMS_RES against unet_ref.linear_attention(heads=...) + x, with the intermediate
    context and k maximum; the tolerances of test_hip_ops.test_linear_attention_block."""
    B, hid, n = 2, 32 * heads, H * W
    x = _q(hh.rand((B, c, H, W), 70, -2, 2), dtype)
    sd = {"a.norm.g": hh.rand((1, c, 1, 1), 71, 0.5, 1.5),
          "a.to_qkv.weight": _q(hh.rand((3 * hid, c, 1, 1), 72, -0.3, 0.3), dtype),
          "a.to_out.0.weight": hh.rand((c, hid, 1, 1), 73, -0.3, 0.3),
          "a.to_out.0.bias": hh.rand((c,), 74),
          "a.to_out.1.g": hh.rand((1, c, 1, 1), 75, 0.5, 1.5)}
    ref = unet_ref.linear_attention(sd, "a", x, heads=heads) + x
    lib, dt = cabi.lib(), cabi.dtype_code(dtype)
    xd = hh.nhwc(x, dtype)
    wq = hh.pack(sd["a.to_qkv.weight"], dtype, 1, scale_in=sd["a.norm.g"].flatten() * math.sqrt(c))
    kmax = torch.zeros(B, cabi.STAT_STRIPES, hid, dtype=torch.int32, device=hh.DEV)
    qkv = hh.conv1x1([hh.make_src(xd, c)], wq, B, H, W, 3 * hid, dtype, epi=cabi.EPI_QKV_LINEAR, rms_in=1, kmax_out=kmax, hidden=hid)
    kmax2 = torch.zeros(B, cabi.STAT_STRIPES, hid, dtype=torch.int32, device=hh.DEV)
    cabi.check(lib.ld_linattn_kmax(qkv.data_ptr(), kmax2.data_ptr(), B, n, heads, 32, dt, hh.st()), "kmax")
    nchunks = max(1, min(32, n // 256))
    ctxn = hh.nans(B, heads, 32, 32)
    ctx = hh.nans(int(lib.ld_linattn_ctx_part_floats(B, heads, 32, nchunks)))
    wfold = hh.nans(B, c * hid, dtype=hh.TDT[dtype])
    wout = sd["a.to_out.0.weight"].reshape(c, hid).contiguous().to(hh.DEV)
    cabi.check(lib.ld_linattn_ctx(qkv.data_ptr(), kmax.data_ptr(), ctx.data_ptr(), B, n, heads, 32, nchunks, dt, hh.st()), "ctx")
    cabi.check(lib.ld_linattn_ctx_reduce(ctx.data_ptr(), nchunks, ctxn.data_ptr(), B, heads, 32, hh.st()), "reduce")
    cabi.check(lib.ld_linattn_fold(ctxn.data_ptr(), wout.data_ptr(), wfold.data_ptr(), B, c, heads, 32, 0, dt, hh.st()), "fold")
    wfold2 = hh.nans(B, c * hid, dtype=hh.TDT[dtype])
    cabi.check(lib.ld_linattn_ctxfold(ctx.data_ptr(), nchunks, wout.data_ptr(), wfold2.data_ptr(), B, c, heads, 32, 0, dt, hh.st()), "ctxfold")
    assert bool(torch.isfinite(wfold.float()).all()) and bool(torch.isfinite(wfold2.float()).all())      # every element of M_b written
    assert hh.rel_err(wfold2.float().cpu(), wfold.float().cpu()) < (1e-5 if dtype == "fp32" else 1e-2)
    kv = F.conv2d(unet_ref.rms_norm(x, sd["a.norm.g"]), sd["a.to_qkv.weight"])
    _, k_, v_ = [t.reshape(B, heads, 32, n) for t in kv.chunk(3, dim=1)]
    cref = torch.einsum("bhdn,bhen->bhde", k_.softmax(dim=-1), v_)
    assert hh.rel_err(ctxn.cpu(), cref) < hh.RTOL[dtype] * 3
    kref = kv.chunk(3, dim=1)[1].reshape(B, hid, n).amax(-1)
    assert hh.rel_err(hh.dec_max(kmax).amax(1), kref) < hh.RTOL[dtype] * 3
    assert hh.rel_err(hh.dec_max(kmax2).amax(1), kref) < hh.RTOL[dtype] * 3
    es = 4 if dtype == "fp32" else 2
    out = hh.conv1x1([hh.make_src(qkv, hid, stride=3 * hid)], wfold, B, H, W, c, dtype, bias=sd["a.to_out.0.bias"].to(hh.DEV),
                     epi=cabi.EPI_RMS_RES, bstride=c * hid * es, g2=(sd["a.to_out.1.g"].flatten() * math.sqrt(c)).to(hh.DEV),
                     residual=xd, hidden=hid)
    assert hh.rel_err(hh.nchw(out), ref) < hh.RTOL[dtype] * (5 if dtype == "fp32" else 2)


# ------------------------------------------------------------------------------------------------ ld_attention
def _attention(qkv, heads, dtype):
    B, n, _ = qkv.shape
    qd = qkv.to(hh.DEV, hh.TDT[dtype]).contiguous()
    out = hh.nans(B, n, 32 * heads, dtype=hh.TDT[dtype])
    cabi.check(cabi.lib().ld_attention(qd.data_ptr(), out.data_ptr(), B, n, heads, 32, cabi.dtype_code(dtype), hh.st()), "attention")
    torch.cuda.synchronize()
    return out.float().cpu()


@pytest.mark.parametrize("route,dtype", ATTN_ROUTES)
@pytest.mark.parametrize("n", P.ATTN_HEADS_SIZES)
@pytest.mark.parametrize("heads", P.OTHER_HEADS)
def test_full_attention(route, dtype, n, heads):
    """Random q, k, v in [-1.5, 1.5] against fp32 torch at hip_helpers.RTOL, one key group and two (switched through the
    tuning table as test_hip_ops.test_full_attention_two_key_groups does; n = 49 fits one tile, where the router keeps
    one group).  B = 2: 2, 4 and 16 (image, head) pairs, which take the natural order, the interleaved and the
    whole-pair branch of the kernel's workgroup-to-XCD map."""
    B = 2
    qkv = _q(hh.rand((B, n, 96 * heads), 63, -1.5, 1.5), dtype)
    ref = P.attention_torch(qkv)
    with routed(**ROUTE_SETS[route]):
        got = _attention(qkv, heads, dtype)
    assert bool(torch.isfinite(got).all())
    assert hh.rel_err(got, ref) < hh.RTOL[dtype]


@pytest.mark.parametrize("route,dtype", ATTN_ROUTES)
@pytest.mark.parametrize("n", P.ATTN_HEADS_SIZES)
@pytest.mark.parametrize("heads", [2, 8])
def test_attention_one_hot(route, dtype, n, heads):
    """test_hip_exact.test_attention_one_hot at 2 and 8 heads: the gather v[pi(i)] bit for bit; every (image, head) has
    its own keys, permutation and values, so a head that reads another head's slice fails."""
    p = P.attention_onehot(n, heads=heads)
    with routed(**ROUTE_SETS[route]):
        got = _attention(p.qkv, heads, dtype)
    assert torch.equal(got, p.ref), (int((got != p.ref).any(-1).sum()), "queries differ")


@pytest.mark.parametrize("route,dtype", ATTN_ROUTES)
@pytest.mark.parametrize("n", P.ATTN_HEADS_SIZES)
@pytest.mark.parametrize("heads", [2, 8])
def test_attention_uniform(route, dtype, n, heads):
    """test_hip_exact.test_attention_uniform at 2 and 8 heads, asserted the same way: even channels within
    max(1e-5, 4 d) of 0 relative to 8, odd channels exactly 1 in 16-bit storage (the fp32 rule in fp32)."""
    p = P.attention_uniform(n, heads=heads)
    with routed(**ROUTE_SETS[route]):
        got = _attention(p.qkv, heads, dtype).double()
    e_even = float(got[..., 0::2].abs().max()) / 8.0
    e_odd = float((got[..., 1::2] - 1.0).abs().max())
    print(f"uniform attention heads={heads} n={n} {dtype} {route}: even {e_even:.2e} (fp32 torch {p.d_even:.2e}), odd {e_odd:.2e} "
          f"(fp32 torch {p.d_odd:.2e})")
    assert e_even <= max(1e-5, 4 * p.d_even)
    if dtype == "fp32":
        assert e_odd <= max(1e-5, 4 * p.d_odd)
    else:
        assert e_odd == 0.0


# ------------------------------------------------------------------------------------------------ ld_linattn_kvctx, the head-generic kernel
def _pack_kv(w, scale, heads, C_, dtype):
    """Per head the 64 rows (k_h | v_h) of to_qkv [3 * hidden, C, 1, 1], packed k = 1 with the RMSNorm scale folded in."""
    hid = 32 * heads
    return torch.cat([hh.pack(torch.cat([w[hid + 32 * h: hid + 32 * h + 32], w[2 * hid + 32 * h: 2 * hid + 32 * h + 32]], 0).contiguous(),
                              dtype, 1, scale_in=scale) for h in range(heads)]).contiguous()


def _kvctx(xd, wkv, B, n, C_, heads, dtype, kshift=None, terms=1):
    """ld_linattn_kvctx_terms + ld_linattn_ctx_reduce -> (rc, partials, normalised context); everything NaN before."""
    lib, dt = cabi.lib(), cabi.dtype_code(dtype)
    nchunks = max(1, min(32, n // 256))
    ctx = hh.nans(int(lib.ld_linattn_ctx_part_floats(B, heads, 32, nchunks)))
    ctxn = hh.nans(B, heads, 32, 32)
    rc = lib.ld_linattn_kvctx_terms(xd.data_ptr(), wkv.data_ptr(), cabi.ptr(kshift), ctx.data_ptr(), B, n, C_, heads, 32, nchunks, dt, terms, hh.st())
    if rc == 0:
        cabi.check(lib.ld_linattn_ctx_reduce(ctx.data_ptr(), nchunks, ctxn.data_ptr(), B, heads, 32, hh.st()), "reduce")
    torch.cuda.synchronize()
    return rc, ctx, ctxn


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("C_,H,W", P.KVCTX_HEADS_SHAPES)
@pytest.mark.parametrize("heads", P.OTHER_HEADS)
def test_linattn_kvctx_generic_uniform(dtype, heads, C_, H, W):
    """The workgroup-per-head kernel (kvctx_kernel: any head count but four, two sweeps, one weight term) on the uniform
    probe of test_hip_exact.test_linattn_kvctx_uniform generalised over heads, the same bound rule: |ctxn - mean_n v_e|
    <= max(1e-5, 4 d), d = fp32 torch's distance on the same probe.  Three pixel chunks of 262 (28 x 28: a full and a
    6-pixel tile each), one ragged tile (14 x 14), 49 pixels with four K-chunks of channels (C = 128; the expected
    context of the balanced channels is 1 / 49 there).
    Measured on the MI355X (printed per case): 0.00e+00 at 28 x 28 and 14 x 14, 4.2e-10 at 7 x 7 (the one division by
    Z = 49), at 1, 2 and 8 heads and both storage types; fp32 torch on the same probe 3.0e-7 - 4.2e-7, bound 1e-5."""
    B, n = 2, H * W
    p = P.linattn_uniform(C_, H, W, heads=heads)
    wkv = _pack_kv(p.w, p.scale.to(hh.DEV), heads, C_, dtype)
    rc, ctx, ctxn = _kvctx(hh.nhwc(p.x, dtype), wkv, B, n, C_, heads, dtype)
    cabi.check(rc, "kvctx")
    assert bool(torch.isfinite(ctx).all())
    e, bound = float((ctxn.cpu().double() - p.ref).abs().max()), max(1e-5, 4 * p.d)
    print(f"linattn ctxn (generic kernel) heads={heads} C={C_} n={n} {dtype}: {e:.2e} (fp32 torch {p.d:.2e}, bound {bound:.2e})")
    assert e <= bound


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("C_,H,W", P.KVCTX_HEADS_SHAPES)
@pytest.mark.parametrize("heads", P.OTHER_HEADS)
def test_linattn_kvctx_generic_random(dtype, heads, C_, H, W):
    """The same kernel on the operands of test_hip_ops.test_linear_attention_fused_16bit (per head its own k and v rows)
    against fp32 torch, at that test's context tolerance (2e-2 bf16, 5e-3 fp16).  Measured on the MI355X: 2.4e-3 - 4.5e-3
    in bf16, 2.4e-4 - 5.5e-4 in fp16."""
    f = 1.0 if dtype == "bf16" else 0.25
    B, hid, n = 2, 32 * heads, H * W
    x = _q(hh.rand((B, C_, H, W), 170, -2, 2), dtype)
    g = hh.rand((1, C_, 1, 1), 171, 0.5, 1.5)
    w = _q(hh.rand((3 * hid, C_, 1, 1), 172, -0.3, 0.3), dtype)
    _, k_, v_ = [t.reshape(B, heads, 32, n) for t in F.conv2d(unet_ref.rms_norm(x, g), w).chunk(3, dim=1)]
    cref = torch.einsum("bhdn,bhen->bhde", k_.softmax(dim=-1), v_)
    wkv = _pack_kv(w, (g.flatten() * math.sqrt(C_)).to(hh.DEV), heads, C_, dtype)
    rc, ctx, ctxn = _kvctx(hh.nhwc(x, dtype), wkv, B, n, C_, heads, dtype)
    cabi.check(rc, "kvctx")
    assert bool(torch.isfinite(ctx).all())
    e = hh.rel_err(ctxn.cpu(), cref)
    print(f"linattn ctxn (generic kernel, random) heads={heads} C={C_} n={n} {dtype}: {e:.2e} (bound {2e-2 * f:.1e})")
    assert e < 2e-2 * f


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("heads", P.OTHER_HEADS)
def test_linattn_kvctx_refuses_what_needs_four_heads(dtype, heads):
    """The single-sweep mode (kshift) and two-term weights exist in the wave-per-head kernel only: with any other head
    count the call returns -1 and the NaN-filled partials stay untouched."""
    B, C_, H, W = 2, 32, 14, 14
    p = P.linattn_uniform(C_, H, W, heads=heads)
    xd = hh.nhwc(p.x, dtype)
    wkv = _pack_kv(p.w, p.scale.to(hh.DEV), heads, C_, dtype)
    rc, ctx, _ = _kvctx(xd, wkv, B, H * W, C_, heads, dtype, kshift=torch.zeros(32 * heads, device=hh.DEV))
    assert rc == -1 and bool(torch.isnan(ctx).all())
    wkv2 = torch.cat([wkv, wkv])                                  # the size two-term weights would have
    rc, ctx, _ = _kvctx(xd, wkv2, B, H * W, C_, heads, dtype, terms=2)
    assert rc == -1 and bool(torch.isnan(ctx).all())


# ------------------------------------------------------------------------------------------------ the whole denoiser
def _inputs(cfg, B, H):
    x = torch.from_numpy(rng.randn((B, cfg.channels, H, H), 1, 100))
    cond = torch.from_numpy(rng.uniform((B, cfg.cond_in_channels, H, H), 1, 101, 0.0, 2.0))
    return x, cond, torch.full((B,), 5, dtype=torch.long)


def _launches(plan):
    return [m["what"] for _, m in sorted(plan.meta.items())]


@pytest.mark.parametrize("heads", [2, 8])
def test_unet_forward_fp32_matches_the_oracle(heads):
    """mnist28 of test_hip_unet.CASES with attn_heads = 2 and 8 against the oracle with the tap table, that file's limits."""
    kw, B, H = CASES["mnist28"]
    net, sd = build(dict(kw, attn_heads=heads), "fp32")
    assert net.cfg.hidden == 32 * heads
    x, cond, tv = _inputs(net.cfg, B, H)
    y = net(x.cuda(), cond.cuda(), tv.cuda()).cpu()
    taps = {}
    with torch.no_grad():
        y_ref = unet_ref.unet_forward(sd, net.cfg, x, cond, tv, taps)
    rows = tap_table(net, net.plan(B, H, H), taps)
    report = "\n".join(f"  {n:24s} err {e:.3e}  (ref max {m:.3e})" for n, e, m in rows)
    worst = max(e / max(m, 1e-6) for _, e, m in rows)
    err = float((y - y_ref).abs().max())
    print(f"mnist28 heads={heads}: out err {err:.3e}; worst tap rel {worst:.3e}\n{report}")
    assert {"downs.0.2", "downs.1.2", "downs.2.2", "mid_attn", "ups.0.2", "ups.2.2"} <= {n for n, _, _ in rows}   # every kind of attention block
    assert worst < 1e-4, report
    assert err < 2e-4


@pytest.mark.parametrize("dtype,tol", [("bf16", 5e-2), ("fp16", 8e-3)])
@pytest.mark.parametrize("heads", [2, 8])
def test_unet_forward_16bit_takes_the_unfused_route(heads, dtype, tol):
    """16-bit storage with attn_heads != 4: no fused-path weights are packed, the plan's launches hold linattn_ctx and
    neither linattn_kvctx nor linattn_out, and the output is within test_hip_unet's 5e-2 / 8e-3 of the oracle's."""
    kw, B, H = CASES["mnist28"]
    net, sd = build(dict(kw, attn_heads=heads), dtype)
    x, cond, tv = _inputs(net.cfg, B, H)
    y = net(x.cuda(), cond.cuda(), tv.cuda()).cpu()
    packed = net.packed()
    assert packed["wq"] == {} and packed["wkv"] == {} and packed["kshift"] == {} and packed["qshift"] == {} and "attn_terms" not in packed
    names = _launches(net.plan(B, H, H))
    assert "linattn_ctx" in names and "linattn_ctxfold" in names and "attention" in names
    assert not any(n in ("linattn_kvctx", "linattn_out") for n in names), names
    with torch.no_grad():
        y_ref = unet_ref.unet_forward(sd, net.cfg, x, cond, tv)
    rel = float((y - y_ref).abs().max()) / float(y_ref.abs().max())
    print(f"mnist28 heads={heads} {dtype}: out rel err {rel:.3e}")
    assert bool(torch.isfinite(y).all()) and rel < tol


@pytest.mark.parametrize("dtype", LOWP)
def test_four_heads_still_take_the_fused_route(dtype):
    kw, B, H = CASES["mnist28"]
    net, _ = build(kw, dtype)
    x, cond, tv = _inputs(net.cfg, B, H)
    net(x.cuda(), cond.cuda(), tv.cuda())
    names = _launches(net.plan(B, H, H))
    nlin = sum(1 for k in net.state_dict() if k.endswith(".to_out.1.g"))
    assert nlin > 0 and names.count("linattn_kvctx") == nlin and names.count("linattn_out") == nlin and "linattn_ctx" not in names
    assert len(net.packed()["wq"]) == nlin
