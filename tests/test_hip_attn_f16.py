"""GPU tests of ``amp_attn="fp16"``: the two attention cores on the fp16 matrix cores (the ``<f16>`` instantiations of
csrc/linattn16.hip and csrc/attention16.hip, ``ld_dn_la_*_f16`` and ``ld_dn_fa_*_f16``).  The six entry points on the exact
probes of tests/attn_f16_ref.py (proved on the CPU by tests/test_attn_f16.py) and on uniform operands, where each output is
held to max(1e-5, 2 d) of the fp64 value of the UNROUNDED operands, d being the distance of the CPU restatement of the fp16
contract from that value; what leaves fp16's range; the fp32 and bf16 siblings' bits; then ``LinearAttention``,
``Attention`` and ``DenoiserTrainer`` with the option.  Every output buffer holds NaN before a launch, and so does the padding
of qkv, out and dout, which is never read; the padding of every output must come out zero.

The distance of two tensors is ``rel_err``: max |difference| / max |reference|."""
import functools
import math

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd.denoiser_train import EmulatedRank

from hip_helpers import DEV, NAN, nans, pad64, padded, st
import attention_ref as RF
import attn_f16_ref as P
import denoiser_train_ref as T
import linattn_ref as RL
import unet_grad_ref as UR
from amp_ref import h
from attention16_ref import core16 as fa_core16
from conv16_ref import _same

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
LA_NAMES = ("context", "out", "backward_reduce", "backward_apply")
rel_err = RL.rel_err


def ratio(e, d):
    return e / d if d else float("inf")


# ------------------------------------------------------------------------------------------------ the entry points
def la_passes(qkv, dout, heads, given=None, suffix="_f16"):
    """The linear core's four entry points ``ld_dn_la_<name><suffix>`` on qkv [B, 3 hidden, H, W] and dout [B, hidden, H, W]
    (cpu).  With ``given`` (ctx, m, Z, dctx, rk: fp32 cpu tensors) every later pass reads those instead of the results of
    the passes before it.  Returns cpu tensors: ctx, kstat, out, dctx, rk, dqkv (NHWC, padded)."""
    lib = cabi.lib()
    B, _, H, W = qkv.shape
    hidden = 32 * heads
    ld3, ldo = pad64(3 * hidden), pad64(hidden)
    qp, dop = padded(qkv, ld3), padded(dout, ldo)
    f = {n: getattr(lib, f"ld_dn_la_{n}{suffix}") for n in LA_NAMES}

    def work():
        nbytes = int(lib.ld_dn_la_work_bytes(B, heads, H, W))
        assert nbytes > 0
        return nans(nbytes // 8, dtype=F64)

    ctx, kstat, out = nans(B, heads, 32, 32), nans(B, heads, 32, 2), nans(B, H, W, ldo)
    cabi.check(f["context"](qp.data_ptr(), work().data_ptr(), ctx.data_ptr(), kstat.data_ptr(), B, H, W, heads, ld3, st()),
               "dn_la_context" + suffix)
    ctx_in, kstat_in = ctx, kstat
    if given is not None:
        ctx_in = given["ctx"].to(DEV).contiguous()
        kstat_in = torch.stack([given["m"], given["Z"]], dim=-1).to(DEV).contiguous()
    cabi.check(f["out"](qp.data_ptr(), ctx_in.data_ptr(), out.data_ptr(), B, H, W, heads, ld3, ldo, st()), "dn_la_out" + suffix)
    dctx, rk, dqkv = nans(B, heads, 32, 32), nans(B, heads, 32), nans(B, H, W, ld3)
    cabi.check(f["backward_reduce"](qp.data_ptr(), dop.data_ptr(), ctx_in.data_ptr(), work().data_ptr(), dctx.data_ptr(),
                                    rk.data_ptr(), B, H, W, heads, ld3, ldo, st()), "dn_la_backward_reduce" + suffix)
    dctx_in, rk_in = dctx, rk
    if given is not None:
        dctx_in, rk_in = given["dctx"].to(DEV).contiguous(), given["rk"].to(DEV).contiguous()
    cabi.check(f["backward_apply"](qp.data_ptr(), dop.data_ptr(), ctx_in.data_ptr(), kstat_in.data_ptr(), dctx_in.data_ptr(),
                                   rk_in.data_ptr(), dqkv.data_ptr(), B, H, W, heads, ld3, ldo, st()),
               "dn_la_backward_apply" + suffix)
    torch.cuda.synchronize()
    return dict(ctx=ctx.cpu(), kstat=kstat.cpu(), out=out.cpu(), dctx=dctx.cpu(), rk=rk.cpu(), dqkv=dqkv.cpu())


def nchw(t, c):
    return t[..., :c].permute(0, 3, 1, 2).contiguous()


def thirds(dqkv, heads):
    """dq, dk, dv [B, heads, 32, n] of a [B, H, W, ld3] tensor, whose padding must be zero."""
    B, H, W, _ = dqkv.shape
    hidden = 32 * heads
    assert bool((dqkv[..., 3 * hidden:] == 0).all())
    return [nchw(dqkv[..., i * hidden:(i + 1) * hidden], hidden).reshape(B, heads, 32, H * W) for i in range(3)]


def la_outputs(hip, heads):
    """ctx, out [B, hidden, H, W], dctx, dq, dk, dv of ``la_passes``' result; the padding of out and dqkv must be zero."""
    hidden = 32 * heads
    assert bool((hip["out"][..., hidden:] == 0).all())
    dq, dk, dv = thirds(hip["dqkv"], heads)
    return dict(ctx=hip["ctx"], out=nchw(hip["out"], hidden), dctx=hip["dctx"], dq=dq, dk=dk, dv=dv)


def fa_passes(qkv, dout, heads, suffix="_f16", given=None, quiet=False):
    """The full core's forward (with lse; ``quiet``: once more without) and, with ``dout``, its backward -- on the forward's
    own lse and out, or on ``given``'s -- through ``ld_dn_fa_*<suffix>``; cpu tensors: out [B, H, W, ldo], lse, dqkv."""
    B, _, H, W = qkv.shape
    hidden, n = 32 * heads, H * W
    lib = cabi.lib()
    fwd, bwd = getattr(lib, "ld_dn_fa_forward" + suffix), getattr(lib, "ld_dn_fa_backward" + suffix)
    ld3, ldo = pad64(3 * hidden), pad64(hidden)
    qp = padded(qkv, ld3)
    out, lse = nans(B, H, W, ldo), nans(B, heads, n)
    cabi.check(fwd(qp.data_ptr(), out.data_ptr(), lse.data_ptr(), B, H, W, heads, ld3, ldo, st()), "dn_fa_forward" + suffix)
    res = dict(out=out, lse=lse)
    if quiet:
        res["quiet"] = nans(B, H, W, ldo)
        cabi.check(fwd(qp.data_ptr(), res["quiet"].data_ptr(), None, B, H, W, heads, ld3, ldo, st()), "dn_fa_forward" + suffix)
    if dout is not None:
        dop, dqkv = padded(dout, ldo), nans(B, H, W, ld3)
        nbytes = int(lib.ld_dn_fa_work_bytes(B, heads, H, W))
        assert nbytes >= 4 * B * heads * n
        work = nans(nbytes // 8, dtype=F64)
        if given is None:
            opad, ls = out.clone(), lse
            opad[..., hidden:] = NAN                     # the backward may not read out's padding either
        else:
            opad, ls = padded(given["out"], ldo), given["lse"].to(DEV).contiguous()
        cabi.check(bwd(qp.data_ptr(), opad.data_ptr(), dop.data_ptr(), ls.data_ptr(), work.data_ptr(), dqkv.data_ptr(), B, H, W,
                       heads, ld3, ldo, st()), "dn_fa_backward" + suffix)
        res["dqkv"] = dqkv
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def within(got, want, name):
    """Element by element within 2^-21 relative of the fp64 value: one trailing fp32 multiplication."""
    bad = (got.double() - want).abs() > 2.0 ** -21 * want.abs()
    assert not bool(bad.any()), (name, int(bad.sum()), float((got.double() - want).abs().max()))


# ------------------------------------------------------------------------------------------------ 1. exact probes
@pytest.mark.parametrize("shape", P.LA_PROBE_SHAPES)
@pytest.mark.parametrize("kind", P.LA_PROBE_KINDS)
def test_linear_core_exact_probes(shape, kind):
    """k constant per channel, q constant per pixel, ``fp16_ties`` in the four rounded memory operands in turn.  ctx, dctx and
    (m, Z) = (c, n), integer sums through the merge's fp64 arithmetic, bit for bit; out / dq / dk, behind one trailing fp32
    multiplication, within 2^-21 relative element by element.  dv = sum_d fp16(dctx[d][e] / n): where n is a power of two
    (8 x 8, 16 x 32) an integer sum over n, bit for bit; elsewhere within the probe's ``dv_bound``.  rk by
    ``reduction_bound``."""
    pr = P.la_probe(shape, kind)
    hip = la_passes(pr.qkv, pr.dout, pr.heads, pr.given)
    w = pr.want
    assert torch.equal(hip["kstat"], w.kstat), "kstat"
    assert torch.equal(hip["ctx"], w.ctx), float((hip["ctx"] - w.ctx).abs().max())
    assert torch.equal(hip["dctx"], w.dctx), float((hip["dctx"] - w.dctx).abs().max())
    got = la_outputs(hip, pr.heads)
    for name in ("out", "dq", "dk"):
        within(got[name], getattr(w, name), name)
    err = (got["dv"].double() - w.dv).abs()
    if w.dv_exact:
        assert torch.equal(got["dv"].double(), w.dv), float(err.max())
    else:
        worst = float((err / w.dv_bound.clamp_min(1e-300)).max())
        print(f"probe {shape} {kind} dv: largest error / bound {worst:.3f}")
        assert bool((err <= w.dv_bound).all()), worst
    RL.reduction_bound(hip["rk"], w.rk64, w.rk32, f"probe {shape} {kind} rk")


@pytest.mark.parametrize("shape", P.FA_PROBE_SHAPES)
@pytest.mark.parametrize("kind", P.FA_FORWARD_KINDS)
def test_full_core_exact_forward_probes(shape, kind):
    """k constant over the keys: p = 1, l = n, out = mean_j(fp16(v_j)) within 2^-21 relative element by element (the one
    multiplication by 1 / n), lse = a + log n within 2^-21 max(1, |lse|); the padding zero; the lse-less forward gives the
    same bits."""
    B, heads, H, W = shape
    pr = P.fa_forward_probe(shape, kind)
    hip = fa_passes(pr.qkv, None, heads, quiet=True)
    hidden = 32 * heads
    within(nchw(hip["out"], hidden), pr.want.out, "out")
    err = (hip["lse"].double() - pr.want.lse).abs()
    assert bool((err <= 2.0 ** -21 * pr.want.lse.abs().clamp_min(1.0)).all()), float(err.max())
    assert bool((hip["out"][..., hidden:] == 0).all()) and torch.equal(hip["out"], hip["quiet"])


@pytest.mark.parametrize("shape", P.FA_PROBE_SHAPES)
@pytest.mark.parametrize("kind", P.FA_BACKWARD_KINDS)
def test_full_core_exact_backward_probes(shape, kind):
    """lse_i = the fp32 logit of row i and out = 0 are fed: p = 1, delta = 0, ds = dP an integer.  dv, a sum of integers, bit
    for bit; dq and dk within 2^-21 relative element by element (the one trailing 32^-0.5); the padding of dqkv zero."""
    B, heads, H, W = shape
    pr = P.fa_backward_probe(shape, kind)
    hip = fa_passes(pr.qkv, pr.dout, heads, given=pr.given)
    dq, dk, dv = thirds(hip["dqkv"], heads)
    assert torch.equal(dv.double(), pr.want.dv)
    within(dq, pr.want.dq, "dq")
    within(dk, pr.want.dk, "dk")


# ------------------------------------------------------------------------------------------------ 2. random operands
@functools.lru_cache(maxsize=None)
def la_case(B, heads, H, W, shifted):
    """tests/test_hip_linattn16.py's operands; the given ctx / (m, Z) / dctx / rk are the fp64 values cast to fp32, so every
    pass is measured by itself.  The fp64 value of the unrounded operands, the restatement of the fp16 contract and the one
    that rounds ks instead of folding.  (Computed once, never changed.)"""
    hidden, n = 32 * heads, H * W
    key = 1000 * heads + 10 * H + W
    qkv = RL.uniform((B, 3 * hidden, H, W), key, -2.0, 2.0)
    if shifted:
        qkv.reshape(B, 3 * hidden, n)[:, hidden:2 * hidden, n - n // 4:] += 100.0
    dout = RL.uniform((B, hidden, H, W), key + 1)
    first = P.la_core(qkv, heads, dout, None, F64, _same)
    given = dict(ctx=first.ctx.float(), m=first.m.float(), Z=first.Z.float(), dctx=first.dctx.float(), rk=first.rk.float())
    ref = P.la_core(qkv, heads, dout, given, F64, _same)
    rest = P.la_core(qkv, heads, dout, given, F64, h)
    rounds_ks = P.la_core(qkv, heads, dout, given, F64, h, fold=False)
    return qkv, dout, given, ref, rest, rounds_ks, la_passes(qkv, dout, heads, given)


def la_values(r, heads):
    return dict(ctx=r.ctx, out=r.out, dctx=r.dctx, dq=r.dq, dk=r.dk, dv=r.dv)


@pytest.mark.parametrize("B,heads,H,W,shifted", P.LA_CORE_CASES + [P.LA_SUBNORMAL_CASE + (False,)])
def test_linear_core_random_operands(B, heads, H, W, shifted):
    """Each pass on given inputs.  For each of ctx, out, dctx, dq, dk, dv: e <= max(1e-5, 2 d), e the distance of HIP from the
    fp64 value of the unrounded operands and d that of the fp16 restatement (fp64 around the rounded operands) from the same
    value; the factor covers computed operands that round the other way on the device and the order of the sums.  m is
    exact, Z is the fp32 path's.  At 128 x 128, where ks = exp(k - m) / Z reaches fp16's subnormals, HIP's dv is also closer
    to the unrounded value than the restatement that rounds ks: the fold, seen on the device.  e, d and e / d are printed; on
    an MI355X e / d was 0.87 ... 1.00 for ctx and 1.00 for the other five (e 1.1e-4 ... 6.0e-4), and dv at 128 x 128 2.00e-4
    against 2.16e-4."""
    qkv, dout, given, ref, rest, rounds_ks, hip = la_case(B, heads, H, W, shifted)
    tag = f"la f16 B{B} h{heads} {H}x{W}{' shifted' if shifted else ''}"
    for v in hip.values():
        assert bool(torch.isfinite(v).all())
    assert torch.equal(hip["kstat"][..., 0].double(), ref.m)
    RL.reduction_bound(hip["kstat"][..., 1], ref.Z, RL.core(qkv, heads, None, F32)["Z"], tag + " Z")
    got, want, restated = la_outputs(hip, heads), la_values(ref, heads), la_values(rest, heads)
    for name in ("ctx", "out", "dctx", "dq", "dk", "dv"):
        e, d = rel_err(got[name].double(), want[name]), rel_err(restated[name], want[name])
        print(f"{tag} {name}: HIP {e:.2e}, restatement {d:.2e}, ratio {ratio(e, d):.2f}")
        assert e <= max(1e-5, 2 * d), (name, e, d)
    if (B, heads, H, W) == P.LA_SUBNORMAL_CASE:
        e, unfolded = rel_err(got["dv"].double(), want["dv"]), rel_err(rounds_ks.dv, want["dv"])
        print(f"{tag} dv: HIP {e:.2e}, the restatement that rounds ks {unfolded:.2e} (ratio {ratio(unfolded, e):.2f})")
        assert e < unfolded


@functools.lru_cache(maxsize=None)
def fa_case(B, heads, H, W, scaled):
    """tests/test_hip_attention16.py's operands, the fp16 entry points' results, the fp64 value of the unrounded operands
    and the restatement of the fp16 contract in fp64 (computed once, never changed)."""
    hidden, n = 32 * heads, H * W
    key = 1000 * heads + 10 * H + W
    qkv = RF.uniform((B, 3 * hidden, H, W), key, -2.0, 2.0)
    if scaled:                                           # logits reach +-121 in the last quarter of the keys
        qkv.reshape(B, 3 * hidden, n)[:, hidden:2 * hidden, n - n // 4:] *= 20.0
    dout = RF.uniform((B, hidden, H, W), key + 1)
    return qkv, dout, fa_passes(qkv, dout, heads, quiet=True), RF.core(qkv, heads, dout, F64), fa_core16(qkv, heads, dout, None, F64, h)


def fa_values(core, heads):
    """out, lse, dq, dk, dv of a reference (the oracle's dict or ``core16``'s namespace)."""
    if isinstance(core, dict):
        hidden = 32 * heads
        return dict(out=core["out"], lse=core["lse"], **{"d" + c: core["dqkv"][:, i * hidden:(i + 1) * hidden] for i, c in enumerate("qkv")})
    hs = core.out.shape
    return dict(out=core.out, lse=core.lse, dq=core.dq.reshape(hs), dk=core.dk.reshape(hs), dv=core.dv.reshape(hs))


def fa_got(hip, heads):
    B, H, W, _ = hip["out"].shape
    hidden = 32 * heads
    assert bool((hip["out"][..., hidden:] == 0).all())
    dq, dk, dv = (t.reshape(B, hidden, H, W) for t in thirds(hip["dqkv"], heads))
    return dict(out=nchw(hip["out"], hidden), lse=hip["lse"], dq=dq, dk=dk, dv=dv)


@pytest.mark.parametrize("B,heads,H,W,scaled", P.FA_CORE_CASES)
def test_full_core_random_operands(B, heads, H, W, scaled):
    """For each of out, lse, dq, dk, dv: e <= max(1e-5, 2 d) as above (the scaled case reaches logits of +-121).  Everything is
    finite, the padding is zero, the lse-less forward gives the same bits.  e, d and e / d are printed; on an MI355X e / d was
    0.97 ... 1.03 (e 3.4e-5 ... 2.0e-3; dq 6.2e-3 in the scaled case, where d is the same).  At a single pixel dq and dk are
    exactly zero in the reference, HIP and the restatement alike."""
    qkv, dout, hip, ref, rest = fa_case(B, heads, H, W, scaled)
    tag = f"fa f16 B{B} h{heads} {H}x{W}{' k x20' if scaled else ''}"
    for k, v in hip.items():
        assert bool(torch.isfinite(v).all()), k
    assert torch.equal(hip["out"], hip["quiet"])
    got, want, restated = fa_got(hip, heads), fa_values(ref, heads), fa_values(rest, heads)
    for name in ("out", "lse", "dq", "dk", "dv"):
        e, d = rel_err(got[name].double(), want[name]), rel_err(restated[name], want[name])
        print(f"{tag} {name}: HIP {e:.2e}, restatement {d:.2e}, ratio {ratio(e, d):.2f}")
        assert e <= max(1e-5, 2 * d), (name, e, d)


# ------------------------------------------------------------------------------------------------ 3. range
def per_head(name, t, heads):
    """[B, heads, ...] view of a result: the per-head statistics as they are, the NHWC tensors out and dqkv split by head
    (the padding dropped)."""
    if name not in ("out", "dqkv"):
        return t
    B, H, W, _ = t.shape
    parts = 3 if name == "dqkv" else 1
    return t[..., :parts * 32 * heads].reshape(B, H * W, parts, heads, 32).permute(0, 3, 1, 2, 4)


def check_range(clean, planted, heads, b, hd, reads_v):
    """``planted``: the results with one 1e5 in v of (sample b, head hd).  Every output that reads v is non-finite there;
    every (sample, head) but that one is finite and has ``clean``'s bits."""
    for name in clean:
        a, p = per_head(name, clean[name], heads), per_head(name, planted[name], heads)
        hit = torch.zeros(a.shape[:2], dtype=torch.bool)
        hit[b, hd] = True
        assert bool(torch.isfinite(p[~hit]).all()), name
        assert torch.equal(a[~hit], p[~hit]), name
        if name in reads_v:
            assert not bool(torch.isfinite(p[hit]).all()), name
    if planted["dqkv"].shape[-1] > 96 * heads:
        assert bool((planted["dqkv"][..., 96 * heads:] == 0).all())
    assert bool((planted["out"][..., 32 * heads:] == 0).all())


def test_linear_core_beyond_fp16s_range():
    """One 1e5 in v (beyond 65504: fp16 rounds it to inf, there is no saturation) of one (sample, head) of the 14 x 14 case:
    what reads v there -- ctx, out, rk, dq and dk, each pass on the results of the one before -- is not finite; dctx, (m, Z)
    and dv do not read v.  Every other (sample, head) is finite and keeps its bits, and the padding stays zero."""
    B, heads, H, W, _ = P.LA_CORE_CASES[1]
    qkv, dout = la_case(B, heads, H, W, False)[:2]
    b, hd = 1, 2
    bad = qkv.clone()
    bad[b, 64 * heads + 32 * hd + 5, 3, 4] = 1e5
    clean, planted = la_passes(qkv, dout, heads), la_passes(bad, dout, heads)
    assert all(bool(torch.isfinite(v).all()) for v in clean.values())
    check_range(clean, planted, heads, b, hd, reads_v=("ctx", "out", "rk", "dqkv"))
    dq, dk, dv = thirds(planted["dqkv"], heads)
    assert not bool(torch.isfinite(dq[b, hd]).all()) and not bool(torch.isfinite(dk[b, hd]).all())
    assert bool(torch.isfinite(dv).all()) and bool(torch.isfinite(planted["dctx"]).all())


def test_full_core_beyond_fp16s_range():
    """The same plant in the full core's 14 x 14 case: out, dq and dk of that (sample, head) are not finite (lse reads q and k
    only, dv reads p and dO), every other (sample, head) is finite and keeps its bits."""
    B, heads, H, W, _ = P.FA_CORE_CASES[3]
    qkv, dout = fa_case(B, heads, H, W, False)[:2]
    b, hd = 1, 2
    bad = qkv.clone()
    bad[b, 64 * heads + 32 * hd + 5, 3, 4] = 1e5
    clean, planted = fa_passes(qkv, dout, heads), fa_passes(bad, dout, heads)
    assert all(bool(torch.isfinite(v).all()) for v in clean.values())
    check_range(clean, planted, heads, b, hd, reads_v=("out", "dqkv"))
    dq, dk, dv = thirds(planted["dqkv"], heads)
    assert not bool(torch.isfinite(dq[b, hd]).all()) and not bool(torch.isfinite(dk[b, hd]).all())
    assert bool(torch.isfinite(dv).all()) and bool(torch.isfinite(planted["lse"]).all())


# ------------------------------------------------------------------------------------------------ 4. the siblings
def test_the_linear_siblings_keep_their_bits():
    """The same operands through the fp32 and the bf16 entry points, before and after the fp16 ones ran: the same bits; the
    fp16 results are neither's (m is every path's)."""
    B, heads, H, W, _ = P.LA_CORE_CASES[1]
    qkv, dout, given, _, _, _, hip = la_case(B, heads, H, W, False)
    before = {s: la_passes(qkv, dout, heads, given, suffix=s) for s in ("", "16")}
    again = la_passes(qkv, dout, heads, given)
    after = {s: la_passes(qkv, dout, heads, given, suffix=s) for s in ("", "16")}
    for s in before:
        for k in before[s]:
            assert torch.equal(before[s][k], after[s][k]), (s, k)
        for k in ("ctx", "out", "dctx", "dqkv"):
            assert not torch.equal(before[s][k], hip[k]), (s, k)
        assert torch.equal(before[s]["kstat"][..., 0], hip["kstat"][..., 0])
    for k in hip:
        assert torch.equal(again[k], hip[k]), k


def test_the_full_siblings_keep_their_bits():
    B, heads, H, W, _ = P.FA_CORE_CASES[3]
    qkv, dout, hip = fa_case(B, heads, H, W, False)[:3]
    before = {s: fa_passes(qkv, dout, heads, suffix=s) for s in ("", "16")}
    again = fa_passes(qkv, dout, heads)
    after = {s: fa_passes(qkv, dout, heads, suffix=s) for s in ("", "16")}
    for s in before:
        for k in before[s]:
            assert torch.equal(before[s][k], after[s][k]), (s, k)
            assert not torch.equal(before[s][k], hip[k]), (s, k)
    for k in again:
        assert torch.equal(again[k], hip[k]), k


# ------------------------------------------------------------------------------------------------ 5. the modules
def hip_module(cls, dim, heads, sd, **kw):
    mod = cls(dim, heads=heads)
    mod.load_state_dict(sd)
    for k, v in kw.items():
        setattr(mod, k, v)
    return mod.to(DEV)


def forward_backward(mod, x, dout):
    xd = x.to(DEV).requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    out = mod(xd)
    out.backward(dout.to(DEV))
    grads = {"x": xd.grad.cpu()}
    grads.update({k: p.grad.cpu() for k, p in mod.named_parameters() if p.grad is not None})
    return out.detach().cpu(), grads


def check_module(cls, R, yardstick_f16, bf16_switch, keys, B, dim, heads, H, W):
    sd = R.make_attn(dim, heads, key=dim + heads)
    x = R.uniform((B, dim, H, W), keys[0] * dim + H)
    dout = R.uniform((B, dim, H, W), keys[1] * dim + H) / (B * H * W)
    out32, g32 = forward_backward(hip_module(cls, dim, heads, sd), x, dout)
    mod = hip_module(cls, dim, heads, sd, amp_attn="fp16")
    out, grads = forward_backward(mod, x, dout)
    o64, g64 = R.yardstick(sd, x, dout, heads, dtype=F64)
    o16, g16 = yardstick_f16(sd, x, dout, heads, F64)
    tag = f"{cls.__name__} amp_attn B{B} dim{dim} h{heads} {H}x{W}"
    assert set(grads) == set(g64)
    for name, got, want, restated in [("out", out, o64, o16)] + [("d " + k, grads[k], g64[k], g16[k]) for k in g64]:
        e, d = rel_err(got.double(), want), rel_err(restated, want)
        print(f"{tag} {name}: HIP {e:.2e}, restatement {d:.2e}, ratio {ratio(e, d):.2f}")
        assert e <= max(1e-5, 2 * d), (name, e, d)
    assert not torch.equal(out, out32) and not torch.equal(grads["to_qkv.weight"], g32["to_qkv.weight"])
    mod.debug_fill = NAN
    out2, grads2 = forward_backward(mod, x, dout)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    mod.amp_attn = "fp32"
    out3, grads3 = forward_backward(mod, x, dout)
    assert torch.equal(out3, out32) and all(torch.equal(grads3[k], g32[k]) for k in g32)
    # the format's advantage, as an ordering only: the bf16 module is further from the fp64 yardstick
    setattr(mod, bf16_switch, "bf16")
    outb, gb = forward_backward(mod, x, dout)
    e16, eb = rel_err(out.double(), o64), rel_err(outb.double(), o64)
    print(f"{tag} out: fp16 {e16:.2e}, bf16 {eb:.2e}, bf16 / fp16 {ratio(eb, e16):.2f}")
    for k in g64:
        print(f"{tag} d {k}: bf16 / fp16 {ratio(rel_err(gb[k].double(), g64[k]), rel_err(grads[k].double(), g64[k])):.2f}")
    assert e16 < eb


@pytest.mark.parametrize("B,dim,heads,H,W", P.LA_MODULE_CASES)
def test_linear_attention_at_amp_attn(B, dim, heads, H, W):
    """``LinearAttention`` at ``amp_attn="fp16"``: the output and all six gradients within max(1e-5, 2 d) of the fp64 yardstick
    of the unrounded module, d = the distance of the module restated on ``LaCore``; reproducible with NaN-filled buffers;
    not the fp32 module's result, and setting the attribute back restores the fp32 bits; the output is closer to the
    yardstick than at ``attn_precision="bf16"`` (the ratios are printed, only the ordering is asserted; on an MI355X the
    output was 4.7 ... 8.8 times closer, and e / d 0.82 ... 1.17)."""
    check_module(ldh.LinearAttention, RL, P.la_yardstick, "attn_precision", (11, 17), B, dim, heads, H, W)


@pytest.mark.parametrize("B,dim,heads,H,W", P.FA_MODULE_CASES)
def test_attention_at_amp_attn(B, dim, heads, H, W):
    """``Attention`` at ``amp_attn="fp16"``: the same, against the module restated on ``FaCore`` and
    ``full_attn_precision="bf16"`` (on an MI355X the output was 6.5 ... 12.1 times closer, and e / d at most 1.20; ``to_out.bias`` does not pass the core: d = 0, e under the floor)."""
    check_module(ldh.Attention, RF, P.fa_yardstick, "full_attn_precision", (13, 19), B, dim, heads, H, W)


@pytest.mark.parametrize("cls,R,case", [(ldh.LinearAttention, RL, P.LA_MODULE_CASES[1]), (ldh.Attention, RF, P.FA_MODULE_CASES[2])])
def test_a_module_composes_with_amp(cls, R, case):
    """``amp_attn="fp16"`` and ``amp="fp16"`` on one module: bit-identical across two runs (the second with NaN-filled
    buffers), finite, and the result of neither alone."""
    B, dim, heads, H, W = case
    sd = R.make_attn(dim, heads, key=dim + heads)
    x = R.uniform((B, dim, H, W), 13 * dim + H)
    dout = R.uniform((B, dim, H, W), 19 * dim + H) / (B * H * W)
    mod = hip_module(cls, dim, heads, sd, amp_attn="fp16", amp="fp16")
    out, grads = forward_backward(mod, x, dout)
    mod.debug_fill = NAN
    out2, grads2 = forward_backward(mod, x, dout)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    for alone in (dict(amp_attn="fp16"), dict(amp="fp16")):
        o, g = forward_backward(hip_module(cls, dim, heads, sd, **alone), x, dout)
        assert not torch.equal(o, out) and not torch.equal(g["x"], grads["x"]), alone
    o64, _ = R.yardstick(sd, x, dout, heads, dtype=F64)
    e = rel_err(out.double(), o64)
    print(f"{cls.__name__} amp_attn with amp: out {e:.2e} from the fp64 yardstick")
    assert e < 8e-3                                            # (fp16's unit roundoff 2^-11 on a handful of stages)


# ------------------------------------------------------------------------------------------------ 6. the trainer
OPTS = dict(branch_out=False, start_intermediate=False, start_timestep=2, mask_x=False, ood_AD=False, ood_confidence=False,
            classifier=False, use_gt=False, data="mnist")
TIMESTEPS = 250
CASE = UR.CASES[1]                                          # mnist, 2 x 1 x 12 x 12
ON = dict(amp=True, amp_attn="fp16")


def make_trainer(**kw):
    inf = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **UR.KWARGS["mnist"])
    inf.load_state_dict(UR.state("mnist"))
    gd = ldh.GaussianDiffusion(OPTS, inf, image_size=12, timesteps=TIMESTEPS, objective="pred_v").to(DEV)
    return ldh.DenoiserTrainer(gd, train_lr=1e-3, **kw)


def batch(j=0, step=0):
    return tuple(v.to(DEV) for v in T.batch(CASE, step, j, TIMESTEPS))


def flat_grad(tr):
    return torch.cat([p.grad.reshape(-1) for k, p in tr.online_model.named_parameters() if p.grad is not None]).clone()


def flat_params(tr):
    return torch.cat([p.detach().reshape(-1) for p in tr.online_model.parameters()]).clone()


def one_step(fill=None, **kw):
    tr = make_trainer(**kw)
    if fill is not None:
        tr.online_model.debug_fill = fill
    hr, lr, t, noise = batch()
    loss = tr.accumulate(hr, lr, t=t, noise=noise)
    grad = flat_grad(tr)
    tr.apply()
    return tr, (loss.clone(), grad, flat_params(tr))


def attention_modules(tr):
    mods = list(tr.online_model.modules())
    return [m for m in mods if isinstance(m, ldh.LinearAttention)], [m for m in mods if isinstance(m, ldh.Attention)]


def test_trainer_with_amp_attn_is_reproducible():
    """Two trainers with ``amp=True, amp_attn="fp16"``, one with NaN-filled buffers: the same loss, flat (scaled) gradient and
    parameters after a step, bit for bit, finite, and the step was not skipped.  All 4 ``LinearAttention`` and all 3
    ``Attention`` modules carry the value.  The gradient is not ``amp=True``'s alone, and the loss differs from that one's by
    less than the 2e-2 relative that the bf16 attention tests allow (printed)."""
    seen = []
    for fill in (None, NAN):
        tr, state = one_step(fill, **ON)
        assert tr.amp_attn == "fp16" and tr.online_model.amp_attn == "fp16" and tr.online_model.amp == "fp16"
        lin, full = attention_modules(tr)
        assert len(lin) == 4 and len(full) == 3 and all(m.amp_attn == "fp16" for m in lin + full)
        assert tr.attn_precision == "fp32" and tr.full_attn_precision == "fp32"
        assert all(bool(torch.isfinite(v).all()) for v in state) and bool(state[1].any())
        s = tr.scaler_state()
        assert (s["adam_steps"], s["skipped_steps"]) == (1, 0)
        seen.append(state)
    for a, b in zip(*seen):
        assert torch.equal(a, b)
    _, base = one_step(amp=True)
    assert not torch.equal(base[1], seen[0][1])
    rel = abs(float(base[0]) - float(seen[0][0])) / float(base[0])
    print(f"amp_attn trainer: loss {float(seen[0][0]):.6f}, amp alone {float(base[0]):.6f} (rel {rel:.2e})")
    assert rel < 2e-2


class Watched:
    """``cabi.lib()`` with the names of the attention cores' entry points it hands out recorded."""

    def __init__(self, real, seen):
        self.real, self.seen = real, seen

    def __getattr__(self, name):
        if name.startswith(("ld_dn_la_", "ld_dn_fa_")) and not name.endswith("work_bytes"):
            self.seen.append(name)
        return getattr(self.real, name)


def core_calls(tr):
    real, seen = cabi.lib, []
    cabi.lib = lambda: Watched(real(), seen)
    try:
        hr, lr, t, noise = batch()
        loss = tr.accumulate(hr, lr, t=t, noise=noise)
        grad = flat_grad(tr)
        tr.apply()
    finally:
        cabi.lib = real
    return set(seen), (loss.clone(), grad, flat_params(tr))


def test_only_the_f16_entry_points_run_with_the_option_and_none_without():
    """With the option every attention-core entry point a step calls is an ``_f16`` one, all six of them; with ``amp=True``
    alone none is, and ``amp_attn="fp32"`` spelled out is that trainer bit for bit, with no module told about the
    attribute."""
    f16 = {f"ld_dn_la_{n}_f16" for n in LA_NAMES} | {"ld_dn_fa_forward_f16", "ld_dn_fa_backward_f16"}
    seen, _ = core_calls(make_trainer(**ON))
    assert seen == f16, seen
    plain = {n[:-4] for n in f16}
    seen, want = core_calls(make_trainer(amp=True))
    assert seen == plain, seen
    tr = make_trainer(amp=True, amp_attn="fp32")
    assert tr.amp_attn == "fp32" and not any("amp_attn" in vars(m) for m in tr.online_model.modules())
    seen, got = core_calls(tr)
    assert seen == plain and all(torch.equal(a, b) for a, b in zip(got, want))


def test_a_checkpoint_does_not_record_amp_attn(tmp_path):
    """``save`` writes the keys it wrote before and ``load`` takes the file into a trainer without the option."""
    tr, _ = one_step(**ON)
    path = str(tmp_path / "model-best1.pt")
    tr.save(path)
    data = torch.load(path, map_location="cpu", weights_only=True)
    assert set(data) == {"step", "model", "opt", "ema", "scaler"}
    assert not any("amp_attn" in str(k) for part in ("model", "ema") for k in data[part])
    other = make_trainer(amp=True)
    other.load(path)
    assert other.step == 1 and other.amp_attn == "fp32"


def test_two_emulated_ranks_stay_identical():
    """Two emulated data-parallel ranks with the option: equal ``replica_digest()``s after a step."""
    ranks = [make_trainer(comm=EmulatedRank(2, r), **ON) for r in range(2)]
    for r, tr in enumerate(ranks):
        hr, lr, t, noise = batch(r)
        tr.accumulate(hr, lr, scale=0.5, t=t, noise=noise)
    gathered = torch.stack([tr.send_buffer() for tr in ranks]).contiguous()
    for tr in ranks:
        tr.apply(gathered=gathered)
    a, b = (dict(tr.replica_digest()) for tr in ranks)
    assert a == b and a["step"] == 1
    assert torch.equal(flat_params(ranks[0]), flat_params(ranks[1]))


N_BACKOFF_STEPS = 20


def test_an_overflowing_init_scale_backs_off_and_then_trains():
    """From ``init_scale=2^30`` the scaled dO overflows fp16 in the attention cores (and the convolutions): at least the
    first step is skipped, the scale halves each time, then at least one step trains; the run ends finite with a scale
    below 2^30, and ``scaler_state()`` agrees with the count of skipped steps.  (On an MI355X the first 10 of the 20 steps
    were skipped and one more later: the scale ended at 2^19.)"""
    tr = make_trainer(scaler_kwargs=dict(init_scale=2.0 ** 30), **ON)
    tr.online_model.debug_fill = NAN
    skipped = []
    for step in range(N_BACKOFF_STEPS):
        hr, lr, t, noise = batch(0, step)
        tr.accumulate(hr, lr, t=t, noise=noise)
        tr.apply()
        skipped.append(bool(tr.scaler_state()["found_inf"]))
    s = tr.scaler_state()
    print(f"amp_attn from init_scale 2^30: skipped {sum(skipped)} of {N_BACKOFF_STEPS} steps (the first {skipped.index(False)}), "
          f"final scale 2^{math.log2(s['scale']):.0f}")
    assert skipped[0] and not all(skipped)
    assert s["skipped_steps"] == sum(skipped) >= 1 and s["adam_steps"] == N_BACKOFF_STEPS - sum(skipped) >= 1
    assert s["scale"] < 2.0 ** 30 and tr.step == N_BACKOFF_STEPS
    assert bool(torch.isfinite(flat_params(tr)).all())


def test_a_step_with_amp_attn_does_not_synchronise():
    """tests/test_hip_amp.py's method: after a warm-up step, ``accumulate`` and ``apply`` run under
    ``set_sync_debug_mode('error')``."""
    tr = make_trainer(**ON)
    hr, lr, t, noise = batch()
    tr.accumulate(hr, lr, t=t, noise=noise)
    tr.apply()
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        with pytest.raises(RuntimeError):
            probe.item()
        value = tr.accumulate(hr, lr, scale=0.5, t=t, noise=noise)       # raises if anything synchronises
        drawn = tr.accumulate(hr, lr, scale=0.5)
        tr.apply()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    s = tr.scaler_state()
    assert math.isfinite(float(value)) and math.isfinite(float(drawn)) and tr.step == 2 and s["adam_steps"] + s["skipped_steps"] == 2
