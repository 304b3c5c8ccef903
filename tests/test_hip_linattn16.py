"""GPU tests of LinearAttention's core on the bf16 matrix cores (``attn_precision="bf16"``, csrc/linattn16.hip): the four
entry points on the exact probes of tests/linattn16_ref.py (proved on the CPU by tests/test_linattn16.py) and on uniform
operands, every pass in isolation against the fp64 value of the UNROUNDED operands within the derived worst-case bound of
two bf16 roundings and a K-term fp32 sum; then ``LinearAttention`` and ``DenoiserTrainer`` at that precision.  Every output
buffer holds NaN before a launch, and so does the padding of qkv and dout, which is never read."""
import functools

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd.denoiser_train import EmulatedRank

from hip_helpers import DEV, NAN, nans, pad64, padded, st
import denoiser_train_ref as T
import linattn16_ref as P
import linattn_ref as R
import unet_grad_ref as UR

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def work(B, heads, H, W):
    nbytes = int(cabi.lib().ld_dn_la_work_bytes(B, heads, H, W))
    assert nbytes > 0
    return nans(nbytes // 8, dtype=F64)


def hip_passes(qkv, dout, heads, given=None, suffix="16"):
    """The four entry points on qkv [B, 3 hidden, H, W] and dout [B, hidden, H, W] (cpu).  The context pass runs on qkv
    alone; with ``given`` (ctx, m, Z, dctx, rk: fp32 cpu tensors) every later pass reads those instead of the results of
    the passes before it.  Returns cpu tensors: ctx, kstat, out, dctx, rk, dqkv (NHWC, padded)."""
    lib = cabi.lib()
    B, _, H, W = qkv.shape
    hidden = 32 * heads
    ld3, ldo = pad64(3 * hidden), pad64(hidden)
    qp, dop = padded(qkv, ld3), padded(dout, ldo)
    f = {n: getattr(lib, f"ld_dn_la_{n}{suffix}") for n in ("context", "out", "backward_reduce", "backward_apply")}
    ctx, kstat, out = nans(B, heads, 32, 32), nans(B, heads, 32, 2), nans(B, H, W, ldo)
    cabi.check(f["context"](qp.data_ptr(), work(B, heads, H, W).data_ptr(), ctx.data_ptr(), kstat.data_ptr(), B, H, W, heads, ld3,
                            st()), "dn_la_context16")
    ctx_in, kstat_in = ctx, kstat
    if given is not None:
        ctx_in = given["ctx"].to(DEV).contiguous()
        kstat_in = torch.stack([given["m"], given["Z"]], dim=-1).to(DEV).contiguous()
    cabi.check(f["out"](qp.data_ptr(), ctx_in.data_ptr(), out.data_ptr(), B, H, W, heads, ld3, ldo, st()), "dn_la_out16")
    dctx, rk, dqkv = nans(B, heads, 32, 32), nans(B, heads, 32), nans(B, H, W, ld3)
    cabi.check(f["backward_reduce"](qp.data_ptr(), dop.data_ptr(), ctx_in.data_ptr(), work(B, heads, H, W).data_ptr(),
                                    dctx.data_ptr(), rk.data_ptr(), B, H, W, heads, ld3, ldo, st()), "dn_la_backward_reduce16")
    dctx_in, rk_in = dctx, rk
    if given is not None:
        dctx_in, rk_in = given["dctx"].to(DEV).contiguous(), given["rk"].to(DEV).contiguous()
    cabi.check(f["backward_apply"](qp.data_ptr(), dop.data_ptr(), ctx_in.data_ptr(), kstat_in.data_ptr(), dctx_in.data_ptr(),
                                   rk_in.data_ptr(), dqkv.data_ptr(), B, H, W, heads, ld3, ldo, st()), "dn_la_backward_apply16")
    torch.cuda.synchronize()
    return dict(ctx=ctx.cpu(), kstat=kstat.cpu(), out=out.cpu(), dctx=dctx.cpu(), rk=rk.cpu(), dqkv=dqkv.cpu())


def thirds(hip, heads):
    """out [B, hidden, H, W] and dq, dk, dv [B, heads, 32, n] of the padded NHWC results; the padding must be zero."""
    hidden = 32 * heads
    B, H, W, _ = hip["out"].shape
    assert bool((hip["out"][..., hidden:] == 0).all()) and bool((hip["dqkv"][..., 3 * hidden:] == 0).all())
    out = hip["out"][..., :hidden].permute(0, 3, 1, 2)
    d = [hip["dqkv"][..., i * hidden:(i + 1) * hidden].permute(0, 3, 1, 2).reshape(B, heads, 32, H * W) for i in range(3)]
    return out, d[0], d[1], d[2]


# ------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("shape", P.PROBE_SHAPES)
@pytest.mark.parametrize("kind", P.PROBE_KINDS)
def test_exact_probes(shape, kind):
    """k constant per channel, q constant per pixel, integers in the four rounded memory operands in turn: ctx, dctx and
    (m, Z) = (c, n) bit for bit (the merge's fp64 arithmetic restated and cast), out / dq / dk / dv within 2^-21 of the fp64
    value element by element (the trailing fp32 multiplications), where a missing or truncating rounding is off by more
    than 2^-12; rk by ``reduction_bound``; padding exactly zero."""
    pr = P.probe(shape, kind)
    hip = hip_passes(pr.qkv, pr.dout, pr.heads, pr.given)
    w = pr.want
    assert torch.equal(hip["kstat"], w.kstat), "kstat"
    assert torch.equal(hip["ctx"], w.ctx), float((hip["ctx"] - w.ctx).abs().max())
    assert torch.equal(hip["dctx"], w.dctx), float((hip["dctx"] - w.dctx).abs().max())
    out, dq, dk, dv = thirds(hip, pr.heads)
    for name, got, want in (("out", out, w.out), ("dq", dq, w.dq), ("dk", dk, w.dk), ("dv", dv, w.dv)):
        err = (got.double() - want).abs()
        worst = float((err / want.abs().clamp_min(1e-300)).max()) if bool(want.any()) else 0.0
        print(f"probe {shape} {kind} {name}: largest relative error {worst:.2e} (bound {2.0 ** -21:.2e})")
        assert bool((err <= 2.0 ** -21 * want.abs()).all()), (name, worst)
    R.reduction_bound(hip["rk"], w.rk64, w.rk32, f"probe {shape} {kind} rk")


# ------------------------------------------------------------------------------------------------ 2. random operands
@functools.lru_cache(maxsize=None)
def random_case(B, heads, H, W, shifted):
    """tests/test_hip_linattn_grad.py's operands; the given ctx / (m, Z) / dctx / rk are the fp64 values cast to fp32, so
    every pass is measured by itself.  (Computed once, never changed.)"""
    hidden, n = 32 * heads, H * W
    key = 1000 * heads + 10 * H + W
    qkv = R.uniform((B, 3 * hidden, H, W), key, -2.0, 2.0)
    if shifted:
        qkv.reshape(B, 3 * hidden, n)[:, hidden:2 * hidden, n - n // 4:] += 100.0
    dout = R.uniform((B, hidden, H, W), key + 1)
    first = P.core16(qkv, heads, dout, None, F64, P._same)
    given = dict(ctx=first.ctx.float(), m=first.m.float(), Z=first.Z.float(), dctx=first.dctx.float(), rk=first.rk.float())
    ref = P.core16(qkv, heads, dout, given, F64, P._same)
    return qkv, dout, given, ref, P.bounds(ref), hip_passes(qkv, dout, heads, given)


@pytest.mark.parametrize("B,heads,H,W,shifted", P.CORE_CASES)
def test_every_pass_within_the_derived_bound(B, heads, H, W, shifted):
    """Each pass on given inputs against the unrounded fp64 value: element by element within ``linattn16_ref.bounds`` (two
    bf16 roundings, a K-term fp32 sum, an absolute term for operands below bf16's normal range -- the shifted case, whose
    ks ~ e^-100 rounds to zero), carried through the fp32 formulas of dq and dk.  m is exact and Z, which sums the unrounded
    P, is held to the fp32 path's bound.  The largest error / bound is printed per output; on an MI355X: ctx 0.05 - 0.24,
    out 0.39 - 0.44, dctx 0.05 - 0.21, dq 0.13 - 0.15, dk 0.29 - 0.32, dv 0.37 - 0.42, relative errors 1.3e-3 - 3.3e-3."""
    qkv, dout, given, ref, bd, hip = random_case(B, heads, H, W, shifted)
    tag = f"core16 B{B} h{heads} {H}x{W}{' shifted' if shifted else ''}"
    for v in hip.values():
        assert bool(torch.isfinite(v).all())
    assert torch.equal(hip["kstat"][..., 0].double(), ref.m)
    ref32 = R.core(qkv, heads, None, F32)
    R.reduction_bound(hip["kstat"][..., 1], ref.Z, ref32["Z"], tag + " Z")
    out, dq, dk, dv = thirds(hip, heads)
    for name, got in (("ctx", hip["ctx"]), ("out", out), ("dctx", hip["dctx"]), ("dq", dq), ("dk", dk), ("dv", dv)):
        want, bound = getattr(ref, name), getattr(bd, name)
        err = (got.double() - want).abs()
        ratio = float((err / bound).max())
        print(f"{tag} {name}: largest error / bound {ratio:.3f}, rel err {R.rel_err(got, want):.2e}")
        assert ratio <= 1.0, (name, ratio)
    rk_bound = (bd.dctx * given["ctx"].double().abs()).sum(dim=-1) + 1e-5 * float(ref.rk.abs().max())
    rk_want = (given["ctx"].double() * ref.dctx).sum(dim=-1)
    assert bool(((hip["rk"].double() - rk_want).abs() <= rk_bound).all())


def test_the_fp32_entry_points_are_untouched_by_the_siblings():
    """The same operands through the fp32 entry points, before and after the bf16 ones ran: the same bits, and not the bf16
    results."""
    B, heads, H, W, _ = P.CORE_CASES[1]
    qkv, dout, given, _, _, hip16 = random_case(B, heads, H, W, False)
    a = hip_passes(qkv, dout, heads, given, suffix="")
    hip_passes(qkv, dout, heads, given)
    b = hip_passes(qkv, dout, heads, given, suffix="")
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for k in ("ctx", "out", "dctx", "dqkv"):
        assert not torch.equal(a[k], hip16[k]), k
    assert torch.equal(a["kstat"][..., 0], hip16["kstat"][..., 0])


# ------------------------------------------------------------------------------------------------ 3. the module
def hip_module(dim, heads, sd, precision):
    mod = ldh.LinearAttention(dim, heads=heads)
    mod.load_state_dict(sd)
    mod.attn_precision = precision
    return mod.to(DEV)


def forward_backward(mod, x, dout):
    xd = x.to(DEV).requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    out = mod(xd)
    out.backward(dout.to(DEV))
    grads = {"x": xd.grad.cpu()}
    grads.update({k: p.grad.cpu() for k, p in mod.named_parameters() if p.grad is not None})
    return out.detach().cpu(), grads


@pytest.mark.parametrize("B,dim,heads,H,W", P.MODULE_CASES)
def test_module_at_bf16(B, dim, heads, H, W):
    """``LinearAttention`` at ``attn_precision="bf16"``: for the output and all six gradients the distance to the fp64
    yardstick of the UNROUNDED module is at most max(1e-5, 2 d), d = the distance of the CPU restatement of the module on
    ``core16`` from the same yardstick (computed here; the factor two covers operands that round the other way on the
    device and the summation order).  The result is reproducible with NaN-filled buffers, differs from the fp32 module's,
    and setting the attribute back gives the fp32 bits again.  The observed HIP / restatement ratios are printed; on an
    MI355X they were 0.84 - 1.21 on the output and the gradients of x and of the weights, and at most 1.48 (the gradient of
    ``to_out.0.bias`` at dim 64, 14 x 14, where both distances are near 1e-5); 1.00 at 5 x 3 and 8 x 8."""
    sd = R.make_attn(dim, heads, key=dim + heads)
    x = R.uniform((B, dim, H, W), 11 * dim + H)
    dout = R.uniform((B, dim, H, W), 17 * dim + H) / (B * H * W)
    mod32 = hip_module(dim, heads, sd, "fp32")
    out32, g32 = forward_backward(mod32, x, dout)
    mod = hip_module(dim, heads, sd, "bf16")
    out, grads = forward_backward(mod, x, dout)
    o64, g64 = R.yardstick(sd, x, dout, heads, dtype=F64)
    o16, g16 = P.yardstick16(sd, x, dout, heads, F64)
    tag = f"module16 B{B} dim{dim} h{heads} {H}x{W}"
    assert set(grads) == set(g64)
    for name, got, want, restated in [("out", out, o64, o16)] + [("d " + k, grads[k], g64[k], g16[k]) for k in g64]:
        e, d = R.rel_err(got, want), R.rel_err(restated, want)
        print(f"{tag} {name}: HIP {e:.2e}, restatement {d:.2e}, ratio {e / d:.2f}")
        assert e <= max(1e-5, 2 * d), (name, e, d)
    assert not torch.equal(out, out32) and not torch.equal(grads["to_qkv.weight"], g32["to_qkv.weight"])
    mod.debug_fill = NAN
    out2, grads2 = forward_backward(mod, x, dout)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    mod.attn_precision = "fp32"
    out3, grads3 = forward_backward(mod, x, dout)
    assert torch.equal(out3, out32) and all(torch.equal(grads3[k], g32[k]) for k in g32)


# ------------------------------------------------------------------------------------------------ 4. the trainer
OPTS = dict(branch_out=False, start_intermediate=False, start_timestep=2, mask_x=False, ood_AD=False, ood_confidence=False,
            classifier=False, use_gt=False, data="mnist")
TIMESTEPS = 250
CASE = UR.CASES[1]                                          # mnist, 2 x 1 x 12 x 12: the smallest net the trainer tests train


def make_trainer(**kw):
    inf = ldh.Unet(dim=32, init_dim=32, compute_dtype="fp32", **UR.KWARGS["mnist"])
    inf.load_state_dict(UR.state("mnist"))
    gd = ldh.GaussianDiffusion(OPTS, inf, image_size=12, timesteps=TIMESTEPS, objective="pred_v").to(DEV)
    return ldh.DenoiserTrainer(gd, train_lr=1e-3, **kw)


def batch(j=0):
    return tuple(v.to(DEV) for v in T.batch(CASE, 0, j, TIMESTEPS))


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
    tr.check_finite()
    return tr, (loss.clone(), grad, flat_params(tr))


@pytest.mark.parametrize("extra", [{}, dict(conv_precision="bf16", act_storage="bf16")])
def test_trainer_at_bf16_attention_is_reproducible(extra):
    """Two trainers built with ``attn_precision="bf16"`` (and, second case, the convolutions' two switches as well), one of
    them with NaN-filled buffers: the same loss, flat gradient and parameters after a step, bit for bit, finite; only the
    ``LinearAttention`` modules carry the precision; the result is not the one without the switch."""
    seen = []
    for fill in (None, NAN):
        tr, state = one_step(fill, attn_precision="bf16", **extra)
        assert tr.attn_precision == "bf16" and tr.online_model.attn_precision == "bf16"
        assert tr.conv_precision == extra.get("conv_precision", "fp32")
        lin = [m for m in tr.online_model.modules() if isinstance(m, ldh.LinearAttention)]
        assert lin and all(m.attn_precision == "bf16" for m in lin)
        assert all(m.attn_precision == "fp32" for m in tr.online_model.modules() if isinstance(m, ldh.Attention))
        assert all(bool(torch.isfinite(v).all()) for v in state) and bool(state[1].any())
        seen.append(state)
    for a, b in zip(*seen):
        assert torch.equal(a, b)
    _, base = one_step(**extra)
    assert not torch.equal(base[1], seen[0][1])
    rel = abs(float(base[0]) - float(seen[0][0])) / float(base[0])
    print(f"attn bf16 trainer {extra}: loss {float(seen[0][0]):.6f}, without {float(base[0]):.6f} (rel {rel:.2e})")
    assert rel < 2e-2


def test_trainer_without_the_keyword_runs_the_fp32_launches():
    """A trainer built without the keyword gives, bit for bit, what one gives whose ``LinearAttention`` modules were never
    told about the attribute and whose library has the four bf16 entry points taken away: the old launches, the old bits."""
    _, want = one_step()
    tr = make_trainer()
    assert tr.attn_precision == "fp32"
    assert all("attn_precision" not in vars(m) for m in tr.online_model.modules() if isinstance(m, ldh.LinearAttention))
    real, seen = cabi.lib, []

    class Fp32Only:
        def __getattr__(self, name):
            assert not (name.startswith("ld_dn_la_") and name.endswith("16")), name
            if name.startswith("ld_dn_la_"):
                seen.append(name)
            return getattr(real(), name)
    cabi.lib = lambda: Fp32Only()
    try:
        hr, lr, t, noise = batch()
        loss = tr.accumulate(hr, lr, t=t, noise=noise)
        grad = flat_grad(tr)
        tr.apply()
    finally:
        cabi.lib = real
    assert {"ld_dn_la_context", "ld_dn_la_out", "ld_dn_la_backward_reduce", "ld_dn_la_backward_apply"} <= set(seen)
    assert torch.equal(loss, want[0]) and torch.equal(grad, want[1]) and torch.equal(flat_params(tr), want[2])


def test_two_emulated_ranks_stay_identical():
    """Two emulated data-parallel ranks at ``attn_precision="bf16"``: equal ``replica_digest()``s after a step."""
    ranks = [make_trainer(comm=EmulatedRank(2, r), attn_precision="bf16") for r in range(2)]
    for r, tr in enumerate(ranks):
        hr, lr, t, noise = batch(r)
        tr.accumulate(hr, lr, scale=0.5, t=t, noise=noise)
    gathered = torch.stack([tr.send_buffer() for tr in ranks]).contiguous()
    for tr in ranks:
        tr.apply(gathered=gathered)
    a, b = (dict(tr.replica_digest()) for tr in ranks)
    assert a == b and a["step"] == 1
    assert torch.equal(flat_params(ranks[0]), flat_params(ranks[1]))
