"""GPU tests of full Attention's core on the bf16 matrix cores (csrc/attention16.hip, ``full_attn_precision="bf16"``):
the exact probes of tests/attention16_ref.py, random operands against the CPU restatement of the contract, the fp32 entry
points next to their siblings, the module, and the trainer.  Every output buffer holds NaN before a launch, and so does
the padding of qkv, out and dout; padding must come out as zero."""
import functools

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd.denoiser_train import EmulatedRank

from hip_helpers import DEV, NAN, nans, pad64, padded, st
import attention16_ref as P
import attention_ref as R
import denoiser_train_ref as T
import unet_grad_ref as UR

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------ 1. the kernels
def hip_core(qkv, dout, heads, suffix="16", given=None, quiet=False):
    """The forward (with lse; ``quiet``: once more without) and, with ``dout``, the backward -- on the forward's own lse and
    out, or on ``given``'s -- through ``ld_dn_fa_*<suffix>``; cpu tensors: out [B, H, W, ldo], lse, dqkv [B, H, W, ld3]."""
    B, c3, H, W = qkv.shape
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


def nchw(t, c):
    return t[..., :c].permute(0, 3, 1, 2).contiguous()


def thirds(dqkv, heads):
    """dq, dk, dv [B, heads, 32, n] of a [B, H, W, ld3] tensor."""
    B, H, W, _ = dqkv.shape
    hidden = 32 * heads
    return [nchw(dqkv[..., i * hidden:(i + 1) * hidden], hidden).reshape(B, heads, 32, H * W) for i in range(3)]


def within(got, want, name):
    """Element by element within 2^-21 relative of the fp64 value: one trailing fp32 multiplication."""
    bad = (got.double() - want).abs() > 2.0 ** -21 * want.abs()
    assert not bool(bad.any()), (name, int(bad.sum()), float((got.double() - want).abs().max()))


@pytest.mark.parametrize("shape", P.PROBE_SHAPES)
@pytest.mark.parametrize("kind", P.FORWARD_KINDS)
def test_exact_forward_probes(shape, kind):
    """k constant over the keys: p = 1, l = n, out = mean_j(v^_j) and lse = a + log n, whatever the order of the sums.  out
    within 2^-21 relative of the fp64 value element by element (the one multiplication by 1 / n), lse within 2^-21 max(1,
    |lse|); the padding exactly zero; the lse-less forward gives the same bits."""
    B, heads, H, W = shape
    pr = P.forward_probe(shape, kind)
    hip = hip_core(pr.qkv, None, heads, quiet=True)
    hidden = 32 * heads
    within(nchw(hip["out"], hidden), pr.want.out, "out")
    err = (hip["lse"].double() - pr.want.lse).abs()
    assert bool((err <= 2.0 ** -21 * pr.want.lse.abs().clamp_min(1.0)).all()), float(err.max())
    assert bool((hip["out"][..., hidden:] == 0).all()) and torch.equal(hip["out"], hip["quiet"])


@pytest.mark.parametrize("shape", P.PROBE_SHAPES)
@pytest.mark.parametrize("kind", P.BACKWARD_KINDS)
def test_exact_backward_probes(shape, kind):
    """lse_i = the fp32 logit of row i and out = 0 are fed: p = 1 on every valid pair, delta = 0, ds = dP an integer.  dv, a
    sum of integers, bit for bit; dq and dk within 2^-21 relative of the fp64 value element by element (the one trailing
    32^-0.5); the padding of dqkv exactly zero.  A row or key past n that entered a sum would show as well: p = 1 there too."""
    B, heads, H, W = shape
    pr = P.backward_probe(shape, kind)
    hip = hip_core(pr.qkv, pr.dout, heads, given=pr.given)
    dq, dk, dv = thirds(hip["dqkv"], heads)
    assert torch.equal(dv.double(), pr.want.dv)
    within(dq, pr.want.dq, "dq")
    within(dk, pr.want.dk, "dk")
    assert bool((hip["dqkv"][..., 96 * heads:] == 0).all())


@functools.lru_cache(maxsize=None)
def random_case(B, heads, H, W, scaled):
    """tests/test_hip_attention_grad.py's operands of the case, the bf16 entry points' results, the fp64 value of the
    unrounded operands and the CPU restatement of the contract in fp64 and in fp32 (computed once, never changed)."""
    hidden, n = 32 * heads, H * W
    key = 1000 * heads + 10 * H + W
    qkv = R.uniform((B, 3 * hidden, H, W), key, -2.0, 2.0)
    if scaled:                                           # logits reach +-121 in the last quarter of the keys
        qkv.reshape(B, 3 * hidden, n)[:, hidden:2 * hidden, n - n // 4:] *= 20.0
    dout = R.uniform((B, hidden, H, W), key + 1)
    hip = hip_core(qkv, dout, heads, quiet=True)
    return qkv, dout, hip, R.core(qkv, heads, dout, F64), P.core16(qkv, heads, dout, None, F64), P.core16(qkv, heads, dout, None, F32)


def five(core, heads):
    """out, lse, dq, dk, dv of a reference (the oracle's dict or ``core16``'s namespace)."""
    if isinstance(core, dict):
        hidden = 32 * heads
        return dict(out=core["out"], lse=core["lse"], **{"d" + c: core["dqkv"][:, i * hidden:(i + 1) * hidden] for i, c in enumerate("qkv")})
    hs = core.out.shape
    return dict(out=core.out, lse=core.lse, dq=core.dq.reshape(hs), dk=core.dk.reshape(hs), dv=core.dv.reshape(hs))


@pytest.mark.parametrize("B,heads,H,W,scaled", P.CORE_CASES)
def test_random_operands_within_twice_the_restatement(B, heads, H, W, scaled):
    """For each of out, lse, dq, dk, dv by itself: e, the distance of HIP from the fp64 value of the UNROUNDED operands, is at
    most max(1e-5, 2 d), d = the distance of ``core16`` (bf16 operands, fp64 elsewhere) from the same value, computed here.
    The factor covers computed operands (p, ds) that round the other way on the device, and the order of the sums.
    Everything is finite, the padding is zero, the lse-less forward gives the same bits.  e, d, e / d and HIP's distance
    from the fp32 restatement are printed.  On an MI355X: e / d 0.88 - 1.15 over the five outputs and seven cases (1.00 for
    lse and dv everywhere, and for everything at 1 and 15 pixels), e 4e-4 - 7e-3 (8e-2 in the scaled case, where d is the
    same); HIP is 1e-7 - 3.6e-3 from the fp32 restatement (p and ds round the other way here and there)."""
    qkv, dout, hip, ref, r64, r32 = random_case(B, heads, H, W, scaled)
    hidden = 32 * heads
    tag = f"fa16 B{B} h{heads} {H}x{W}{' k x20' if scaled else ''}"
    for k, v in hip.items():
        assert bool(torch.isfinite(v).all()), k
    assert torch.equal(hip["out"], hip["quiet"])
    dq, dk, dv = (t.reshape(B, hidden, H, W) for t in thirds(hip["dqkv"], heads))
    got = dict(out=nchw(hip["out"], hidden), lse=hip["lse"], dq=dq, dk=dk, dv=dv)
    want, rest, rest32 = five(ref, heads), five(r64, heads), five(r32, heads)
    for name in ("out", "lse", "dq", "dk", "dv"):
        e, d = R.rel_err(got[name].double(), want[name]), R.rel_err(rest[name], want[name])
        print(f"{tag} {name}: HIP {e:.2e}, restatement {d:.2e}, ratio {e / d if d else float('inf'):.2f}, HIP to the fp32 restatement "
              f"{R.rel_err(got[name], rest32[name]):.2e}")
        assert e <= max(1e-5, 2 * d), (name, e, d)
    assert bool((hip["out"][..., hidden:] == 0).all())
    assert bool((hip["dqkv"][..., 3 * hidden:] == 0).all())


# ------------------------------------------------------------------------------------------------ 2. the siblings
def test_the_fp32_entry_points_are_untouched_by_the_siblings():
    """The same operands through the fp32 entry points, before and after the bf16 ones ran: the same bits, and not the bf16
    results."""
    B, heads, H, W, _ = P.CORE_CASES[3]
    qkv, dout, hip16, _, _, _ = random_case(B, heads, H, W, False)
    a = hip_core(qkv, dout, heads, suffix="")
    again = hip_core(qkv, dout, heads)
    b = hip_core(qkv, dout, heads, suffix="")
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(again[k], hip16[k]), k
        assert not torch.equal(a[k], hip16[k]), k


# ------------------------------------------------------------------------------------------------ 3. the module
def hip_module(dim, heads, sd, precision, **kw):
    mod = ldh.Attention(dim, heads=heads)
    mod.load_state_dict(sd)
    mod.full_attn_precision = precision
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


@pytest.mark.parametrize("B,dim,heads,H,W", P.MODULE_CASES)
def test_module_at_bf16(B, dim, heads, H, W):
    """``Attention`` at ``full_attn_precision="bf16"``: for the output and all five gradients the distance to the fp64
    yardstick of the UNROUNDED module is at most max(1e-5, 2 d), d = the distance of the CPU restatement of the module on
    ``core16`` from the same yardstick (computed here).  The result is reproducible with NaN-filled buffers, differs from
    the fp32 module's, and setting the attribute back gives the fp32 bits again.  The HIP / restatement ratios are printed;
    on an MI355X they were 0.86 - 1.14 on the output and the gradients of x, ``norm.g`` and the two weights (e 6e-4 - 2.7e-3);
    the gradient of ``to_out.bias`` does not pass the core: d = 0, e at most 4.2e-8, under the floor."""
    sd = R.make_attn(dim, heads, key=dim + heads)
    x = R.uniform((B, dim, H, W), 13 * dim + H)
    dout = R.uniform((B, dim, H, W), 19 * dim + H) / (B * H * W)
    mod32 = hip_module(dim, heads, sd, "fp32")
    out32, g32 = forward_backward(mod32, x, dout)
    mod = hip_module(dim, heads, sd, "bf16")
    out, grads = forward_backward(mod, x, dout)
    o64, g64 = R.yardstick(sd, x, dout, heads, dtype=F64)
    o16, g16 = P.yardstick16(sd, x, dout, heads, F64)
    tag = f"module16 B{B} dim{dim} h{heads} {H}x{W}"
    assert set(grads) == set(g64) == {"x", "norm.g", "to_qkv.weight", "to_out.weight", "to_out.bias"}
    for name, got, want, restated in [("out", out, o64, o16)] + [("d " + k, grads[k], g64[k], g16[k]) for k in g64]:
        e, d = R.rel_err(got.double(), want), R.rel_err(restated, want)
        print(f"{tag} {name}: HIP {e:.2e}, restatement {d:.2e}, ratio {e / d if d else float('inf'):.2f}")
        assert e <= max(1e-5, 2 * d), (name, e, d)
    assert not torch.equal(out, out32) and not torch.equal(grads["to_qkv.weight"], g32["to_qkv.weight"])
    mod.debug_fill = NAN
    out2, grads2 = forward_backward(mod, x, dout)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    mod.full_attn_precision = "fp32"
    out3, grads3 = forward_backward(mod, x, dout)
    assert torch.equal(out3, out32) and all(torch.equal(grads3[k], g32[k]) for k in g32)


def test_module_composes_with_bf16_convolutions():
    """Both switches on one module: bit-identical across two runs (the second with NaN-filled buffers), finite, and neither
    the result of one switch alone."""
    B, dim, heads, H, W = P.MODULE_CASES[2]
    sd = R.make_attn(dim, heads, key=dim + heads)
    x = R.uniform((B, dim, H, W), 13 * dim + H)
    dout = R.uniform((B, dim, H, W), 19 * dim + H) / (B * H * W)
    mod = hip_module(dim, heads, sd, "bf16", conv_precision="bf16")
    out, grads = forward_backward(mod, x, dout)
    mod.debug_fill = NAN
    out2, grads2 = forward_backward(mod, x, dout)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    for alone in (dict(precision="bf16"), dict(precision="fp32", conv_precision="bf16")):
        o, g = forward_backward(hip_module(dim, heads, sd, **alone), x, dout)
        assert not torch.equal(o, out) and not torch.equal(g["x"], grads["x"]), alone
    o64, _ = R.yardstick(sd, x, dout, heads, dtype=F64)
    e = R.rel_err(out.double(), o64)
    print(f"module16 with bf16 convolutions: out {e:.2e} from the fp64 yardstick")
    assert e < 5e-2


# ------------------------------------------------------------------------------------------------ 4. the trainer
# (tests/test_hip_linattn16.py's helpers restated: a test file is not importable from another)
OPTS = dict(branch_out=False, start_intermediate=False, start_timestep=2, mask_x=False, ood_AD=False, ood_confidence=False,
            classifier=False, use_gt=False, data="mnist")
TIMESTEPS = 250
CASE = UR.CASES[1]                                          # mnist, 2 x 1 x 12 x 12: full attention sees 9 pixels or fewer


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


@pytest.mark.parametrize("extra", [{}, dict(conv_precision="bf16", act_storage="bf16", attn_precision="bf16")])
def test_trainer_at_bf16_full_attention_is_reproducible(extra):
    """Two trainers built with ``full_attn_precision="bf16"`` (and, second case, the other three switches as well), one of
    them with NaN-filled buffers: the same loss, flat gradient and parameters after a step, bit for bit, finite; every
    ``Attention`` carries the precision and ``LinearAttention.attn_precision`` is what ``attn_precision`` says; the gradient
    is not the one without the switch."""
    seen = []
    for fill in (None, NAN):
        tr, state = one_step(fill, full_attn_precision="bf16", **extra)
        assert tr.full_attn_precision == "bf16" and tr.online_model.full_attn_precision == "bf16"
        assert tr.attn_precision == extra.get("attn_precision", "fp32") and tr.conv_precision == extra.get("conv_precision", "fp32")
        full = [m for m in tr.online_model.modules() if isinstance(m, ldh.Attention)]
        lin = [m for m in tr.online_model.modules() if isinstance(m, ldh.LinearAttention)]
        assert len(full) == 3 and all(m.full_attn_precision == "bf16" and m.attn_precision == "fp32" for m in full)
        assert len(lin) == 4 and all(m.attn_precision == extra.get("attn_precision", "fp32") for m in lin)
        assert not any(hasattr(m, "full_attn_precision") for m in lin)
        assert all(bool(torch.isfinite(v).all()) for v in state) and bool(state[1].any())
        seen.append(state)
    for a, b in zip(*seen):
        assert torch.equal(a, b)
    _, base = one_step(**extra)
    assert not torch.equal(base[1], seen[0][1])
    rel = abs(float(base[0]) - float(seen[0][0])) / float(base[0])
    print(f"full attn bf16 trainer {extra}: loss {float(seen[0][0]):.6f}, without {float(base[0]):.6f} (rel {rel:.2e})")
    assert rel < 2e-2


def test_a_default_trainer_is_the_one_without_the_argument():
    """``full_attn_precision="fp32"`` spelled out gives, bit for bit, what a trainer built without the argument gives, no
    module carries the attribute in ``vars()``, and only the fp32 entry points of the core are called."""
    _, want = one_step()
    tr = make_trainer(full_attn_precision="fp32")
    assert tr.full_attn_precision == "fp32" and tr.online_model.full_attn_precision == "fp32"
    assert not any("full_attn_precision" in vars(m) for m in tr.online_model.modules())
    real, seen = cabi.lib, []

    class Fp32Only:
        def __getattr__(self, name):
            assert not (name.startswith("ld_dn_fa_") and name.endswith("16")), name
            if name.startswith("ld_dn_fa_"):
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
    assert {"ld_dn_fa_forward", "ld_dn_fa_backward"} <= set(seen)
    assert torch.equal(loss, want[0]) and torch.equal(grad, want[1]) and torch.equal(flat_params(tr), want[2])


def test_two_emulated_ranks_stay_identical():
    """Two emulated data-parallel ranks at ``full_attn_precision="bf16"``: equal ``replica_digest()``s after a step."""
    ranks = [make_trainer(comm=EmulatedRank(2, r), full_attn_precision="bf16") for r in range(2)]
    for r, tr in enumerate(ranks):
        hr, lr, t, noise = batch(r)
        tr.accumulate(hr, lr, scale=0.5, t=t, noise=noise)
    gathered = torch.stack([tr.send_buffer() for tr in ranks]).contiguous()
    for tr in ranks:
        tr.apply(gathered=gathered)
    a, b = (dict(tr.replica_digest()) for tr in ranks)
    assert a == b and a["step"] == 1
    assert torch.equal(flat_params(ranks[0]), flat_params(ranks[1]))
