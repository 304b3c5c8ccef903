"""CPU tests of mixed-precision training (``amp``): the yardsticks of tests/amp_ref.py prove their own preconditions, the
scaler's rule is held against the real ``torch.amp.GradScaler``, and everything ``amp`` refuses is refused without a GPU."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import checkpoint, denoiser_train, trainable, weights
from localdiffusion_hallucination_amd.trainable import TrainableModule

import amp_ref as A
import conv16_ref as P
import denoiser_train_ref as T
import unet_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
CFG = dict(branch_out=False, start_intermediate=False, start_timestep=2, data="mnist", mask_x=False, ood_AD=False,
           ood_confidence=False, classifier=False, use_gt=False)
OVERFLOW_SCALE, SAFE_SCALE = 2.0 ** 30, 2.0 ** 10       # tests/test_hip_amp.py starts its overflowing run at the first


def diffusion(seed=3, timesteps=100, objective="pred_x0"):
    net = ldh.Unet(dim=32, init_dim=32, **R.KWARGS["mnist"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.procedural_state_dict(net.cfg, seed).items()})
    return ldh.GaussianDiffusion(dict(CFG), net, image_size=28, timesteps=timesteps, objective=objective)


# ------------------------------------------------------------------------------------------------ 1. rounding and probes
def test_fp16_rounding_helpers():
    """``h`` rounds to nearest even and overflows to inf; ``trunc16`` chops; the operand builders hold what they promise."""
    t = torch.tensor([2049.0, 2051.0, 4095.0, 257.0, 2047.0, 65504.0, 65519.0, 65520.0, 1e5, -1e5])
    assert A.h(t).tolist() == [2048.0, 2052.0, 4096.0, 257.0, 2047.0, 65504.0, 65504.0, math.inf, math.inf, -math.inf]
    assert A.trunc16(t[:5]).tolist() == [2048.0, 2050.0, 4094.0, 257.0, 2047.0]
    only = A.fp16_only_ints((4096,), 1)
    assert torch.equal(A.h(only), only) and not torch.equal(P.q(only), only) and 257 <= float(only.abs().min()) and \
        float(only.abs().max()) <= 2047 and bool((only < 0).any()) and bool((only > 0).any())
    ties = A.fp16_ties((4096,), 2)
    odd = ties[ties.abs() > 2048]
    assert odd.numel() > 1000 and bool((odd.abs() % 2 == 1).all()) and float(odd.abs().max()) <= 4095
    assert bool((A.h(odd) != odd).all()) and bool(((A.h(odd) - odd).abs() == 1).all()) and bool((A.h(odd) % 4 == 0).all())


@pytest.mark.parametrize("shape", P.CONV_SHAPES)
@pytest.mark.parametrize("kind", ["identity", "rounding"])
def test_conv_probes_prove_themselves(shape, kind):
    """(The builder asserts: exact below 2^24, and not the result of a bf16, a truncating or a non-rounding kernel.)"""
    p = A.conv_probe(shape, kind, epilogue=shape == P.CONV_WITH_EPILOGUE)
    assert p.ref.shape == (shape[0], shape[2], shape[3], shape[4]) and bool(p.ref.any())


@pytest.mark.parametrize("kind", ["identity_w", "rounding_w", "identity_dy", "rounding_dy"])
def test_dgrad_probes_prove_themselves(kind):
    p = A.dgrad_probe(P.DGRAD_SHAPE, kind)
    assert p.ref.shape == (P.DGRAD_SHAPE[0], P.DGRAD_SHAPE[1], P.DGRAD_SHAPE[3], P.DGRAD_SHAPE[4]) and bool(p.ref.any())


@pytest.mark.parametrize("shape", P.WGRAD_SHAPES)
@pytest.mark.parametrize("kind", ["identity_dy", "rounding_dy", "identity_a", "rounding_a"])
def test_wgrad_probes_prove_themselves(shape, kind):
    p = A.wgrad_probe(shape, kind)
    assert p.ref.shape == (shape[2], shape[1], shape[5], shape[5]) and bool(p.ref.any())


@pytest.mark.parametrize("shape", P.PACK_SHAPES)
def test_pack_probes_prove_themselves(shape):
    p = A.pack_probe(shape)
    co, ci, k = shape
    assert p.fwd.numel() == p.cop * k * k * p.cip and int((p.fwd != 0).sum()) == co * ci * k * k == int((p.dgr != 0).sum())
    assert torch.equal(p.fwd.to(torch.float16).float(), p.fwd)


# ------------------------------------------------------------------------------------------------ 2. the scaler's rule
SEQUENCE = ["finite", "finite", "inf", "finite", "nan"] + ["finite"] * 5      # crosses growth_interval = 3 twice
SCALER = dict(init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)


def scripted_grads(sizes, step, what, scale):
    g = {str(i): R.uniform((c,), 8000 + 10 * step + i) * scale for i, c in enumerate(sizes)}
    if what != "finite":
        g["1"][2] = float(what)
    return g


def test_scaler_rule_is_gradscalers():
    """The literal restatement of ``ld_dn_opt_scaler_update`` (amp_ref.scaler_rule) against the real
    ``torch.amp.GradScaler('cpu')`` driving ``torch.optim.Adam(foreach=False)`` with ``clip_grad_norm_`` after ``unscale_``, over
    finite, finite, inf, finite, NaN and five finite steps at ``growth_interval`` 3: the scale, the tracker, which steps were
    skipped and Adam's ``state['step']`` are equal after every step; and parameters stepped by the rule's own arithmetic --
    unscale, clip, Adam with the rule's ``step_size`` / ``bc2_sqrt`` in fp64 -- equal torch's fp64 parameters bit for bit
    (``torch.equal``) when fed the same gradient bits."""
    sizes = [5, 32, 7]
    lr, betas, eps = 1e-3, T.ADAM["betas"], T.ADAM["eps"]
    p0 = {str(i): R.uniform((c,), 7900 + i) for i, c in enumerate(sizes)}
    rep = A.ScaledReplica(p0, lr, 1.0, F64, None, no_grad=(), **SCALER)
    state = A.scaler_state(SCALER["init_scale"])
    mine = {k: v.double().clone() for k, v in p0.items()}
    m = {k: torch.zeros_like(v) for k, v in mine.items()}
    v2 = {k: torch.zeros_like(v) for k, v in mine.items()}
    skipped = []
    for step, what in enumerate(SEQUENCE):
        grads = scripted_grads(sizes, step, what, state["scale"])
        assert state["scale"] == rep.scaler.get_scale()                       # the gradients are scaled by both alike
        rep.step(grads)
        sumsq = sum(float((g.double() ** 2).sum()) for g in grads.values())
        A.scaler_rule(state, math.isfinite(sumsq), lr, betas, SCALER["growth_factor"], SCALER["backoff_factor"],
                      SCALER["growth_interval"])
        skipped.append(bool(state["found_inf"]))
        sd = rep.scaler.state_dict()
        assert set(sd) == set(denoiser_train.SCALER_KEYS)
        assert (state["scale"], state["growth_tracker"]) == (sd["scale"], sd["_growth_tracker"]), (step, state, sd)
        assert state["adam_steps"] == rep.adam_steps() and skipped == rep.skipped, step
        if not state["found_inf"]:                                            # the step kernel's arithmetic, in fp64
            t = state["adam_steps"]
            g = {k: grads[k].double() * state["inv_scale"] for k in grads}
            norm = math.sqrt(sum(float((x ** 2).sum()) for x in g.values()))
            coef = min(1.0, 1.0 / (norm + 1e-6))
            for k in mine:
                gk = g[k] * coef
                m[k].lerp_(gk, 1.0 - betas[0])
                v2[k].mul_(betas[1]).addcmul_(gk, gk, value=1.0 - betas[1])
                denom = (v2[k].sqrt() / math.sqrt(1.0 - betas[1] ** t)).add_(eps)
                mine[k].addcdiv_(m[k], denom, value=-(lr / (1.0 - betas[0] ** t)))
        for k in mine:
            assert torch.equal(mine[k], rep.p[k].detach()), (step, k)
    assert skipped == [w != "finite" for w in SEQUENCE] and state["skipped_steps"] == 2 and state["adam_steps"] == 8
    # finite x2 (tracker 2), inf (2^15, 0), finite (1), nan (2^14, 0), finite x3 (2^15, 0), finite x2 (tracker 2)
    assert (state["scale"], state["growth_tracker"]) == (2.0 ** 15, 2)


def test_the_rule_never_grows_into_inf():
    """At the largest fp32 power of two the growth is refused (torch checks the product), the tracker still returns to 0."""
    state = A.scaler_state(2.0 ** 127)
    A.scaler_rule(state, True, 1e-3, (0.9, 0.99), growth_interval=1)
    assert state["scale"] == 2.0 ** 127 and state["growth_tracker"] == 0 and state["adam_steps"] == 1
    s = torch.amp.GradScaler("cpu", init_scale=2.0 ** 127, growth_interval=1)
    p = torch.zeros(2, requires_grad=True)
    opt = torch.optim.Adam([p], foreach=False)
    s.scale(torch.zeros(1))
    p.grad = torch.ones(2)
    s.step(opt)
    s.update()
    assert s.get_scale() == 2.0 ** 127


def test_the_overflowing_scale_overflows_on_the_cpu_too():
    """The run of tests/test_hip_amp.py whose first step must be skipped starts at 2^30: the CPU denoiser with fp16-rounded
    convolution operands (amp_ref.fp16_convs) and the loss times 2^30 has non-finite gradients at the trainer tests' first
    step, and finite, non-zero ones at 2^10, which are 2^10 times the unscaled ones up to the operands' rounding."""
    case = R.CASES[1]
    gd = diffusion(0, timesteps=250, objective="pred_v")
    schedule = tuple(getattr(gd, n) for n in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "loss_weight"))
    sd = R.state("mnist")
    big = A.first_step_grads(case, sd, schedule, "pred_v", 250, OVERFLOW_SCALE)
    bad = [k for k, g in big.items() if not bool(torch.isfinite(g).all())]
    small = A.first_step_grads(case, sd, schedule, "pred_v", 250, SAFE_SCALE)
    print(f"loss scale 2^30: {len(bad)} of {len(big)} gradients are not finite; 2^10: largest element "
          f"{max(float(g.abs().max()) for g in small.values()):.3e}")
    assert bad and all(bool(torch.isfinite(g).all()) for g in small.values())
    assert all(bool(g.any()) for k, g in small.items())
    # and outside the context the convolution is torch's again
    assert torch.nn.functional.conv2d is A._conv2d


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_amp_is_validated_on_assignment_and_no_switch():
    assert trainable.AMP_TYPES == ("no", "fp16") and "amp" not in trainable.SWITCHES and TrainableModule.amp == "no"
    blk = ldh.ResnetBlock(32, 64, time_emb_dim=32)
    assert blk.amp == "no" and blk.operand_precision == "fp32" and "amp" not in blk.state_dict()
    for bad in ("bf16", "fp32", True, None, "FP16"):
        with pytest.raises(ValueError, match="amp .* is not one of 'no', 'fp16'"):
            blk.amp = bad
        assert blk.amp == "no"
    blk.amp = "fp16"
    assert blk.operand_precision == "fp16" and blk.conv_precision == "fp32" and "amp" not in blk.state_dict()
    with pytest.raises(ValueError, match="amp 'fp16' and conv_precision 'bf16'"):
        blk.conv_precision = "bf16"
    assert blk.conv_precision == "fp32"
    with pytest.raises(ValueError, match="needs conv_precision 'bf16'"):       # the storage switches stay out of reach
        trainable.check_storage_precision("ResnetBlock", "act_storage", "bf16", blk.conv_precision)
    blk.amp = "no"
    blk.conv_precision = "bf16"
    assert blk.operand_precision == "bf16"
    with pytest.raises(ValueError, match="amp 'fp16' and conv_precision 'bf16'"):
        blk.amp = "fp16"
    assert blk.amp == "no"


def test_trainable_unet_hands_amp_down():
    kw = dict(dim=32, init_dim=32, **R.KWARGS["mnist"])
    net = ldh.TrainableUnet(**kw, amp="fp16")
    mods = [m for m in net.modules() if isinstance(m, TrainableModule)]
    assert net.amp == "fp16" and len(mods) > 20 and all(m.amp == "fp16" and m.operand_precision == "fp16" for m in mods)
    assert not any("amp" in k for k in net.state_dict())
    with pytest.raises(ValueError, match="amp 'fp16' and conv_precision 'bf16'"):
        net.conv_precision = "bf16"
    assert net.conv_precision == "fp32" and all(m.conv_precision == "fp32" for m in mods)
    net.amp = "no"
    assert all(m.amp == "no" for m in mods)
    net.conv_precision = "bf16"
    with pytest.raises(ValueError, match="amp 'fp16' and conv_precision 'bf16'"):
        net.amp = "fp16"
    assert net.amp == "no" and all(m.amp == "no" for m in mods)
    with pytest.raises(ValueError, match="is not one of 'no', 'fp16'"):
        ldh.TrainableUnet(**kw, amp="bf16")
    with pytest.raises(ValueError, match="amp 'fp16' and conv_precision 'bf16'"):
        ldh.TrainableUnet(**kw, amp="fp16", conv_precision="bf16")
    plain = ldh.TrainableUnet(**kw)
    assert plain.amp == "no" and all("amp" not in vars(m) for m in plain.modules() if isinstance(m, TrainableModule))


def test_the_packed_weight_cache_key_holds_amp():
    import inspect
    src = inspect.getsource(trainable.PackedWeights._packed_for)
    assert '"amp"' in src and '"conv_precision"' in src


def test_trainer_refusals_need_no_gpu():
    gd = diffusion()
    with pytest.raises(ValueError, match="GaussianDiffusion"):                # as the other argument checks: before any GPU use
        ldh.DenoiserTrainer(None, amp=True)
    for kw, match in ((dict(amp=True, mixed_precision_type="fp8"), "mixed_precision_type"),
                      (dict(amp=True, mixed_precision_type="no"), "mixed_precision_type"),
                      (dict(amp=False, mixed_precision_type="tf32"), "mixed_precision_type"),
                      (dict(amp=1), "amp"),
                      (dict(amp=True, conv_precision="bf16"), "amp 'fp16' and conv_precision 'bf16'"),
                      (dict(amp=True, conv_precision="fp16"), "conv_precision"),
                      (dict(amp=True, mixed_precision_type="bf16", conv_precision="fp32"), "contradicts"),
                      (dict(amp=True, mixed_precision_type="bf16", scaler_kwargs=dict(init_scale=2.0)), "no loss scaler"),
                      (dict(amp=False, scaler_kwargs=dict(init_scale=2.0)), "scaler_kwargs"),
                      (dict(amp=True, act_storage="bf16"), "needs conv_precision 'bf16'"),
                      (dict(amp=True, scaler_kwargs=dict(init_scale=3.0)), "power of two"),
                      (dict(amp=True, scaler_kwargs=dict(init_scale=0.0)), "power of two"),
                      (dict(amp=True, scaler_kwargs=dict(init_scale=-4.0)), "power of two"),
                      (dict(amp=True, scaler_kwargs=dict(init_scale=float("inf"))), "init_scale"),
                      (dict(amp=True, scaler_kwargs=dict(growth_factor=1.0)), "growth_factor"),
                      (dict(amp=True, scaler_kwargs=dict(backoff_factor=1.0)), "backoff_factor"),
                      (dict(amp=True, scaler_kwargs=dict(backoff_factor=0.0)), "backoff_factor"),
                      (dict(amp=True, scaler_kwargs=dict(growth_interval=0)), "growth_interval"),
                      (dict(amp=True, scaler_kwargs=dict(growth_interval=2.5)), "growth_interval"),
                      (dict(amp=True, scaler_kwargs=dict(enabled=True)), "scaler_kwargs")):
        with pytest.raises(ValueError, match=match):
            ldh.DenoiserTrainer(gd, **kw)
    for kw in (dict(amp=True), dict(amp=True, mixed_precision_type="bf16"), dict(amp=True, mixed_precision_type="bf16",
               conv_precision="bf16"), dict(amp=True, scaler_kwargs=dict(init_scale=2.0 ** 30, growth_interval=2)), dict()):
        with pytest.raises(ValueError, match="is on cpu"):                    # the last refusal: everything else is fine
            ldh.DenoiserTrainer(gd, **kw)
    assert denoiser_train.check_amp(True, "fp16", None, None) == ("fp16", "fp32", denoiser_train.SCALER_DEFAULTS)
    assert denoiser_train.check_amp(True, "bf16", None, None) == ("no", "bf16", None)
    assert denoiser_train.check_amp(False, "fp16", None, None) == ("no", "fp32", None)
    assert denoiser_train.SCALER_DEFAULTS == dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)
    ref = torch.amp.GradScaler("cpu")
    ref.scale(torch.zeros(1))
    assert {k: ref.state_dict()[k] for k in denoiser_train.SCALER_DEFAULTS if k != "init_scale"} == \
        {k: v for k, v in denoiser_train.SCALER_DEFAULTS.items() if k != "init_scale"} and ref.get_scale() == 65536.0


# ------------------------------------------------------------------------------------------------ 4. checkpoint_dict
def trainer_state(step=7, **kw):
    gd = diffusion(3)
    online = ldh.TrainableUnet(**denoiser_train.online_kwargs(gd.model))
    online.load_state_dict({k: torch.from_numpy(v) for k, v in weights.procedural_state_dict(gd.model.cfg, 4).items()})
    osd = {k: p.detach() for k, p in online.named_parameters()}
    esd = {k: v.detach() for k, v in gd.model.state_dict().items()}
    moments = {k: (torch.full_like(v, 0.25), torch.full_like(v, 0.5)) for k, v in osd.items() if k not in T.NO_GRAD}
    args = (gd.state_dict(), osd, esd, moments)
    return args, lambda opt_step, **kw: denoiser_train.checkpoint_dict(step, *args, opt_step, 2e-4, (0.8, 0.95), 1e-7, step, True, **kw)


def test_checkpoint_dict_with_a_scaler(tmp_path):
    """``'scaler'`` holds ``GradScaler.state_dict()``'s five keys, every ``opt`` step is Adam's own count (below ``step`` after
    skipped steps), the file round-trips through ``torch.save`` / ``checkpoint._read`` (the safe loader), and the real
    ``GradScaler.load_state_dict`` takes it; without a scaler the dictionary is what it was."""
    _, make = trainer_state(7)
    scaler = {"scale": 2.0 ** 14, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 3}
    data = make(5, scaler=scaler)
    assert set(data) == {"step", "model", "opt", "ema", "scaler"} and data["step"] == 7
    assert data["scaler"] == scaler and set(data["scaler"]) == set(torch.amp.GradScaler("cpu").state_dict())
    assert {float(s["step"]) for s in data["opt"]["state"].values()} == {5.0}
    path = str(tmp_path / "model-best100.pt")
    torch.save(data, path)
    back = checkpoint._read(path, False)
    assert back["scaler"] == scaler and back["step"] == 7 and float(back["opt"]["state"][0]["step"]) == 5.0
    ref = torch.amp.GradScaler("cpu")
    ref.load_state_dict(back["scaler"])
    assert ref.get_scale() == 2.0 ** 14 and ref.get_growth_interval() == 2000
    plain, old = make(7), make(7, scaler=None)
    assert plain["scaler"] is None and old["scaler"] is None and set(plain) == set(data)
    assert {float(s["step"]) for s in plain["opt"]["state"].values()} == {7.0}
    for k in plain["model"]:
        assert torch.equal(plain["model"][k], data["model"][k]), k
    with pytest.raises(ValueError, match="scaler must have the keys"):
        make(5, scaler={"scale": 1.0})
    with pytest.raises(ValueError, match="Adam's step count"):
        make(8, scaler=scaler)


# ------------------------------------------------------------------------------------------------ the C ABI, host half
NEW_SYMBOLS = ["ld_dn_conv_f16", "ld_dn_wgrad_f16", "ld_dn_pack_conv_f16", "ld_dn_scaler_init", "ld_dn_opt_scaler_update",
               "ld_dn_opt_step_scaled", "ld_p_losses_grad_scaled"]


def test_header_declares_and_cabi_binds_the_new_symbols():
    src = open(os.path.join(ROOT, "include", "localdiff_hip.h")).read()
    lib = cabi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)), f"{name} is not declared"
        assert name in cabi.EXPORTS and hasattr(lib, name)
    body = re.search(r"typedef struct ld_dn_scaler_state \{(.*?)\} ld_dn_scaler_state;", src, flags=re.S).group(1)
    fields = re.findall(r"^\s*(float|int32_t)\s+(\w+);", body, flags=re.M)
    ctype = {"float": C.c_float, "int32_t": C.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(cabi.DnScalerState._fields_) and C.sizeof(cabi.DnScalerState) == 32
    assert [n for _, n in fields][:5] == ["scale", "growth_tracker", "adam_steps", "skipped_steps", "found_inf"]


def test_argument_validation_needs_no_gpu():
    """The fp16 entry points refuse what their bf16 twins refuse, in their words; the scaler's refuse bad pointers and
    factors.  All return -1 before any launch."""
    lib = cabi.lib()
    buf = (C.c_double * 64)()
    p, N = (C.addressof(buf) + 15) // 16 * 16, None

    def conv(fn, **kw):
        a = cabi.PcConvArgs()
        a.src, a.scale, a.shift, a.out = p, p, p, p
        a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.Cout, a.ksize, a.stride, a.relu = 1, 4, 4, 32, 4, 4, 64, 3, 1, 0
        w = kw.pop("w", p)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = fn(C.byref(a), w, N)
        return rc, lib.ld_last_error().decode()
    for kw in (dict(ksize=5), dict(stride=2), dict(B=0), dict(Ho=5), dict(Cin=48), dict(Cout=32), dict(src=N), dict(w=N),
               dict(src=p + 4), dict(w=p + 8)):
        (rc16, e16), (rcf, ef) = conv(lib.ld_dn_conv16, **dict(kw)), conv(lib.ld_dn_conv_f16, **dict(kw))
        assert rc16 == rcf == -1 and ef == e16.replace("ld_dn_conv16", "ld_dn_conv_f16") and "ld_dn_conv_f16" in ef, (kw, e16, ef)

    def wgrad(fn, dy=p, a=p, work=p, dw=p, B=1, H=4, W=4, cin=64, cout=64, k=3, splits=1):
        return fn(dy, a, work, dw, B, H, W, cin, cout, k, splits, N), lib.ld_last_error().decode()
    for kw in (dict(k=2), dict(B=0), dict(cin=32), dict(cout=96), dict(splits=0), dict(splits=2), dict(dy=N), dict(dw=N),
               dict(a=p + 4)):
        (rc16, e16), (rcf, ef) = wgrad(lib.ld_dn_wgrad16, **kw), wgrad(lib.ld_dn_wgrad_f16, **kw)
        assert rc16 == rcf == -1 and ef == e16.replace("ld_dn_wgrad16", "ld_dn_wgrad_f16") and "ld_dn_wgrad_f16" in ef, (kw, e16, ef)

    def pack(fn, w=p, fwd=p, dgr=p, co=20, cop=64, ci=3, cip=64, k=3):
        return fn(w, fwd, dgr, co, cop, ci, cip, k, N), lib.ld_last_error().decode()
    for kw in (dict(k=5), dict(co=0), dict(cop=16), dict(cip=63, ci=3), dict(w=N), dict(fwd=p + 2)):
        (rc16, e16), (rcf, ef) = pack(lib.ld_dn_pack_conv16, **kw), pack(lib.ld_dn_pack_conv_f16, **kw)
        assert rc16 == rcf == -1 and ef == e16.replace("ld_dn_pack_conv16", "ld_dn_pack_conv_f16") and "ld_dn_pack_conv_f16" in ef, kw

    assert lib.ld_dn_scaler_init(N, 65536.0, 0, 0, N) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_scaler_init(p + 2, 65536.0, 0, 0, N) == -1
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.ld_dn_scaler_init(p, scale, 0, 0, N) == -1 and b"init_scale" in lib.ld_last_error(), scale
    assert lib.ld_dn_scaler_init(p, 2.0, -1, 0, N) == -1 and lib.ld_dn_scaler_init(p, 2.0, 0, -1, N) == -1

    def update(state=p, ss=p, lr=1e-3, b1=0.9, b2=0.99, growth=2.0, backoff=0.5, interval=2000):
        return lib.ld_dn_opt_scaler_update(state, ss, lr, b1, b2, growth, backoff, interval, N)
    for kw in (dict(state=N), dict(ss=N)):
        assert update(**kw) == -1 and b"null" in lib.ld_last_error(), kw
    for kw in (dict(state=p + 2), dict(ss=p + 4)):
        assert update(**kw) == -1 and b"aligned" in lib.ld_last_error(), kw
    for kw in (dict(lr=0.0), dict(b1=1.0), dict(b2=-0.1), dict(growth=1.0), dict(backoff=1.0), dict(backoff=0.0), dict(interval=0),
               dict(growth=float("nan"))):
        assert update(**kw) == -1, kw

    def step(table=p, n=3, wg=4, g=p, m=p, v=p, e=p, flat=64, ss=p, state=p, max_norm=1.0, a=(0.9, 0.99, 1e-8), mode=0, w=0.5):
        return lib.ld_dn_opt_step_scaled(table, n, wg, g, m, v, e, flat, ss, state, max_norm, *a, mode, w, N)
    for kw in (dict(table=N), dict(g=N), dict(m=N), dict(v=N), dict(e=N), dict(ss=N), dict(state=N)):
        assert step(**kw) == -1 and b"null" in lib.ld_last_error(), kw
    for kw in (dict(g=p + 4), dict(m=p + 8), dict(ss=p + 4), dict(table=p + 4), dict(state=p + 2)):
        assert step(**kw) == -1 and b"aligned" in lib.ld_last_error(), kw
    for kw in (dict(n=0), dict(wg=2), dict(flat=62), dict(max_norm=-1.0), dict(a=(1.0, 0.99, 1e-8)), dict(mode=3), dict(mode=2, w=1.5)):
        assert step(**kw) == -1, kw

    def lossgrad(scale=p, out=p, B=2, per=16, obj=0):
        return lib.ld_p_losses_grad_scaled(p, p, p, p, p, p, p, 1.0, scale, out, B, per, obj, N)
    assert lossgrad(scale=N) == -1 and b"ld_p_losses_grad_scaled: null" in lib.ld_last_error()
    assert lossgrad(B=0) == -1 and lossgrad(obj=9) == -1 and lossgrad(out=N) == -1
    assert all(v == 0.0 for v in buf)
