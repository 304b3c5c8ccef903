"""CPU-side checks of ``DenoiserTrainer`` (no GPU needed): the EMA rule as a pure function, the refusals, the layout of the
checkpoint ``save`` writes, the host half of the optimiser kernels' C ABI (the table layout, the argument checks), and the
yardstick of the GPU tests exercised for two steps."""
import ctypes as C
import json
import os
import re

import pytest
import torch

import conftest
import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import checkpoint, denoiser_train, weights

import denoiser_train_ref as T
import unet_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ld_dn_opt_layout", "ld_dn_opt_sqnorm_work_bytes", "ld_dn_opt_sqnorm", "ld_dn_opt_step"]
CFG = dict(branch_out=False, start_intermediate=False, start_timestep=2, data="mnist", mask_x=False, ood_AD=False,
           ood_confidence=False, classifier=False, use_gt=False)
F32, F64 = torch.float32, torch.float64


def diffusion(seed=3, timesteps=100, objective="pred_x0", **kw):
    args = dict(dim=32, init_dim=32, **R.KWARGS["mnist"])
    args.update(kw)
    net = ldh.Unet(**args)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.procedural_state_dict(net.cfg, seed).items()})
    return ldh.GaussianDiffusion(dict(CFG), net, image_size=28, timesteps=timesteps, objective=objective)


def test_public_surface():
    assert "DenoiserTrainer" in ldh.__all__ and ldh.DenoiserTrainer is denoiser_train.DenoiserTrainer
    assert (denoiser_train.EMA_KEEP, denoiser_train.EMA_COPY, denoiser_train.EMA_LERP) == (0, 1, 2)


# ------------------------------------------------------------------------------------------------ the EMA rule
def test_ema_action_pattern_and_decays():
    """s = 0 .. 40 with update_every 2 and update_after_step 4: odd calls do nothing, 0 / 2 / 4 copy, every even call from 6 on
    lerps with the decay of the formula (here written out again); an EMA never initialised copies at its first lerp call."""
    kw = dict(beta=0.9, update_every=2, update_after_step=4, inv_gamma=1.0, power=2 / 3, min_value=0.0)
    for s in range(41):
        mode, decay = denoiser_train.ema_action(s, **kw)
        if s % 2:
            assert (mode, decay) == (0, 0.0), s
        elif s <= 4:
            assert (mode, decay) == (1, 0.0), s
        else:
            e = s + 1 - 4 - 1
            want = min(max(1.0 - (1.0 + e) ** (-2.0 / 3.0), 0.0), 0.9)
            assert mode == 2 and decay == pytest.approx(want, rel=1e-15, abs=0.0), s
            assert decay == T.ema_decay(s, **kw)
    assert denoiser_train.ema_action(40, **kw)[1] == 0.9                                   # clamped to beta
    assert denoiser_train.ema_action(6, initted=False, **kw) == (1, denoiser_train.ema_action(6, **kw)[1])
    low = dict(kw, min_value=0.8)
    assert denoiser_train.ema_action(6, **low)[1] == 0.8                                   # clamped to min_value
    assert denoiser_train.ema_action(12, **dict(kw, inv_gamma=2.0, power=1.0))[1] == pytest.approx(1 - 1 / (1 + 8 / 2.0))


def test_ema_action_at_the_references_defaults():
    """EMA(beta 0.995, update_every 10) with ema_pytorch's update_after_step 100, inv_gamma 1, power 2/3: 1 - (1 + e)^(-2/3)."""
    table = {0: (1, 0.0), 1: (0, 0.0), 9: (0, 0.0), 10: (1, 0.0), 55: (0, 0.0), 100: (1, 0.0), 105: (0, 0.0),
             110: (2, 0.79781999176642), 120: (2, 0.86862265826756), 200: (2, 0.95389099497223),
             1000: (2, 0.98928027923520), 2000: (2, 0.99348353717434), 2500: (2, 0.99442294115809), 3000: (2, 0.995),
             10000: (2, 0.995), 100000: (2, 0.995)}                         # (from s = 2930 on the formula exceeds beta)
    for s, (mode, decay) in table.items():
        got = denoiser_train.ema_action(s)
        assert got[0] == mode and got[1] == pytest.approx(decay, abs=1e-13), (s, got)


def test_literal_rule_agrees_with_ema_action():
    """tests/denoiser_train_ref.ema_update (copy-on-first-use, then lerp, written out) against ema_action + one lerp / copy: the
    same tensors, bit for bit, over 12 calls -- the never-initialised lerp call is a copy."""
    online = {"w": torch.arange(5.0)}
    ema_a, ema_b = {"w": torch.zeros(5)}, {"w": torch.zeros(5)}
    initted_a = initted_b = False
    seen = []
    for s in range(12):
        online["w"] = online["w"] * 1.25 + 0.5
        what, initted_a = T.ema_update(s, ema_a, online, initted_a, **T.EMA_KW)
        mode, decay = denoiser_train.ema_action(s, initted=initted_b, **T.EMA_KW)
        if s % 2 == 0 and s > T.EMA_KW["update_after_step"]:
            initted_b = True
        if mode == 1:
            ema_b["w"].copy_(online["w"])
        elif mode == 2:
            ema_b["w"].lerp_(online["w"], 1.0 - decay)
        seen.append((what, mode))
        assert torch.equal(ema_a["w"], ema_b["w"]), s
    assert seen[:7] == [("copy", 1), ("skip", 0), ("copy", 1), ("skip", 0), ("lerp", 1), ("skip", 0), ("lerp", 2)]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_need_no_gpu():
    with pytest.raises(ValueError, match="self_condition"):
        ldh.DenoiserTrainer(diffusion(self_condition=True))
    with pytest.raises(ValueError, match="groups"):                       # what TrainableUnet refuses
        ldh.DenoiserTrainer(diffusion(resnet_block_groups=16))
    with pytest.raises(ValueError, match="GaussianDiffusion"):
        ldh.DenoiserTrainer(torch.nn.Linear(2, 2))
    gd = diffusion()
    for kw, match in ((dict(train_lr=0.0), "train_lr"), (dict(train_lr=float("nan")), "train_lr"), (dict(eps=-1e-8), "eps"),
                      (dict(max_grad_norm=-1.0), "max_grad_norm"), (dict(adam_betas=(0.9, 1.0)), "adam_betas"),
                      (dict(adam_betas=(0.9,)), "adam_betas"), (dict(ema_decay=1.5), "ema_decay"),
                      (dict(ema_min_value=0.999), "ema_min_value"), (dict(ema_update_every=0), "ema_update_every"),
                      (dict(ema_update_every=2.5), "ema_update_every"), (dict(ema_update_after_step=-1), "ema_update_after_step"),
                      (dict(ema_inv_gamma=0.0), "ema_inv_gamma"), (dict(ema_power=-1.0), "ema_power")):
        with pytest.raises(ValueError, match=match):
            ldh.DenoiserTrainer(gd, **kw)
    with pytest.raises(ValueError, match="is on cpu"):                    # the last refusal: everything else is fine
        ldh.DenoiserTrainer(gd)


# ------------------------------------------------------------------------------------------------ the checkpoint's layout
def trainer_state(step=7):
    gd = diffusion(3)
    online = ldh.TrainableUnet(**denoiser_train.online_kwargs(gd.model))
    online.load_state_dict({k: torch.from_numpy(v) for k, v in weights.procedural_state_dict(gd.model.cfg, 4).items()})
    osd = {k: p.detach() for k, p in online.named_parameters()}
    esd = {k: v.detach() for k, v in gd.model.state_dict().items()}
    moments = {k: (torch.full_like(v, 0.25), torch.full_like(v, 0.5)) for k, v in osd.items() if k not in T.NO_GRAD}
    data = denoiser_train.checkpoint_dict(step, gd.state_dict(), osd, esd, moments, step, 2e-4, (0.8, 0.95), 1e-7, step, True)
    return gd, osd, esd, data


def test_checkpoint_layout_matches_the_references_manifest(tmp_path):
    """``model`` and ``ema`` of the dictionary ``save`` writes, built from CPU state_dicts through ``checkpoint_dict``, against
    the manifest of the file the reference's own ``Trainer.save`` wrote (g12): names, shapes, dtypes; ``opt`` has no entry for
    the two ``conv_fusion.mlp.1.*`` indices and ``torch.optim.Adam.load_state_dict`` accepts it; ``load_reference_checkpoint``
    reads the file back with source ``ema``."""
    want = json.load(open(os.path.join(conftest.GOLDEN, "g12_trainer_save_manifest.json")))
    gd, osd, esd, data = trainer_state()
    assert set(data) == {"step", "model", "opt", "ema", "scaler"} and data["scaler"] is None and data["step"] == 7

    def walk(d):
        return {k: [list(v.shape), str(v.dtype)] for k, v in d.items()}
    assert walk(data["model"]) == want["model"] and walk(data["ema"]) == want["ema"]
    assert list(data["model"]) == list(gd.state_dict())
    assert torch.equal(data["model"]["model.init_conv.weight"], osd["init_conv.weight"])
    assert torch.equal(data["ema"]["online_model.model.init_conv.weight"], osd["init_conv.weight"])
    assert torch.equal(data["ema"]["ema_model.model.init_conv.weight"], esd["init_conv.weight"])
    assert not torch.equal(osd["init_conv.weight"], esd["init_conv.weight"])
    assert torch.equal(data["ema"]["ema_model.betas"], gd.betas) and int(data["ema"]["step"]) == 7 and bool(data["ema"]["initted"])
    names = list(osd)
    absent = [i for i in range(len(names)) if i not in data["opt"]["state"]]
    assert [names[i] for i in absent] == list(T.NO_GRAD)
    group = data["opt"]["param_groups"][0]
    assert group["lr"] == 2e-4 and group["betas"] == (0.8, 0.95) and group["eps"] == 1e-7
    assert group["params"] == list(range(len(names)))
    path = tmp_path / "model-best100.pt"
    torch.save(data, str(path))
    back = torch.load(str(path), map_location="cpu", weights_only=True)
    params = [torch.nn.Parameter(v.clone()) for v in osd.values()]
    opt = torch.optim.Adam(params, lr=1.0)
    opt.load_state_dict(back["opt"])
    assert opt.param_groups[0]["lr"] == 2e-4 and len(opt.state) == len(names) - 2
    assert float(opt.state[params[0]]["step"]) == 7.0 and bool((opt.state[params[0]]["exp_avg_sq"] == 0.5).all())
    dst = diffusion(9)
    info = checkpoint.load_reference_checkpoint(str(path), dst)
    assert info == {"step": 7, "source": "ema", "missing": [], "unexpected": []}
    for k, v in esd.items():
        assert torch.equal(dst.model.state_dict()[k], v), k
    with pytest.raises(ValueError, match="do not match"):
        denoiser_train.checkpoint_dict(0, gd.state_dict(), {"init_conv.weight": osd["init_conv.weight"]}, esd, {}, 0, 1e-4,
                                       (0.9, 0.99), 1e-8, 0, False)


# ------------------------------------------------------------------------------------------------ the C ABI, host half
def test_header_declares_and_cabi_binds_the_new_symbols():
    src = open(os.path.join(ROOT, "include", "localdiff_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = cabi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in the header"
        assert name in cabi.EXPORTS and hasattr(lib, name)
    assert re.search(r"#define\s+LD_DN_OPT_CHUNK\s+%d\b" % cabi.DN_OPT_CHUNK, src)
    assert re.search(r"#define\s+LD_DN_OPT_ADAM\s+%d\b" % cabi.DN_OPT_ADAM, src)
    assert C.sizeof(cabi.DnOptTensor) == 32
    build = open(os.path.join(ROOT, "localdiffusion-hallucination_amd", "csrc", "build.sh")).read()
    assert "denoiser_opt" in build


def host_table(counts, flags=None, base=None):
    buf = (C.c_float * 64)()
    p = C.addressof(buf) if base is None else base
    tab = (cabi.DnOptTensor * len(counts))()
    for i, (e, c) in enumerate(zip(tab, counts)):
        e.param, e.count, e.flags = p, c, (1 if flags is None else flags[i])
    tab._keep = buf
    return tab


def test_layout_is_aligned_and_no_workgroup_straddles_two_tensors():
    lib = cabi.lib()
    counts = [1, 3, 5, 32, 1000, 4096, 4097, 294912, 2]
    tab = host_table(counts, flags=[1, 1, 0, 1, 1, 1, 1, 1, 0])
    flat, wgs = cabi.i64(), cabi.i64()
    assert lib.ld_dn_opt_layout(tab, len(counts), C.byref(flat), C.byref(wgs)) == 0
    off = wg = 0
    for e, c in zip(tab, counts):
        assert (e.offset, e.first_wg) == (off, wg) and e.offset % 4 == 0 and e.count == c
        off += (c + 3) // 4 * 4
        wg += (c + cabi.DN_OPT_CHUNK - 1) // cabi.DN_OPT_CHUNK
    assert (flat.value, wgs.value) == (off, wg) and wg == 6 + 2 + 72 + 1
    assert int(lib.ld_dn_opt_sqnorm_work_bytes(wg)) == 8 * wg and int(lib.ld_dn_opt_sqnorm_work_bytes(0)) == 0
    # refused: nothing is written
    for bad in (dict(counts=[4, 0]), dict(counts=[4, -1]), dict(counts=[4, 4], flags=[1, 2]), dict(counts=[4, 1 << 41])):
        tab = host_table(**bad)
        flat.value = wgs.value = -7
        assert lib.ld_dn_opt_layout(tab, 2, C.byref(flat), C.byref(wgs)) == -1
        assert (flat.value, wgs.value) == (-7, -7) and all(e.offset == 0 and e.first_wg == 0 for e in tab)
    tab = host_table([4, 4])
    tab[1].param = None
    assert lib.ld_dn_opt_layout(tab, 2, C.byref(flat), C.byref(wgs)) == -1 and b"null" in lib.ld_last_error()
    tab[1].param = C.addressof(tab._keep) + 2
    assert lib.ld_dn_opt_layout(tab, 2, C.byref(flat), C.byref(wgs)) == -1 and b"misaligned" in lib.ld_last_error()
    tab = host_table([4])
    assert lib.ld_dn_opt_layout(tab, 0, C.byref(flat), C.byref(wgs)) == -1
    assert lib.ld_dn_opt_layout(None, 1, C.byref(flat), C.byref(wgs)) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_opt_layout(tab, 1, None, C.byref(wgs)) == -1


def test_argument_validation_needs_no_gpu():
    """Null or misaligned pointers, a zero count, a negative max_norm and bad hyper-parameters return -1 before any launch."""
    lib = cabi.lib()
    buf = (C.c_double * 64)()
    p, N = (C.addressof(buf) + 15) // 16 * 16, None
    adam = (0.9, 0.99, 1e-8, 1e-3, 0.1)

    def step(table=p, n=3, wg=4, g=p, m=p, v=p, e=p, flat=64, ss=p, max_norm=1.0, a=adam, mode=0, w=0.5):
        return lib.ld_dn_opt_step(table, n, wg, g, m, v, e, flat, ss, max_norm, *a, mode, w, N)

    def sqnorm(table=p, n=3, wg=4, g=p, flat=64, work=p, ss=p):
        return lib.ld_dn_opt_sqnorm(table, n, wg, g, flat, work, ss, N)
    for kw in (dict(table=N), dict(g=N), dict(m=N), dict(v=N), dict(e=N), dict(ss=N)):
        assert step(**kw) == -1 and b"null" in lib.ld_last_error(), kw
    for kw in (dict(g=p + 4), dict(m=p + 8), dict(v=p + 4), dict(e=p + 12), dict(ss=p + 4), dict(table=p + 4)):
        assert step(**kw) == -1 and b"aligned" in lib.ld_last_error(), kw
    for kw in (dict(n=0), dict(n=-1), dict(wg=0), dict(wg=2), dict(flat=0), dict(flat=-4), dict(flat=62), dict(n=1 << 20, wg=1 << 20)):
        assert step(**kw) == -1, kw
        assert sqnorm(**kw) == -1, kw
    assert step(max_norm=-1.0) == -1 and b"max_norm" in lib.ld_last_error()
    assert step(max_norm=float("nan")) == -1 and b"max_norm" in lib.ld_last_error()
    for a in ((1.0, 0.99, 1e-8, 1e-3, 0.1), (0.9, 1.0, 1e-8, 1e-3, 0.1), (0.9, 0.99, -1e-8, 1e-3, 0.1), (0.9, 0.99, 1e-8, 1e-3, 0.0),
              (-0.1, 0.99, 1e-8, 1e-3, 0.1)):
        assert step(a=a) == -1 and b"beta1" in lib.ld_last_error(), a
    for kw in (dict(mode=3), dict(mode=-1), dict(mode=2, w=1.5), dict(mode=2, w=-0.1), dict(mode=2, w=float("nan"))):
        assert step(**kw) == -1 and b"ema_mode" in lib.ld_last_error(), kw
    for kw in (dict(table=N), dict(g=N), dict(work=N), dict(ss=N)):
        assert sqnorm(**kw) == -1 and b"null" in lib.ld_last_error(), kw
    for kw in (dict(g=p + 4), dict(work=p + 4), dict(ss=p + 4), dict(table=p + 4)):
        assert sqnorm(**kw) == -1 and b"aligned" in lib.ld_last_error(), kw
    assert all(v == 0.0 for v in buf)


# ------------------------------------------------------------------------------------------------ the yardstick
def test_yardstick_runs_two_steps_at_the_mnist_case():
    """tests/denoiser_train_ref.yardstick_steps, the GPU tests' yardstick, for two steps of two batches at the mnist case in
    fp32 and fp64: the losses agree to fp32 rounding, the clipped first Adam step moves every trained parameter by at most
    lr (1 + 1e-6) and the two unused ones not at all, and the EMA followed the rule (copy at call 0, nothing at call 1)."""
    case = R.CASES[1]
    assert case[0] == "mnist"
    gd = diffusion(0, timesteps=250, objective="pred_v")
    schedule = tuple(getattr(gd, n) for n in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "loss_weight"))
    sd = R.state("mnist")
    lr = 1e-3
    l32, r32 = T.yardstick_steps(case, sd, schedule, "pred_v", lr, 2, 2, 250, F32, T.EMA_KW)
    l64, r64 = T.yardstick_steps(case, sd, schedule, "pred_v", lr, 2, 2, 250, F64, T.EMA_KW)
    print("yardstick losses: fp32 " + " ".join(f"{v:.8f}" for v in l32) + "; fp64 " + " ".join(f"{v:.8f}" for v in l64))
    assert all(abs(a - b) < 1e-5 * max(1.0, abs(b)) for a, b in zip(l32, l64))
    assert r64.norm > 1.0                                                  # the clip is live at these weights
    _, one = T.yardstick_steps(case, sd, schedule, "pred_v", lr, 1, 2, 250, F64, T.EMA_KW)
    for k, v in sd.items():
        moved = float((one.p[k].detach() - v.double()).abs().max())
        if k in T.NO_GRAD:
            assert moved == 0.0 and torch.equal(r32.p[k].detach(), v), k
        else:
            assert 0.0 < moved <= lr * (1 + 1e-6), (k, moved)
        assert torch.equal(one.ema[k], one.p[k].detach()), k              # call 0: copy
        assert not torch.equal(r64.ema[k], r64.p[k].detach()) or k in T.NO_GRAD, k      # call 1: nothing
    assert r32.s == 2 and not r32.initted
