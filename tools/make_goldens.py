#!/usr/bin/env python3
"""Golden-vector generator.  Runs ONLY in the build container (needs /root/reference).

It imports the *real* reference modules (``ddpm.py``, ``attend.py``, ``unet_model.py``) through
stub modules for the packages/files the reference imports but this image lacks,
loads this repo's procedural weights into the reference ``Unet`` by parameter name, replaces
``torch.randn`` / ``torch.randn_like`` with the portable counter-based generator
(localdiffusion_hallucination_amd.rng), runs the reference's own code on CPU and

  1. checks the oracle (oracle/unet_ref.py, oracle/diffusion_ref.py) against it, and
  2. writes small input/output fixtures to tests/golden/*.npz.

The fixtures are data (inputs + expected outputs); no reference source travels.
Usage:  python tools/make_goldens.py [--only G1,G2,...] [--skip-long]
"""
import argparse
import contextlib
import gzip
import io
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = "/root/reference"
GOLD = os.path.join(ROOT, "tests", "golden")

import localdiffusion_hallucination_amd as ldh           # noqa: E402
from localdiffusion_hallucination_amd import rng, weights, schedule   # noqa: E402
from oracle import unet_ref, diffusion_ref                # noqa: E402


# ----------------------------------------------------------------------------- reference import
def import_reference():
    sys.dont_write_bytecode = True

    class _Dummy:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return self

    def mk(name):
        m = types.ModuleType(name)

        def ga(attr):
            if attr.startswith("__"):
                raise AttributeError(attr)
            return _Dummy
        m.__getattr__ = ga
        m.__path__ = []
        sys.modules[name] = m
    for n in ["torchvision", "torchvision.transforms", "torchvision.utils",
              "torchvision.transforms.functional", "ema_pytorch", "idx2numpy", "timm", "nibabel",
              "medpy", "medpy.io", "anomalib", "anomalib.models", "anomalib.models.components",
              "anomalib.models.patchcore", "anomalib.models.patchcore.anomaly_map",
              "anomalib.pre_processing", "anomalib.config", "train_fusion", "data", "models"]:
        mk(n)
    sys.path.insert(0, REF)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import ddpm
    torch.Tensor.cuda = lambda self, *a, **k: self          # ddpm.py:743,748,754 on a CPU box
    return ddpm


class PortableNoise:
    """Monkeypatch target: every randn/randn_like call is draw #k of the portable stream."""

    def __init__(self, seed=10):
        self.seed, self.k = seed, 0

    def randn(self, *shape, **kw):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        out = torch.from_numpy(rng.randn(tuple(shape), self.seed, self.k))
        self.k += 1
        return out

    def randn_like(self, x, **kw):
        return self.randn(tuple(x.shape))

    def __call__(self, shape):
        return self.randn(tuple(shape))


@contextlib.contextmanager
def reference_run(noise):
    """temp CWD with ./fusion_test, silenced stdout, portable noise patched into torch."""
    old = (torch.randn, torch.randn_like, os.getcwd())
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "fusion_test"))
        os.chdir(d)
        torch.randn, torch.randn_like = noise.randn, noise.randn_like
        try:
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                yield
        finally:
            torch.randn, torch.randn_like = old[0], old[1]
            os.chdir(old[2])


def sd_torch(cfg, seed=0):
    return {k: torch.from_numpy(v) for k, v in weights.procedural_state_dict(cfg, seed).items()}


def build_reference_unet(ddpm, cfg, sd):
    m = ddpm.Unet(dim=cfg.dim, init_dim=cfg.init_dim, out_dim=cfg.out_dim, dim_mults=cfg.dim_mults,
                  channels=cfg.channels, full_attn=cfg.full_attn, mode=cfg.mode)
    ref_sd = m.state_dict()
    assert list(ref_sd.keys()) == list(sd.keys()), "parameter inventory differs from the reference"
    for k in ref_sd:
        assert tuple(ref_sd[k].shape) == tuple(sd[k].shape), k
    m.load_state_dict(sd)
    return m.eval()


def base_config(**kw):
    c = dict(branch_out=False, start_intermediate=False, start_timestep=2, data="mri", mask_x=False,
             mask_cond=False, ood_AD=False, ood_confidence=False, classifier=False,
             classifier_obj="tile", use_gt=False, use_gt_timestep=100, continue_fusion_timestep=0)
    c.update(kw)
    return c


def opts_from(config, T, S=None, objective="pred_x0", sched="sigmoid"):
    return diffusion_ref.SamplerOptions(
        timesteps=T, sampling_timesteps=S, objective=objective, beta_schedule=sched,
        branch_out=config["branch_out"], start_intermediate=config["start_intermediate"],
        start_timestep=config["start_timestep"], data=config["data"], mask_x=config["mask_x"],
        ood_AD=config["ood_AD"], ood_confidence=config["ood_confidence"], classifier=bool(config.get("classifier", False)),
        use_gt=bool(config.get("use_gt", False)), use_gt_timestep=int(config.get("use_gt_timestep", 100)))


def maxdiff(a, b):
    return float((a - b).abs().max())


def save(name, **arrs):
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    print(f"  wrote {os.path.relpath(path, ROOT)}  ({os.path.getsize(path)/1024:.1f} KiB)")


CFG_MNIST = weights.UnetConfig(dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist")
CFG_MRI = weights.UnetConfig(mode="mri")
CFG_MVTEC = weights.UnetConfig(channels=3, out_dim=3, mode="mvtec")


def mnist_digits(n=4, label=3):
    """First n test digits with the given label (config.yaml:14 anomaly_name: 3)."""
    with gzip.open(os.path.join(REF, "MNIST/raw/t10k-images-idx3-ubyte.gz"), "rb") as f:
        raw = f.read()
    imgs = np.frombuffer(raw, dtype=np.uint8, offset=16).reshape(-1, 28, 28)
    with gzip.open(os.path.join(REF, "MNIST/raw/t10k-labels-idx1-ubyte.gz"), "rb") as f:
        lab = np.frombuffer(f.read(), dtype=np.uint8, offset=8)
    idx = np.nonzero(lab == label)[0][:n]
    return imgs[idx].copy()


def import_reference_dataset():
    """The reference's real ``data.py`` (its MNIST dataset class), loaded under another module name: the name
    ``data`` is a stub while ``ddpm`` is imported.  torchvision is absent here, so ``transforms.Compose`` -- the only
    torchvision symbol MNIST.__getitem__ reaches in test mode, with an empty list (data.py:792-795) -- is given its
    defining behaviour (apply the listed transforms in order)."""
    import importlib.util

    class Compose:
        def __init__(self, ts):
            self.ts = list(ts)

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x
    for n in ("torchvision.transforms",):
        sys.modules[n].Compose = Compose
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    # data.py:17,29 only takes a user-agent string from `datasets` (for an image downloader far from this path); the
    # installed package refuses to import beside the torchvision stub, so it is stubbed for the load as well
    saved = {n: sys.modules.get(n) for n in ("datasets", "datasets.utils", "datasets.utils.file_utils")}
    for n in saved:
        m = types.ModuleType(n)
        m.__path__ = []
        m.get_datasets_user_agent = lambda *a, **k: "stub"
        sys.modules[n] = m
    spec = importlib.util.spec_from_file_location("ref_data_real", os.path.join(REF, "data.py"))
    mod = importlib.util.module_from_spec(spec)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            spec.loader.exec_module(mod)
        finally:
            for n, m in saved.items():
                if m is None:
                    sys.modules.pop(n, None)
                else:
                    sys.modules[n] = m
    return mod


def mnist_lr_hr(digits, labels=None):
    """LR / HR pairs from the reference's OWN dataset code (MNIST.__getitem__, data.py:808-829), test mode.
    NB the reference indexes the [1,1,28,28] image with ``img[:, ::2, ::2]``, which decimates dims 0-2, i.e. only
    the ROWS (-> [1,1,14,28]) before the bilinear resize back to 28x28; the product's evalio.mnist_pairs follows
    that and is pinned by this fixture."""
    ref_data = import_reference_dataset()
    labels = np.full(len(digits), 3, dtype=np.uint8) if labels is None else labels
    ds = ref_data.MNIST({"augmentations": False}, digits, labels, train=False, num=[int(v) for v in set(labels.tolist())])
    assert len(ds) == len(digits)
    hr, lr = [], []
    for i in range(len(ds)):
        img, img_down, _ = ds[i]
        hr.append(img)
        lr.append(img_down)
    return torch.stack(lr), torch.stack(hr)


# ----------------------------------------------------------------------------- G1 schedules
def g1(ddpm):
    print("G1 schedule buffers")
    out = {}
    for sched in ("sigmoid", "linear", "cosine"):
        for T in (50, 100, 1000):
            gd = _ref_diffusion(ddpm, base_config(), _DummyModel(), 28, T, sched, "pred_x0", None)
            ours = schedule.make_buffers(T, sched, "pred_x0")
            orc = diffusion_ref.schedule_buffers(sched, T, "pred_x0")
            for name in schedule.BUFFER_NAMES:
                ref = getattr(gd, name)
                assert torch.equal(ref, ours[name]), (sched, T, name, "product schedule != reference")
                d = maxdiff(ref, orc[name]) / max(1e-30, float(ref.abs().max()))
                assert d < 2e-7, (sched, T, name, d)
                out[f"{sched}_{T}_{name}"] = ref.numpy()
    save("g1_schedules", **out)


class _DummyModel(torch.nn.Module):
    channels = 1
    out_dim = 1
    self_condition = False
    random_or_learned_sinusoidal_cond = False


def _ref_diffusion(ddpm, config, model, image_size, T, sched, objective, S):
    return ddpm.GaussianDiffusion(config, model, image_size=image_size, timesteps=T,
                                  beta_schedule=sched, objective=objective, auto_normalize=False,
                                  sampling_timesteps=S)


# ----------------------------------------------------------------------------- G2 forward
def tap_stats(t):
    t = t.detach().float()
    flat = t.flatten()
    idx = torch.linspace(0, flat.numel() - 1, 16).long()
    return np.concatenate([[float(t.mean()), float(t.norm())], flat[idx].numpy()]).astype(np.float32)


def g2(ddpm):
    print("G2 Unet.forward")
    out = {}
    cases = [("mnist28", CFG_MNIST, 4, 28, (0, 5, 99)),
             ("mri64", CFG_MRI, 1, 64, (0, 500, 999)),
             ("mvtec32", CFG_MVTEC, 2, 32, (3, 777))]
    for tag, cfg, B, H, ts in cases:
        sd = sd_torch(cfg)
        ref = build_reference_unet(ddpm, cfg, sd)
        cin = cfg.cond_in_channels
        x = torch.from_numpy(rng.randn((B, cfg.channels, H, H), 1, 100))
        cond = torch.from_numpy(rng.uniform((B, cin, H, H), 1, 101, 0.0, 2.0))
        for t in ts:
            tv = torch.full((B,), t, dtype=torch.long)
            hooks, caught = [], {}
            names = dict(ref.named_modules())
            want = [n for n in names if n in ("init_conv", "cond_model", "conv_fusion", "mid_block1",
                                              "mid_block2", "final_res_block")
                    or (n.count(".") == 2 and n.split(".")[0] in ("downs", "ups") and n[-1] in "01")]
            for n in want:
                hooks.append(names[n].register_forward_hook(
                    lambda mod, inp, o, n=n: caught.__setitem__(n, o.detach())))
            with torch.no_grad():
                y_ref = ref(x, cond, tv)
            for h in hooks:
                h.remove()
            taps = {}
            with torch.no_grad():
                y_orc = unet_ref.unet_forward(sd, cfg, x, cond, tv, taps)
            d = maxdiff(y_ref, y_orc)
            worst = max(maxdiff(caught[n], taps[n]) for n in want)
            print(f"  {tag} t={t}: oracle-vs-reference out {d:.2e}, worst tap {worst:.2e}")
            assert d <= 1e-5 and worst <= 1e-4, (tag, t, d, worst)
            out[f"{tag}_t{t}_out"] = y_ref.numpy()
            for n in want:
                out[f"{tag}_t{t}_tap_{n}"] = tap_stats(caught[n])
        out[f"{tag}_shape"] = np.array([B, cfg.channels, H, cin])
    save("g2_unet_forward", **out)


# ----------------------------------------------------------------------------- sampler runs
def run_pair(ddpm, cfg, config, T, S, B, H, cond, mask, lohi, objective="pred_x0", sched="sigmoid",
             record_ts=()):
    """Run reference sample() and oracle sample() on identical inputs -> (ref_out, orc_out, recs)."""
    sd = sd_torch(cfg)
    ref_model = build_reference_unet(ddpm, cfg, sd)
    config = dict(config)
    gd = _ref_diffusion(ddpm, config, ref_model, H, T, sched, objective, S).eval()
    noise = PortableNoise(10)
    t0 = time.time()
    with reference_run(noise):
        with torch.inference_mode():
            ref_out = gd.sample(cond.clone(), None, batch_size=B, mask=None if mask is None else mask.clone(),
                                min_max_val=lohi)
    t_ref = time.time() - t0
    return ref_out, t_ref, sd


def oracle_run(cfg, sd, config, T, S, B, H, cond, mask, lohi, objective="pred_x0", sched="sigmoid",
               record=None):
    o = opts_from(config, T, S, objective, sched)
    smp = diffusion_ref.RefSampler(diffusion_ref.make_model_fn(sd, cfg), o, cfg.channels, H)
    noise = PortableNoise(10)
    with torch.no_grad():
        if record is None:
            return smp.sample(cond, mask, lohi, B, noise)
        branch, fuse = o.branch_out, o.start_intermediate
        mask_x = o.mask_x or o.ood_AD or o.ood_confidence
        return smp.p_sample_loop(cond, mask, lohi, (B, cfg.channels, H, H), noise, branch, fuse, mask_x,
                                 record=record)


def to_np(x):
    if isinstance(x, (list, tuple)):
        return np.stack([t.numpy() for t in x])
    return x.numpy()


def compare(tag, ref_out, orc_out, tol):
    a, b = torch.from_numpy(to_np(ref_out)), torch.from_numpy(to_np(orc_out))
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    d = maxdiff(a, b)
    print(f"  {tag}: shape {tuple(a.shape)} oracle-vs-reference max-abs {d:.3e}")
    assert d <= tol, (tag, d)
    return d


def band_mask(B, H, ncols):
    m = torch.zeros(B, 1, H, H)
    m[:, :, :, :ncols] = 1.0
    return m


def g3(ddpm):
    """Single p_sample steps (non-branch, branch, fusion) are covered as T=3 runs with
    start_timestep=1: step t=2 is a pure branch step, t=1 the fusion step, t=0 a joint step."""
    print("G3 three-step runs (branch / fusion / joint)")
    cfg, H, B = CFG_MNIST, 28, 2
    cond = torch.from_numpy(rng.uniform((B, 1, H, H), 3, 1, 0.0, 2.0))
    mask = band_mask(B, H, 7)
    out = {"cond": cond.numpy(), "mask": mask.numpy()}
    for tag, kw in [("nonbranch", dict(data="mnist")),
                    ("branch_fuse_mnist", dict(data="mnist", branch_out=True, start_intermediate=True,
                                               start_timestep=1, mask_x=True)),
                    ("branch_fuse_mri", dict(data="mri", branch_out=True, start_intermediate=True,
                                             start_timestep=1, mask_x=True)),
                    ("branch_nofuse", dict(data="mri", branch_out=True, start_intermediate=False,
                                           mask_x=True))]:
        config = base_config(**kw)
        ref_out, _, sd = run_pair(ddpm, cfg, config, 3, None, B, H, cond, mask, (0.0, 2.0))
        orc = oracle_run(cfg, sd, base_config(**kw), 3, None, B, H, cond, mask, (0.0, 2.0))
        compare("G3 " + tag, ref_out, orc, 1e-5)
        out[tag] = to_np(ref_out)
    save("g3_three_step", **out)


def g4(ddpm):
    print("G4 cfg1: MNIST 28x28, T=100, 4 patches, branch + fusion (config.yaml defaults)")
    cfg, H, B, T = CFG_MNIST, 28, 4, 100
    digits = mnist_digits(B, 3)
    lr, hr = mnist_lr_hr(digits)
    mask = band_mask(B, H, 7)                                   # test.py:379-381
    kw = dict(data="mnist", branch_out=True, start_intermediate=True, start_timestep=2, mask_x=True,
              ood_AD=True)
    ref_out, t_ref, sd = run_pair(ddpm, cfg, base_config(**kw), T, None, B, H, lr, mask, (0.0, 2.0))
    recs = {}
    keep = (99, 50, 10, 2, 1, 0)
    orc = oracle_run(cfg, sd, base_config(**kw), T, None, B, H, lr, mask, (0.0, 2.0),
                     record=lambda t, x: recs.__setitem__(t, to_np(x)) if t in keep else None)
    compare("G4", ref_out, orc, 2e-5)
    print(f"  reference sample() wall {t_ref:.1f}s")
    save("g4_cfg1_mnist", digits=digits, cond=lr.numpy(), hr=hr.numpy(), mask=mask.numpy(),
         final=to_np(ref_out), **{f"x_after_t{t}": v for t, v in recs.items()})


def g5(ddpm):
    print("G5 cfg2: 4-stage 1-ch 128x128, T=1000, fp32, non-branch  (several minutes)")
    cfg, H, B, T = CFG_MRI, 128, 1, 1000
    cond = torch.from_numpy(rng.uniform((B, 1, H, H), 5, 1, 0.0, 2.0))
    kw = dict(data="mri")
    ref_out, t_ref, sd = run_pair(ddpm, cfg, base_config(**kw), T, None, B, H, cond, None, (0.0, 2.0))
    print(f"  reference sample() wall {t_ref:.1f}s")
    recs = {}
    keep = (999, 750, 500, 250, 100, 10, 0)
    t0 = time.time()
    orc = oracle_run(cfg, sd, base_config(**kw), T, None, B, H, cond, None, (0.0, 2.0),
                     record=lambda t, x: recs.__setitem__(t, to_np(x)) if t in keep else None)
    print(f"  oracle sample() wall {time.time()-t0:.1f}s")
    compare("G5", ref_out, orc, 1e-4)
    save("g5_cfg2_mri128", final=to_np(ref_out), ref_seconds=np.array([t_ref]),
         **{f"x_after_t{t}": v for t, v in recs.items()})


def g6(ddpm):
    print("G6 branch+fusion T=50: data='mri' 32x32 (UNet out kept) and data='mnist' 28x28")
    out = {}
    for tag, cfg, H, data in [("mri32", CFG_MRI, 32, "mri"), ("mnist28", CFG_MNIST, 28, "mnist")]:
        B, T = 2, 50
        cond = torch.from_numpy(rng.uniform((B, 1, H, H), 6, 1, 0.0, 2.0))
        mask = band_mask(B, H, H // 4)
        kw = dict(data=data, branch_out=True, start_intermediate=True, start_timestep=2, mask_x=True)
        ref_out, _, sd = run_pair(ddpm, cfg, base_config(**kw), T, None, B, H, cond, mask, (0.0, 2.0))
        orc = oracle_run(cfg, sd, base_config(**kw), T, None, B, H, cond, mask, (0.0, 2.0))
        compare("G6 " + tag, ref_out, orc, 2e-5)
        out[tag + "_final"] = to_np(ref_out)
    save("g6_branch_fusion", **out)


def g7(ddpm):
    print("G7 DDIM S=50 of T=1000, 64x64 1-ch, branch + fusion; and S=10 of T=50 no-fusion (list)")
    cfg, H, B = CFG_MRI, 64, 1
    cond = torch.from_numpy(rng.uniform((B, 1, H, H), 7, 1, 0.0, 2.0))
    mask = torch.zeros(B, 1, H, H)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(H), indexing="ij")
    mask[:, :, ((yy - H // 2) ** 2 + (xx - H // 2) ** 2) <= (H // 8) ** 2] = 1.0
    out = {"mask": mask.numpy()}
    kw = dict(data="mri", branch_out=True, start_intermediate=True, start_timestep=2, mask_x=True)
    ref_out, _, sd = run_pair(ddpm, cfg, base_config(**kw), 1000, 50, B, H, cond, mask, (0.0, 2.0))
    orc = oracle_run(cfg, sd, base_config(**kw), 1000, 50, B, H, cond, mask, (0.0, 2.0))
    compare("G7 fused", ref_out, orc, 2e-5)
    out["fused_final"] = to_np(ref_out)
    kw = dict(data="mri", branch_out=True, start_intermediate=False, mask_x=True)
    ref_out, _, sd = run_pair(ddpm, cfg, base_config(**kw), 50, 10, B, H, cond, mask, (0.0, 2.0))
    orc = oracle_run(cfg, sd, base_config(**kw), 50, 10, B, H, cond, mask, (0.0, 2.0))
    compare("G7 nofuse", ref_out, orc, 2e-5)
    out["nofuse_final"] = to_np(ref_out)
    kw = dict(data="mri")
    ref_out, _, sd = run_pair(ddpm, cfg, base_config(**kw), 50, 10, B, H, cond, None, (0.0, 2.0))
    orc = oracle_run(cfg, sd, base_config(**kw), 50, 10, B, H, cond, None, (0.0, 2.0))
    compare("G7 single", ref_out, orc, 2e-5)
    out["single_final"] = to_np(ref_out)
    save("g7_ddim", **out)


def g8(ddpm):
    print("G8 all-ones mask fallback + pred_noise / pred_v objectives (non-branch)")
    cfg, H, B, T = CFG_MNIST, 28, 2, 20
    cond = torch.from_numpy(rng.uniform((B, 1, H, H), 8, 1, 0.0, 2.0))
    out = {}
    kw = dict(data="mnist", branch_out=True, start_intermediate=True, start_timestep=2, mask_x=True)
    ones = torch.ones(B, 1, H, H)
    ref_out, _, sd = run_pair(ddpm, cfg, base_config(**kw), T, None, B, H, cond, ones, (0.0, 2.0))
    orc = oracle_run(cfg, sd, base_config(**kw), T, None, B, H, cond, ones, (0.0, 2.0))
    compare("G8 all-ones", ref_out, orc, 1e-5)
    out["allones_final"] = to_np(ref_out)
    for obj in ("pred_noise", "pred_v"):
        kw = dict(data="mnist")
        ref_out, _, sd = run_pair(ddpm, cfg, base_config(**kw), T, None, B, H, cond, None, (0.0, 2.0),
                                  objective=obj)
        orc = oracle_run(cfg, sd, base_config(**kw), T, None, B, H, cond, None, (0.0, 2.0), objective=obj)
        compare("G8 " + obj, ref_out, orc, 1e-4)
        out[obj + "_final"] = to_np(ref_out)
    save("g8_fallback_objectives", **out)


class StubClassifier:
    """Deterministic stand-in for Classifier_PatchCore (ddpm.py:622-625, anomalib is not installed): same call
    convention -- x0 -> (score, _, _) -- rejecting (score -1) the first ``reject`` calls, then accepting (+1).
    Records the x0 it was shown."""
    def __init__(self, reject):
        self.reject, self.calls, self.seen = reject, 0, []

    def __call__(self, x0):
        self.calls += 1
        self.seen.append(x0.detach().clone().cpu())
        return (torch.tensor(-1.0 if self.calls <= self.reject else 1.0), None, None)


def g9(ddpm):
    print("G9 classifier-gated re-branching (fusion(), ddpm.py:883-916) with a stub classifier")
    out = {}
    for tag, cfg, H, data, reject in [("mnist28_reject2", CFG_MNIST, 28, "mnist", 2), ("mri32_reject3", CFG_MRI, 32, "mri", 3),
                                      ("mri32_reject_all", CFG_MRI, 32, "mri", 99)]:
        B, T = 2, 12
        cond = torch.from_numpy(rng.uniform((B, 1, H, H), 9, 1, 0.0, 2.0))
        mask = band_mask(B, H, H // 4)
        kw = dict(data=data, branch_out=True, start_intermediate=True, start_timestep=7, mask_x=True, classifier=True)
        sd = sd_torch(cfg)
        ref_model = build_reference_unet(ddpm, cfg, sd)
        gd = _ref_diffusion(ddpm, base_config(**kw), ref_model, H, T, "sigmoid", "pred_x0", None).eval()
        stub = StubClassifier(reject)
        gd.classifier = stub
        noise = PortableNoise(10)
        with reference_run(noise):
            with torch.inference_mode():
                ref_out = gd.sample(cond.clone(), None, batch_size=B, mask=mask.clone(), min_max_val=(0.0, 2.0))
        o = opts_from(base_config(**kw), T)
        smp = diffusion_ref.RefSampler(diffusion_ref.make_model_fn(sd, cfg), o, cfg.channels, H)
        stub2 = StubClassifier(reject)
        smp.classifier = stub2
        with torch.no_grad():
            orc = smp.sample(cond, mask, (0.0, 2.0), B, PortableNoise(10))
        compare("G9 " + tag, ref_out, orc, 2e-5)
        assert stub.calls == stub2.calls, (stub.calls, stub2.calls)
        for a, b in zip(stub.seen, stub2.seen):
            assert maxdiff(a, b) <= 2e-5
        print(f"    classifier calls: {stub.calls}")
        out[tag + "_final"] = to_np(ref_out)
        out[tag + "_calls"] = np.array([stub.calls, reject])
        if tag == "mnist28_reject2":
            out["cond28"], out["mask28"] = cond.numpy(), mask.numpy()
        elif tag == "mri32_reject3":
            out["cond32"], out["mask32"] = cond.numpy(), mask.numpy()
    save("g9_classifier_gate", **out)


def g10(ddpm):
    print("G10 use_gt start (ddpm.py:937-944) and return_all_timesteps / return_all_outputs (:946,959-977,1072)")
    out = {}

    def both(cfg, H, config, T, S, B, cond, mask, hr, rat, rao):
        sd = sd_torch(cfg)
        ref_model = build_reference_unet(ddpm, cfg, sd)
        gd = _ref_diffusion(ddpm, dict(config), ref_model, H, T, "sigmoid", "pred_x0", S).eval()
        with reference_run(PortableNoise(10)):
            with torch.inference_mode():
                ref = gd.sample(cond.clone(), None if hr is None else hr.clone(), batch_size=B,
                                mask=None if mask is None else mask.clone(), min_max_val=(0.0, 2.0),
                                return_all_timesteps=rat, return_all_outputs=rao)
        o = opts_from(config, T, S)
        smp = diffusion_ref.RefSampler(diffusion_ref.make_model_fn(sd, cfg), o, cfg.channels, H)
        with torch.no_grad():
            orc = smp.sample(cond, mask, (0.0, 2.0), B, PortableNoise(10), gt=hr, return_all_timesteps=rat,
                             return_all_outputs=rao)
        return ref, orc

    def flat_x0(lst):
        """x_start_lst -> one array [steps, (2,) B, C, H, W] per homogeneous run of entries"""
        pairs = [np.stack([e[0].numpy(), e[1].numpy()]) for e in lst if isinstance(e, (list, tuple))]
        singles = [e.numpy() for e in lst if not isinstance(e, (list, tuple))]
        return (np.stack(pairs) if pairs else np.zeros((0,), np.float32)), (np.stack(singles) if singles else np.zeros((0,), np.float32))

    # (a) single-branch, use_gt start at t0 = 20 of T = 50, every x_t and every x0 returned
    B, H, T = 2, 28, 50
    cond = torch.from_numpy(rng.uniform((B, 1, H, H), 10, 1, 0.0, 2.0))
    hr = torch.from_numpy(rng.uniform((B, 1, H, H), 10, 2, 0.0, 2.0))
    kw = base_config(data="mnist", start_intermediate=True, use_gt=True, use_gt_timestep=20)
    (r_ret, r_x0, r_cm), (o_ret, o_x0, o_cm) = both(CFG_MNIST, H, kw, T, None, B, cond, None, hr, True, True)
    compare("G10a x_t history", r_ret, o_ret, 2e-5)
    assert tuple(r_ret.shape) == (B, 21, 1, H, H) and len(r_x0) == len(o_x0) == 20 and r_cm == [] and o_cm == []
    for a, b in zip(r_x0, o_x0):
        assert maxdiff(a, b) <= 2e-5
    out["a_cond"], out["a_hr"], out["a_hist"] = cond.numpy(), hr.numpy(), to_np(r_ret)
    out["a_x0"] = np.stack([e.numpy() for e in r_x0])
    # (b) branch + fusion from a use_gt start, x0 history (pairs for the branch steps, then fused / joint x0)
    B, H, T = 2, 32, 40
    cond = torch.from_numpy(rng.uniform((B, 1, H, H), 10, 3, 0.0, 2.0))
    hr = torch.from_numpy(rng.uniform((B, 1, H, H), 10, 4, 0.0, 2.0))
    mask = band_mask(B, H, H // 4)
    kw = base_config(data="mri", branch_out=True, start_intermediate=True, start_timestep=3, mask_x=True, use_gt=True,
                     use_gt_timestep=12)
    (r_ret, r_x0, _), (o_ret, o_x0, _) = both(CFG_MRI, H, kw, T, None, B, cond, mask, hr, False, True)
    compare("G10b final", r_ret, o_ret, 2e-5)
    assert len(r_x0) == len(o_x0) == 12
    for a, b in zip(r_x0, o_x0):
        assert isinstance(a, (list, tuple)) == isinstance(b, (list, tuple))
        assert maxdiff(torch.from_numpy(to_np(a)), torch.from_numpy(to_np(b))) <= 2e-5
    out["b_cond"], out["b_hr"], out["b_mask"], out["b_final"] = cond.numpy(), hr.numpy(), mask.numpy(), to_np(r_ret)
    out["b_x0_pairs"], out["b_x0_single"] = flat_x0(r_x0)
    assert out["b_x0_pairs"].shape[0] == 8 and out["b_x0_single"].shape[0] == 4      # t = 11..4 branch, 3 fusion, 2..0 joint
    # (c) DDIM, single branch, every x_t returned
    B, H, T, S = 2, 28, 50, 10
    cond = torch.from_numpy(rng.uniform((B, 1, H, H), 10, 5, 0.0, 2.0))
    kw = base_config(data="mnist")
    r_ret, o_ret = both(CFG_MNIST, H, kw, T, S, B, cond, None, None, True, False)
    compare("G10c DDIM x_t history", r_ret, o_ret, 2e-5)
    assert tuple(r_ret.shape) == (B, S + 1, 1, H, H)
    out["c_cond"], out["c_hist"] = cond.numpy(), to_np(r_ret)
    # (d) return_all_timesteps with branches: the reference's torch.stack raises; record the exception type
    kw = base_config(data="mri", branch_out=True, start_intermediate=True, start_timestep=3, mask_x=True)
    for S_ in (None, 10):
        try:
            both(CFG_MRI, 32, kw, 40, S_, 2, torch.from_numpy(rng.uniform((2, 1, 32, 32), 10, 3, 0.0, 2.0)), band_mask(2, 32, 8), None, True, False)
            raise AssertionError("expected the reference to fail")
        except TypeError as e:
            print(f"    branch + return_all_timesteps (S={S_}): reference raises TypeError ({str(e)[:60]}...)")
    save("g10_use_gt_return_all", **out)


def g11(ddpm):
    """The floor of ANY 16-bit-storage implementation on cfg2: the reference's own fp32 code with nothing but its
    denoiser OUTPUT rounded to bf16 / fp16 once per step (an implementation that stores activations in 16 bits rounds
    hundreds of tensors per step).  The distance of these runs from the fp32 golden G5 is the yardstick the
    16-bit chain tests price the HIP path against (tests/test_hip_lowp_chain.py)."""
    print("G11 cfg2 with the reference's denoiser output rounded to 16 bits once per step  (several minutes)")
    cfg, H, B, T = CFG_MRI, 128, 1, 1000
    cond = torch.from_numpy(rng.uniform((B, 1, H, H), 5, 1, 0.0, 2.0))
    g5_ = np.load(os.path.join(GOLD, "g5_cfg2_mri128.npz"))
    out = {}
    keep = (999, 750, 500, 250, 100, 10, 0)
    for tag, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        sd = sd_torch(cfg)
        ref_model = build_reference_unet(ddpm, cfg, sd)
        inner = ref_model.forward
        ref_model.forward = lambda *a, _f=inner, _dt=dt, **k: _f(*a, **k).to(_dt).to(torch.float32)
        gd = _ref_diffusion(ddpm, base_config(data="mri"), ref_model, H, T, "sigmoid", "pred_x0", None).eval()
        t0 = time.time()
        with reference_run(PortableNoise(10)):
            with torch.inference_mode():
                hist = gd.sample(cond.clone(), None, batch_size=B, mask=None, min_max_val=(0.0, 2.0), return_all_timesteps=True)
        hist = hist.numpy()
        print(f"  {tag}: reference sample() wall {time.time()-t0:.1f}s")
        for t in keep:
            d = np.abs(hist[:, T - t] - g5_[f"x_after_t{t}"])
            print(f"    output rounded to {tag}: x after t={t}: max-abs {d.max():.3e} mean-abs {d.mean():.3e}")
            out[f"{tag}_x_after_t{t}"] = hist[:, T - t]
    save("g11_cfg2_output_rounded", **out)


def g12(ddpm):
    """Checkpoint format pinned to what the reference's own Trainer.save writes (ddpm.py:1495-1507) and
    Trainer.load reads (:1509-1527).  Both methods are called unbound on a minimal trainer object holding a real
    accelerate.Accelerator, the reference GaussianDiffusion, an Adam optimiser and an EMA wrapper (ema_pytorch is
    absent from this image: the stand-in has the package's state_dict layout -- online_model.*, ema_model.*,
    initted, step).  The file is ~40 MB of procedural weights, so what is committed is its MANIFEST (every key with
    shape and dtype); tests rebuild the file with checkpoint.save_reference_checkpoint and compare manifests."""
    import copy
    import json
    import pathlib
    from accelerate import Accelerator
    from localdiffusion_hallucination_amd import checkpoint
    print("G12 Trainer.save / Trainer.load checkpoint format")
    cfg, H, T = CFG_MNIST, 28, 100
    sd = sd_torch(cfg, 3)
    ref_model = build_reference_unet(ddpm, cfg, sd)
    kw = base_config(data="mnist", branch_out=True, start_intermediate=True, start_timestep=2, mask_x=True)
    gd = _ref_diffusion(ddpm, kw, ref_model, H, T, "sigmoid", "pred_x0", None)

    class EMA(torch.nn.Module):
        def __init__(self, model):
            super().__init__()
            self.online_model = model
            self.ema_model = copy.deepcopy(model)
            self.register_buffer("initted", torch.tensor(True))
            self.register_buffer("step", torch.tensor(0))

    def manifest(data):
        def walk(d):
            return {k: ([list(v.shape), str(v.dtype)] if torch.is_tensor(v) else walk(v) if isinstance(v, dict) else type(v).__name__)
                    for k, v in d.items()}
        m = {k: (walk(v) if isinstance(v, dict) else type(v).__name__) for k, v in data.items()}
        m["opt"] = "dict"                      # optimiser state is training-side, not read by the sampling path
        return m

    with tempfile.TemporaryDirectory() as d:
        tr = types.SimpleNamespace(accelerator=Accelerator(cpu=True), model=gd, opt=torch.optim.Adam(gd.parameters(), lr=1e-4),
                                   ema=EMA(gd), step=2900, results_folder=pathlib.Path(d))
        ddpm.Trainer.save(tr, "best2900")                     # the reference's own writer
        path = os.path.join(d, "model-best2900.pt")
        data = torch.load(path, map_location="cpu", weights_only=True)      # loads under the safe unpickler
        man = manifest(data)
        # the product reads what the reference wrote ...
        net = ldh.Unet(dim=32, init_dim=32, dim_mults=cfg.dim_mults, full_attn=cfg.full_attn, mode=cfg.mode)
        mine = ldh.GaussianDiffusion(dict(kw), net, image_size=H, timesteps=T, objective="pred_x0")
        info = checkpoint.load_reference_checkpoint(path, mine)
        assert info == {"step": 2900, "source": "ema", "missing": [], "unexpected": []}, info
        for k, v in gd.state_dict().items():
            assert torch.equal(mine.state_dict()[k], v), k
        # ... and the reference reads what the product writes (Trainer.load on a second trainer object)
        path2 = os.path.join(d, "model-mine.pt")
        checkpoint.save_reference_checkpoint(mine, path2, step=2900)
        assert manifest(torch.load(path2, map_location="cpu", weights_only=True)) == man
        gd2 = _ref_diffusion(ddpm, kw, build_reference_unet(ddpm, cfg, sd_torch(cfg, 4)), H, T, "sigmoid", "pred_x0", None)
        tr2 = types.SimpleNamespace(accelerator=Accelerator(cpu=True), model=gd2, opt=torch.optim.Adam(gd2.parameters(), lr=1e-4),
                                    ema=EMA(gd2), step=0, results_folder=pathlib.Path(d))
        with contextlib.redirect_stdout(io.StringIO()):
            ddpm.Trainer.load(tr2, "mine")
        assert tr2.step == 2900
        for k, v in gd.state_dict().items():
            assert torch.equal(gd2.state_dict()[k], v), k
    with open(os.path.join(GOLD, "g12_trainer_save_manifest.json"), "w") as f:
        json.dump(man, f, indent=0, sort_keys=True)
    print(f"  wrote tests/golden/g12_trainer_save_manifest.json ({len(man['model'])} model keys, {len(man['ema'])} ema keys)")


def g13(ddpm):
    """How far the REFERENCE is from ITSELF on cfg2 when only its summation order changes: the same code, weights and
    noise with torch.set_num_threads(1) instead of all cores (MKL-DNN / ATen split reductions differently).  This is the
    reproducibility floor of the 1e-3 gate: any fp32 implementation that sums in another order sits at this distance."""
    print("G13 cfg2 on ONE thread vs the golden made on all cores  (tens of minutes)")
    cfg, H, B, T = CFG_MRI, 128, 1, 1000
    cond = torch.from_numpy(rng.uniform((B, 1, H, H), 5, 1, 0.0, 2.0))
    g5_ = np.load(os.path.join(GOLD, "g5_cfg2_mri128.npz"))
    sd = sd_torch(cfg)
    ref_model = build_reference_unet(ddpm, cfg, sd)
    gd = _ref_diffusion(ddpm, base_config(data="mri"), ref_model, H, T, "sigmoid", "pred_x0", None).eval()
    n0 = torch.get_num_threads()
    torch.set_num_threads(1)
    t0 = time.time()
    try:
        with reference_run(PortableNoise(10)):
            with torch.inference_mode():
                hist = gd.sample(cond.clone(), None, batch_size=B, mask=None, min_max_val=(0.0, 2.0), return_all_timesteps=True).numpy()
    finally:
        torch.set_num_threads(n0)
    print(f"  reference sample() on 1 thread: wall {time.time()-t0:.1f}s")
    out = {}
    for t in (999, 750, 500, 250, 100, 10, 0):
        d = np.abs(hist[:, T - t] - g5_[f"x_after_t{t}"])
        print(f"    1 thread vs {n0} threads: x after t={t}: max-abs {d.max():.3e} mean-abs {d.mean():.3e}")
        out[f"maxabs_t{t}"] = np.float64(d.max())
        out[f"meanabs_t{t}"] = np.float64(d.mean())
    out["final_1thread"] = hist[:, -1]
    out["threads"] = np.array([1, n0])
    save("g13_cfg2_reference_self_distance", **out)


G16_GAIN = 0.25


def g16(ddpm):
    """The end-to-end pin of the 16-bit storage modes: cfg2's shape and schedule (128x128 1-ch, T = 1000,
    fp32, non-branch) run by the REAL reference on a CONTRACTIVE procedural denoiser -- the same weights with final_conv's
    gain 0.25 instead of 3 (weights.procedural_state_dict(final_gain=...)).  With gain 3 the last 100 steps of the chain
    amplify any perturbation x40-170 (G11 / G13: a random-init net's prediction swings over the whole range whatever x_t
    is), so the final-image distance of a 16-bit run says nothing about the implementation; with gain 0.25 the same
    perturbation (weights rounded to bf16) grows x1.7 in the mean from t = 100 to t = 0 and not at all over the last 10
    steps (tools/exp_contractive.py), as for a trained denoiser whose prediction at small t stays near x_t.  Stored: the
    states after t = 999, 750, 500, 250, 100, 10, 0, the oracle checked bit for bit, and the reference's own 1-thread
    self-distance on this net (the floor any other summation order has)."""
    print("G16 cfg2 shape on the contractive procedural net (final_conv gain 0.25)  (tens of minutes)")
    cfg, H, B, T = CFG_MRI, 128, 1, 1000
    cond = torch.from_numpy(rng.uniform((B, 1, H, H), 5, 1, 0.0, 2.0))
    sd = {k: torch.from_numpy(v) for k, v in weights.procedural_state_dict(cfg, 0, final_gain=G16_GAIN).items()}
    keep = (999, 750, 500, 250, 100, 10, 0)
    out = {}

    def ref_hist(threads):
        ref_model = build_reference_unet(ddpm, cfg, sd)
        gd = _ref_diffusion(ddpm, base_config(data="mri"), ref_model, H, T, "sigmoid", "pred_x0", None).eval()
        n0 = torch.get_num_threads()
        torch.set_num_threads(threads)
        t0 = time.time()
        try:
            with reference_run(PortableNoise(10)):
                with torch.inference_mode():
                    h = gd.sample(cond.clone(), None, batch_size=B, mask=None, min_max_val=(0.0, 2.0), return_all_timesteps=True).numpy()
        finally:
            torch.set_num_threads(n0)
        print(f"  reference sample() on {threads} threads: wall {time.time()-t0:.1f}s")
        return h
    hist = ref_hist(os.cpu_count())
    recs = {}
    orc = oracle_run(cfg, sd, base_config(data="mri"), T, None, B, H, cond, None, (0.0, 2.0),
                     record=lambda t, x: recs.__setitem__(t, to_np(x)) if t in keep else None)
    compare("G16", torch.from_numpy(hist[:, -1]), orc, 1e-4)
    for t in keep:
        assert maxdiff(torch.from_numpy(hist[:, T - t]), torch.from_numpy(recs[t])) == 0.0, t
        out[f"x_after_t{t}"] = hist[:, T - t]
    out["final"] = hist[:, -1]
    h1 = ref_hist(1)
    for t in keep:
        d = np.abs(h1[:, T - t] - hist[:, T - t])
        print(f"    1 thread vs {os.cpu_count()} threads: x after t={t}: max-abs {d.max():.3e} mean-abs {d.mean():.3e}")
        out[f"self_maxabs_t{t}"] = np.float64(d.max())
        out[f"self_meanabs_t{t}"] = np.float64(d.mean())
    out["final_gain"] = np.float64(G16_GAIN)
    print(f"  x_0 range [{hist[:, -1].min():.3f}, {hist[:, -1].max():.3f}] std {hist[:, -1].std():.4f}")
    save("g16_cfg2_contractive", **out)


def g14(ddpm):
    """Two (or three) consecutive sample() calls on ONE GaussianDiffusion object.  The reference clears
    config['mask_x'] at the fusion step (ddpm.py:780-781, 1023-1024) and in the all-ones fallback (:1114) and
    re-arms it in sample() only under ood_AD / ood_confidence (:1106-1108), so with {mask_x: True, ood_AD: False}
    the SECOND call runs its branch steps without masking the OOD prediction.  Every call gets a fresh portable
    noise stream (DDPM re-seeds per call, :934; for DDIM that is this fixture's convention)."""
    print("G14 consecutive sample() calls on one object (mask_x call state), DDPM and DDIM")
    cfg, H, B = CFG_MRI, 32, 2
    cond = torch.from_numpy(rng.uniform((B, 1, H, H), 14, 1, 0.0, 2.0))
    band, ones = band_mask(B, H, H // 4), torch.ones(B, 1, H, H)
    out = {"cond": cond.numpy(), "band": band.numpy()}
    fuse = dict(data="mri", branch_out=True, start_intermediate=True, start_timestep=2)
    cases = [("ddpm_maskx", dict(fuse, mask_x=True), 50, None, [band, band]),
             ("ddpm_oodad", dict(fuse, ood_AD=True), 50, None, [band, band]),
             ("ddpm_ones_then_band", dict(fuse, mask_x=True), 50, None, [ones, band]),
             ("ddim_maskx", dict(fuse, mask_x=True), 50, 10, [band, band]),
             ("ddim_oodad", dict(fuse, ood_AD=True), 50, 10, [band, band])]
    for tag, kw, T, S, masks in cases:
        sd = sd_torch(cfg)
        gd = _ref_diffusion(ddpm, base_config(**kw), build_reference_unet(ddpm, cfg, sd), H, T, "sigmoid", "pred_x0", S).eval()
        smp = diffusion_ref.RefSampler(diffusion_ref.make_model_fn(sd, cfg), opts_from(base_config(**kw), T, S), cfg.channels, H)
        refs = []
        for i, m in enumerate(masks):
            with reference_run(PortableNoise(10)):
                with torch.inference_mode():
                    r = gd.sample(cond.clone(), None, batch_size=B, mask=m.clone(), min_max_val=(0.0, 2.0))
            with torch.no_grad():
                o = smp.sample(cond, m, (0.0, 2.0), B, PortableNoise(10))
            compare(f"G14 {tag} call {i + 1}", r, o, 2e-5)
            refs.append(to_np(r))
            out[f"{tag}_call{i + 1}"] = to_np(r)
        d = float(np.abs(refs[-1] - refs[0]).max()) if refs[-1].shape == refs[0].shape else float("nan")
        print(f"    last call vs first call: max-abs {d:.3e}")
        if tag.endswith("_maskx"):
            assert d > 1e-3, "the second call should differ (mask_x is disarmed by the first call's fusion step)"
        if tag.endswith("_oodad"):
            assert d == 0.0, "ood_AD re-arms mask_x: both calls must agree"
    save("g14_consecutive_calls", **out)


def g15(ddpm):
    print("G15 training-side forward: GaussianDiffusion.forward / p_losses (ddpm.py:1156-1214), three objectives")
    out = {}
    for tag, cfg, H, B in (("mnist28", CFG_MNIST, 28, 4), ("mri32", CFG_MRI, 32, 2)):
        sd = sd_torch(cfg)
        x0 = torch.from_numpy(rng.uniform((B, 1, H, H), 15, 1, 0.0, 2.0))
        cond = torch.from_numpy(rng.uniform((B, 1, H, H), 15, 2, 0.0, 2.0))
        out[tag + "_x0"], out[tag + "_cond"] = to_np(x0), to_np(cond)
        for obj in ("pred_x0", "pred_noise", "pred_v"):
            T = 100
            ref_model = build_reference_unet(ddpm, cfg, sd)
            gd = _ref_diffusion(ddpm, base_config(data="mnist" if cfg is CFG_MNIST else "mri"), ref_model, H, T, "sigmoid", obj, None).eval()
            # (a) forward(img, cond, train=False): the reference seeds torch's generator with 42 and draws t with torch.randint
            noise = PortableNoise(10)
            with reference_run(noise):
                with torch.inference_mode():
                    loss_fwd = gd(x0.clone(), cond.clone(), False)
            torch.random.manual_seed(42)
            t_fwd = torch.randint(0, T, (B,)).long()
            # (b) p_losses with explicit timesteps (first / middle / last) and offset noise
            t_exp = torch.tensor(([0, T // 2, T - 1, 7] * B)[:B])
            noise = PortableNoise(10)
            with reference_run(noise):
                with torch.inference_mode():
                    loss_exp = gd.p_losses(x0.clone(), cond.clone(), t_exp, offset_noise_strength=0.1)
            # oracle restatement on the same draws
            o = opts_from(base_config(), T, None, obj)
            smp = diffusion_ref.RefSampler(diffusion_ref.make_model_fn(sd, cfg), o, 1, H)
            pn = PortableNoise(10)
            with torch.no_grad():
                o_fwd, per_fwd = smp.p_losses(x0, cond, t_fwd, pn.randn_like(x0))
                pn = PortableNoise(10)
                n1 = pn.randn_like(x0)
                off = pn.randn(B, 1)
                o_exp, per_exp = smp.p_losses(x0, cond, t_exp, n1, offset_noise=off, offset_noise_strength=0.1)
            d1, d2 = abs(float(loss_fwd) - float(o_fwd)), abs(float(loss_exp) - float(o_exp))
            print(f"  {tag} {obj}: forward loss {float(loss_fwd):.6e} (t = {t_fwd.tolist()}), p_losses {float(loss_exp):.6e}; "
                  f"oracle-vs-reference {d1:.3e} / {d2:.3e}")
            assert d1 <= 1e-6 * max(1.0, abs(float(loss_fwd))) and d2 <= 1e-6 * max(1.0, abs(float(loss_exp)))
            out[f"{tag}_{obj}_t_fwd"], out[f"{tag}_{obj}_loss_fwd"] = t_fwd.numpy(), np.float32(float(loss_fwd))
            out[f"{tag}_{obj}_per_fwd"] = to_np(per_fwd)
            out[f"{tag}_{obj}_t_exp"], out[f"{tag}_{obj}_loss_exp"] = t_exp.numpy(), np.float32(float(loss_exp))
            out[f"{tag}_{obj}_per_exp"] = to_np(per_exp)
    save("g15_p_losses", **out)


def g0_inventory(ddpm):
    print("G0 parameter inventory")
    lines = []
    for tag, cfg in [("mnist", CFG_MNIST), ("mri", CFG_MRI), ("mvtec", CFG_MVTEC)]:
        sd = sd_torch(cfg)
        build_reference_unet(ddpm, cfg, sd)
        n = sum(v.numel() for v in sd.values())
        lines.append(f"{tag} {len(sd)} {n}")
        print("  ", lines[-1])
    with open(os.path.join(GOLD, "g0_inventory.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def g17(ddpm):
    """The reference's remaining Unet constructor options (ddpm.py:294-300), which no shipped caller sets: learned_variance
    (out_dim doubles, :394), learned_sinusoidal_cond / random_fourier_features (RandomOrLearnedSinusoidalPosEmb, :151-165) and
    self_condition (accepted by the constructor; the forward then fails in init_conv, :406-413).  Forward outputs of the real
    reference with the first two on, on the MNIST-shaped net; the oracle must reproduce them."""
    print("G17 Unet constructor options: learned_variance + learned Fourier time features; self_condition")
    cfg = weights.UnetConfig(dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist", out_dim=2, learned_sinusoidal_dim=16)
    sd = sd_torch(cfg)
    out = {}
    for tag, kw in (("learned", dict(learned_sinusoidal_cond=True)), ("random", dict(random_fourier_features=True))):
        ref = ddpm.Unet(dim=cfg.dim, init_dim=cfg.init_dim, dim_mults=cfg.dim_mults, channels=cfg.channels, full_attn=cfg.full_attn,
                        mode=cfg.mode, learned_variance=True, learned_sinusoidal_dim=16, **kw)
        assert ref.out_dim == 2 and ref.random_or_learned_sinusoidal_cond
        ref_sd = ref.state_dict()
        assert list(ref_sd.keys()) == list(sd.keys()), set(ref_sd) ^ set(sd)
        for k in ref_sd:
            assert tuple(ref_sd[k].shape) == tuple(sd[k].shape), k
        ref.load_state_dict(sd)
        ref.eval()
        B, H = 2, 28
        x = torch.from_numpy(rng.randn((B, 1, H, H), 17, 100))
        cond = torch.from_numpy(rng.uniform((B, 1, H, H), 17, 101, 0.0, 2.0))
        for t in (0, 7, 99):
            tv = torch.full((B,), t, dtype=torch.long)
            with torch.no_grad():
                y_ref = ref(x, cond, tv)
                y_orc = unet_ref.unet_forward(sd, cfg, x, cond, tv)
            d = maxdiff(y_ref, y_orc)
            print(f"  {tag} t={t}: out {tuple(y_ref.shape)}, oracle-vs-reference {d:.2e}")
            assert tuple(y_ref.shape) == (B, 2, H, H) and d <= 1e-5, (tag, t, d)
            if tag == "learned":
                out[f"t{t}_out"] = y_ref.numpy()
        try:                          # the reference's own GaussianDiffusion refuses both (ddpm.py:515-516)
            _ref_diffusion(ddpm, base_config(data="mnist"), ref, H, 10, "sigmoid", "pred_x0", None)
            raise SystemExit("GaussianDiffusion accepted a learned-variance / learned-sinusoidal Unet")
        except AssertionError:
            pass
    sc = ddpm.Unet(dim=32, init_dim=32, dim_mults=cfg.dim_mults, channels=1, full_attn=cfg.full_attn, mode="mnist", self_condition=True)
    try:
        with torch.no_grad():
            sc(x, cond, torch.zeros(B, dtype=torch.long))
        raised = ""
    except RuntimeError as e:
        raised = str(e)
    print("  self_condition=True forward:", raised[:120] or "no error")
    assert "channels" in raised
    out["selfcond_forward_raises"] = np.array([1])
    out["shape"] = np.array([B, 1, H, 1])
    save("g17_unet_options", **out)


# config.yaml:55-56: the MRI intensity normalisation that test.py:213-216 undoes in front of the segmentation net
MEAN_T1, STD_T1 = 610.7180906353575, 1018.7631901605115
SEG_SEED = 18


def mri_like_slices(B, H, seed):
    """Synthetic MRI-like LR slices in the translated units test.py feeds the net (background 0): an elliptical head with a
    smooth low-frequency texture and one bright blob (the 'lesion').  [B, 1, H, H] float32."""
    yy, xx = np.mgrid[0:H, 0:H].astype(np.float64) / H
    out = np.zeros((B, 1, H, H), np.float32)
    for b in range(B):
        u = rng.uniform((12,), seed, 1800 + b, 0.0, 1.0).astype(np.float64)
        cy, cx = 0.5 + 0.08 * (u[0] - 0.5), 0.5 + 0.08 * (u[1] - 0.5)
        r = np.sqrt(((yy - cy) / (0.36 + 0.04 * u[2])) ** 2 + ((xx - cx) / (0.30 + 0.04 * u[3])) ** 2)
        head = 1.0 / (1.0 + np.exp((r - 1.0) * 25.0))
        tex = 0.9 + 0.15 * np.sin(2 * np.pi * (2 + 2 * u[4]) * yy + 6.28 * u[5]) * np.cos(2 * np.pi * (1 + 2 * u[6]) * xx + 6.28 * u[7])
        by, bx = cy + 0.35 * (u[8] - 0.5), cx + 0.3 * (u[9] - 0.5)
        rb = np.sqrt((yy - by) ** 2 + (xx - bx) ** 2) / (0.06 + 0.05 * u[10])
        blob = (2.0 + u[11]) / (1.0 + np.exp((rb - 1.0) * 8.0))
        out[b, 0] = (head * tex + head * blob).astype(np.float32)
    return out


def g18(ddpm):
    """The reference's segmentation U-Net (unet_model.py:140-243, UNet() as test.py:218 builds it) with the procedural
    weights of weights.procedural_seg_state_dict and BatchNorm running statistics calibrated the way train_seg.py would
    leave them (train mode, cumulative averages over procedural batches, no optimiser); then the reference's own forward
    on four inputs.  The 128^2 slice is chosen so that no logit sits within 1e-3 of the largest one of zero (its mask is
    unambiguous), and it holds both classes."""
    print("G18 segmentation U-Net (OOD-mask producer)")
    import unet_model
    ref = unet_model.UNet()
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_seg_state_dict(SEG_SEED).items()}
    ref_sd = ref.state_dict()
    assert list(ref_sd.keys()) == list(sd.keys()), set(ref_sd) ^ set(sd)
    for k in ref_sd:
        assert tuple(ref_sd[k].shape) == tuple(sd[k].shape) and ref_sd[k].dtype == sd[k].dtype, k
    ref.load_state_dict(sd)
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = None                     # cumulative moving average
    ref.train()
    mini = abs((0 - MEAN_T1) / STD_T1)
    with torch.no_grad():
        for k in range(4):
            xb = torch.from_numpy(mri_like_slices(4, 64, 180 + k)) - mini
            xb = xb + 0.05 * torch.from_numpy(rng.randn(tuple(xb.shape), SEG_SEED, 1900 + k))
            ref(xb)
    ref.eval()
    # The head bias is calibrated too: moved (by at most 0.25) into the widest gap of the 128^2 slice's logits around zero,
    # so that the slice's mask is unambiguous -- no logit within 1e-4 of the largest one of the 0.5-probability threshold
    # (the logits of a random-weight net are spatially rough: without this, some of 16384 pixels always sit at ~1e-5).
    mini_t = torch.abs(torch.tensor((0 - MEAN_T1) / STD_T1))                    # test.py:215
    b0 = float(ref.outc.conv.bias[0])
    best = None
    with torch.no_grad():
        for c in range(16):                                                       # first slice with a wide enough gap
            lr = torch.from_numpy(mri_like_slices(1, 128, 128000 + c))
            feat = (ref(lr - mini_t) - b0).numpy().ravel().astype(np.float64)
            cand = np.sort(-feat[(-feat > b0 - 0.25) & (-feat < b0 + 0.25)])
            i = int(np.argmax(np.diff(cand)))
            bias, half = float(np.float32((cand[i] + cand[i + 1]) / 2)), (cand[i + 1] - cand[i]) / 2
            best = (lr, bias)
            if half > 2e-4 * np.abs(feat + bias).max():
                break
        lr128, bias = best
        ref.outc.conv.bias.fill_(bias)
    out = {"mean_t1": np.float64(MEAN_T1), "std_t1": np.float64(STD_T1), "seed": np.int64(SEG_SEED)}
    for k, v in ref.state_dict().items():
        if "running_" in k or k.endswith("num_batches_tracked") or k == "outc.conv.bias":
            out[k] = v.numpy().copy()
    with torch.no_grad():
        x32 = torch.from_numpy(mri_like_slices(2, 32, 32)) - mini
        x64 = torch.from_numpy(mri_like_slices(1, 64, 64)) - mini
        out["x32"], out["logits32"] = x32.numpy(), ref(x32).numpy()
        out["x64"], out["logits64"] = x64.numpy(), ref(x64).numpy()
        for H in (128, 256):
            lr = lr128 if H == 128 else torch.from_numpy(mri_like_slices(1, H, 1000 * H))
            lr_ad = lr - mini_t                                                   # test.py:216
            logits = ref(lr_ad)
            mask = (torch.sigmoid(logits) > 0.5).float()                          # test.py:287-288
            frac = float(mask.mean())
            lmin, lmax = float(logits.abs().min()), float(logits.abs().max())
            print(f"  {H}^2: logits in [{float(logits.min()):.3f}, {float(logits.max()):.3f}], min |logit| {lmin:.2e}, "
                  f"mask fraction {frac:.3f}")
            if H == 128:
                assert 0.02 < frac < 0.98 and lmin > 1e-4 * lmax, (frac, lmin, lmax)
            out[f"lr{H}"], out[f"logits{H}"], out[f"mask{H}"] = lr.numpy(), logits.numpy(), mask.numpy()
    for H, key in ((32, "logits32"), (64, "logits64")):
        print(f"  {H}^2 logits in [{out[key].min():.3f}, {out[key].max():.3f}]")
    save("g18_segunet", **out)
    with open(os.path.join(GOLD, "g18_segunet_inventory.txt"), "w") as f:
        for k, v in ref.state_dict().items():
            f.write(f"{k} {list(v.shape)} {str(v.dtype).replace('torch.', '')}\n")


SEG_TRAIN_BATCHES, SEG_TRAIN_B, SEG_TRAIN_H = 6, 4, 32


def seg_train_batches(seeds):
    """G19's batches: mri_like_slices shifted as G18 does, target = the slice's lesion (slice > 1.6)."""
    mini = abs((0 - MEAN_T1) / STD_T1)
    out = []
    for s in seeds:
        sl = mri_like_slices(SEG_TRAIN_B, SEG_TRAIN_H, s)
        out.append((torch.from_numpy(sl) - mini, torch.from_numpy((sl > 1.6).astype(np.float32))))
    return out


def g19(ddpm):
    """The reference's segmentation training step (train_seg.py:78-95): its own unet_model.UNet(), DiceLoss,
    BCEWithLogitsLoss(pos_weight=10) and torch.optim.Adam(lr=1e-3) on six batches of B = 4 at 32^2, in fp64 (the yardstick)
    and in fp32 in three arithmetic orders (the reference's own spread, which the whole-net tolerances of the GPU tests are
    multiples of).  Two files (each below the size limit): g19_segtrain.npz and g19_segtrain_grads.npz (the gradients of
    the tensors of at most 4,096 elements)."""
    print("G19 segmentation U-Net training step")
    import unet_model
    import train_seg
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import segtrain_ref
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_seg_state_dict(SEG_SEED).items()}

    def fresh(dtype, channels_last=False):
        m = unet_model.UNet()
        m.load_state_dict(sd)
        m = m.to(dtype)
        if channels_last:
            m = m.to(memory_format=torch.channels_last)
        for p in m.parameters():
            p.requires_grad = True
        return m.train()

    def criterion(m, x, t):
        pred = m(x)
        pw = torch.tensor([10]).to(pred.dtype)
        return torch.nn.BCEWithLogitsLoss(pos_weight=pw)(pred, t) + train_seg.DiceLoss()(torch.sigmoid(pred), t)

    def grads_at_init(dtype, x, t, channels_last=False, with_stats=False):
        m = fresh(dtype, channels_last)
        stats, hooks = {}, []
        if with_stats:
            for name, mod in m.named_modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    def hook(_m, inp, name=name):
                        stats[name + ".mean"] = inp[0].detach().mean(dim=(0, 2, 3)).numpy().copy()
                        stats[name + ".var"] = inp[0].detach().var(dim=(0, 2, 3), unbiased=False).numpy().copy()
                    hooks.append(mod.register_forward_pre_hook(hook))
        x, t = x.to(dtype), t.to(dtype)
        if channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        loss = criterion(m, x, t)
        loss.backward()
        return float(loss.detach()), [p.grad.detach().clone().contiguous() for p in m.parameters()], stats

    def six_steps(dtype, batches, channels_last=False):
        m = fresh(dtype, channels_last)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        losses, first = [], None
        for x, t in batches:
            opt.zero_grad()
            x, t = x.to(dtype), t.to(dtype)
            if channels_last:
                x = x.contiguous(memory_format=torch.channels_last)
            loss = criterion(m, x, t)
            loss.backward()
            opt.step()
            losses.append(float(loss))
            if first is None:
                first = {k: v.detach().clone().numpy() for k, v in m.state_dict().items()
                         if "running_" in k or k.endswith("num_batches_tracked")}
        return losses, first

    names = [k for k, _ in unet_model.UNet().named_parameters()]
    assert len(names) == 64
    orders = ("default", "channels_last", "onednn_off")

    def run_order(order, fn):
        if order == "onednn_off":
            with torch.backends.mkldnn.flags(enabled=False):
                return fn(False)
        return fn(order == "channels_last")

    probe_cache = {}
    for attempt in range(8):
        seeds = [190 + 10 * attempt + k for k in range(SEG_TRAIN_BATCHES)]
        batches = seg_train_batches(seeds)
        out = {"seeds": np.asarray(seeds, np.int64), "seed": np.int64(SEG_SEED),
               "x": np.stack([b[0].numpy() for b in batches]), "target": np.stack([b[1].numpy() for b in batches]).astype(np.uint8)}
        small = {}
        ref_grads = []
        losses0, norms, dots = [], np.zeros((SEG_TRAIN_BATCHES, 64)), np.zeros((SEG_TRAIN_BATCHES, 64, 4))
        for b, (x, t) in enumerate(batches):
            loss, grads, stats = grads_at_init(torch.float64, x, t, with_stats=True)
            losses0.append(loss)
            ref_grads.append(grads)
            for i, g in enumerate(grads):
                norms[b, i] = float(g.norm())
                dots[b, i] = segtrain_ref.probe_dots(i, g, probe_cache)
                if g.numel() <= 4096:
                    small[f"grad{b}.{names[i]}"] = g.numpy().copy()
            for k, v in stats.items():
                out[f"bn{b}.{k}"] = v
        out["loss_init"], out["grad_norm"], out["grad_dots"] = np.asarray(losses0), norms, dots
        losses64, first = six_steps(torch.float64, batches)
        out["loss_steps"] = np.asarray(losses64)
        for k, v in first.items():
            out["step1." + k] = v
        frac = float(np.mean(out["target"]))
        print(f"  seeds {seeds}: positives {100 * frac:.1f} %, fp64 losses {['%.4f' % l for l in losses64]}")
        grad_spread, loss_spread, clean = 0.0, 0.0, np.zeros((3, SEG_TRAIN_BATCHES), np.int64)
        first_loss_err = 0.0
        for o, order in enumerate(orders):
            for b, (x, t) in enumerate(batches):
                loss, grads, _ = run_order(order, lambda cl: grads_at_init(torch.float32, x, t, channels_last=cl))
                rel = [segtrain_ref.rel_l2(g, r) for g, r in zip(grads, ref_grads[b])]
                grad_spread = max(grad_spread, max(rel))
                clean[o, b] = sum(r <= 1e-4 for r in rel)
                first_loss_err = max(first_loss_err, abs(loss - losses0[b]))
            l32, _ = run_order(order, lambda cl: six_steps(torch.float32, batches, channels_last=cl))
            loss_spread = max(loss_spread, max(abs(a - c) for a, c in zip(l32, losses64)))
            print(f"  fp32 {order}: parameters within 1e-4 per batch {clean[o].tolist()}")
        print(f"  grad_spread {grad_spread:.3e}, loss_spread {loss_spread:.3e}, first-step loss error {first_loss_err:.2e}")
        out["grad_spread"], out["loss_spread"], out["clean"] = np.float64(grad_spread), np.float64(loss_spread), clean
        out["first_loss_err"] = np.float64(first_loss_err)
        if all(int((clean[o] >= 32).sum()) >= 2 for o in range(3)):
            break
        print("  an fp32 order misses the tight tier on these batches: other seeds")
    else:
        raise AssertionError("no batch seeds on which all three fp32 orders meet the tight tier")
    assert 0.005 < frac < 0.2 and losses64[-1] < 0.8 * losses64[0], (frac, losses64)
    save("g19_segtrain", **out)
    save("g19_segtrain_grads", **small)


def reference_simple_cnn():
    """The reference's real ``SimpleCNN`` class.  train_mnist_cls.py does not import here (matplotlib, medpy, pandas, ...), and
    everything around the class is a script; so only the class definition is compiled, from the reference's own file at
    generation time, into a namespace that holds what it names (``nn``)."""
    import ast
    path = os.path.join(REF, "train_mnist_cls.py")
    tree = ast.parse(open(path).read(), filename=path)
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "SimpleCNN"]
    assert len(nodes) == 1
    ns = {"nn": torch.nn, "torch": torch, "F": torch.nn.functional}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns["SimpleCNN"]


MNISTCLS_SEED, MNISTCLS_TRAIN, MNISTCLS_TEST, MNISTCLS_B, MNISTCLS_EPOCHS = 20, 1024, 512, 64, 3
MNISTCLS_FULL = 32768        # tensors up to this many elements are stored whole; fc1.weight as norm, probe dots and a sample
MNISTCLS_SAMPLE_STRIDE, MNISTCLS_SAMPLE_N = 97, 4096
MNISTCLS_MOVED_RUNS = 6


def g20(ddpm):
    """The reference's digit classifier and its training (train_mnist_cls.py:31-47, 79-96): the real SimpleCNN,
    nn.CrossEntropyLoss() and torch.optim.Adam(lr=1e-3) in fp64 (the yardstick) on the first 1,024 digits of t10k in file
    order at B = 64 for three epochs, evaluated on the next 512; and in fp32 in four arithmetic orders (the reference's own
    spread; which the tolerances of the GPU tests are multiples of).  Three files, each below the size limit:
    g20_mnist_digits.npz (the digits), g20_mnistcls.npz, g20_mnistcls_grads.npz (the three-batch gradients)."""
    print("G20 MNIST digit classifier and its training step")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mnistcls_ref
    SimpleCNN = reference_simple_cnn()
    with gzip.open(os.path.join(REF, "MNIST/raw/t10k-images-idx3-ubyte.gz"), "rb") as f:
        all_imgs = np.frombuffer(f.read(), dtype=np.uint8, offset=16).reshape(-1, 28, 28)
    with gzip.open(os.path.join(REF, "MNIST/raw/t10k-labels-idx1-ubyte.gz"), "rb") as f:
        all_lab = np.frombuffer(f.read(), dtype=np.uint8, offset=8)
    sd_np = weights.procedural_mnistcls_state_dict(MNISTCLS_SEED)
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    names = list(sd.keys())
    assert names == [k for k, _ in SimpleCNN().named_parameters()] == list(SimpleCNN().state_dict().keys())
    for k, v in SimpleCNN().state_dict().items():
        assert tuple(v.shape) == tuple(sd[k].shape), k
    n_all = MNISTCLS_TRAIN + MNISTCLS_TEST

    def fresh(dtype, channels_last=False, state=None):
        m = SimpleCNN()
        m.load_state_dict(sd if state is None else state)
        m = m.to(dtype)
        if channels_last:
            m = m.to(memory_format=torch.channels_last)
        return m.train()

    def one_ulp_off(trial):
        """The initial weights with every element moved by -1, 0 or +1 fp32 ulp (procedural, keyed by name and trial)."""
        moved = {}
        for k, v in sd_np.items():
            step = np.floor(rng.uniform(v.shape, 2021 + trial, rng.fnv1a64("g20." + k), 0.0, 3.0)).astype(np.int32) - 1
            moved[k] = torch.from_numpy((v.view(np.int32) + step).view(np.float32).copy())
        return moved

    def prep(x, dtype, channels_last):
        x = x.to(dtype)
        return x.contiguous(memory_format=torch.channels_last) if channels_last else x

    criterion = torch.nn.CrossEntropyLoss()

    def grads_at_init(dtype, x, y, channels_last=False):
        m = fresh(dtype, channels_last)
        loss = criterion(m(prep(x, dtype, channels_last)), y)
        loss.backward()
        return float(loss.detach()), [p.grad.detach().clone().contiguous() for p in m.parameters()]

    def trajectory(dtype, batches, x_test, channels_last=False, keep=(), state=None):
        m = fresh(dtype, channels_last, state)
        opt = torch.optim.Adam(m.parameters(), lr=0.001)
        losses, kept = [], {}
        for i, (x, y) in enumerate(batches):
            opt.zero_grad()
            loss = criterion(m(prep(x, dtype, channels_last)), y)
            loss.backward()
            opt.step()
            losses.append(float(loss))
            if i + 1 in keep:
                kept[i + 1] = {k: v.detach().clone() for k, v in m.state_dict().items()}
        m.eval()
        with torch.no_grad():
            logits = m(prep(x_test, dtype, channels_last)).detach().clone()
        return losses, kept, logits

    # channels_last is not an order this net has: the reference's own x.view(-1, 64 * 7 * 7) raises on a channels_last
    # activation.  The orders are the default, oneDNN off, one thread, and oneDNN off on one thread
    orders = ("default", "onednn_off", "one_thread", "onednn_off_one_thread")

    def run_order(order, fn):
        if order == "onednn_off":
            with torch.backends.mkldnn.flags(enabled=False):
                return fn(False)
        if order in ("one_thread", "onednn_off_one_thread"):
            n = torch.get_num_threads()
            torch.set_num_threads(1)
            try:
                return run_order(order[:-len("_one_thread")] or "default", fn) if order != "one_thread" else fn(False)
            finally:
                torch.set_num_threads(n)
        return fn(False)

    def exact_or(a, b, what):
        a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
        if torch.equal(a, b):
            return
        rel = float((a - b).abs().max()) / max(1e-300, float(b.abs().max()))
        assert rel <= 1e-12, (what, rel)

    def summarise(prefix, t, store):
        """A tensor as the fixture holds it: whole up to MNISTCLS_FULL elements, else norm, probe dots and a sample."""
        t = t.detach().double().contiguous()
        if t.numel() <= MNISTCLS_FULL:
            store[prefix] = t.numpy().copy()
            return
        flat = t.reshape(-1)
        store[prefix + ".norm"] = np.float64(float(flat.norm()))
        store[prefix + ".dots"] = np.asarray([float(torch.dot(flat, torch.from_numpy(
            rng.uniform((flat.numel(),), 2020 + j, 20, -1.0, 1.0)).double())) for j in range(4)])
        store[prefix + ".sample"] = flat[::MNISTCLS_SAMPLE_STRIDE][:MNISTCLS_SAMPLE_N].numpy().copy()

    for attempt in range(6):
        lo = attempt * n_all
        imgs, lab = all_imgs[lo:lo + n_all].copy(), all_lab[lo:lo + n_all].copy()
        x_all, y_all = mnistcls_ref.images_of(imgs, torch.float32), torch.from_numpy(lab.astype(np.int64))
        x_tr, y_tr, x_te, y_te = x_all[:MNISTCLS_TRAIN], y_all[:MNISTCLS_TRAIN], x_all[MNISTCLS_TRAIN:], y_all[MNISTCLS_TRAIN:]
        batches = mnistcls_ref.epoch_batches(x_tr, y_tr, MNISTCLS_EPOCHS, MNISTCLS_B)
        n_steps = len(batches)
        assert n_steps == 48
        out = {"seed": np.int64(MNISTCLS_SEED), "first_digit": np.int64(lo), "n_train": np.int64(MNISTCLS_TRAIN)}
        grads_out = {}
        # ---- fp64: the real reference, and the restatement against it
        m64 = fresh(torch.float64).eval()
        with torch.no_grad():
            logits_init = m64(x_tr[:MNISTCLS_B].double())
        exact_or(mnistcls_ref.forward(mnistcls_ref.params_of(sd, torch.float64), x_tr[:MNISTCLS_B].double()).detach(), logits_init,
                 "initial logits")
        out["logits_init"] = logits_init.numpy().copy()
        ref_grads, losses0 = [], []
        for b in range(3):
            x, y = batches[b]
            loss, grads = grads_at_init(torch.float64, x, y)
            r_loss, r_grads = mnistcls_ref.loss_and_grads(mnistcls_ref.params_of(sd, torch.float64), x, y)
            exact_or(r_loss, loss, f"loss {b}")
            for k, g_, r_ in zip(names, grads, r_grads.values()):
                exact_or(r_, g_, f"grad {b} {k}")
                summarise(f"grad{b}.{k}", g_, grads_out)
            ref_grads.append(grads)
            losses0.append(loss)
        out["loss_init"] = np.asarray(losses0)
        losses64, kept64, logits64 = trajectory(torch.float64, batches, x_te, keep=(1, n_steps))
        r_losses, r_kept, r_params = mnistcls_ref.train_steps(sd, batches, torch.float64, keep=(1, n_steps))
        exact_or(torch.tensor(r_losses), torch.tensor(losses64), "losses")
        for step in (1, n_steps):
            for k in names:
                exact_or(r_kept[step][k], kept64[step][k], f"step {step} {k}")
                summarise(f"step{step}.{k}", kept64[step][k], out)
        exact_or(mnistcls_ref.forward(r_params, x_te.double()).detach(), logits64, "test logits")
        out["loss_steps"], out["test_logits"] = np.asarray(losses64), logits64.numpy().copy()
        acc64 = float((logits64.argmax(1) == y_te).float().mean())
        print(f"  digits {lo}..{lo + n_all - 1}: fp64 loss {losses64[0]:.4f} -> {losses64[-1]:.4f}, accuracy {100 * acc64:.1f} %")
        assert acc64 > 0.80 and losses64[-1] < 0.5 * losses64[0], (acc64, losses64[0], losses64[-1])
        # ---- fp32 in four arithmetic orders: the reference's own spread
        grad_spread, loss_spread, logit_spread, runs = 0.0, 0.0, 0.0, {}
        for order in orders:
            for b in range(3):
                x, y = batches[b]
                _, grads = run_order(order, lambda cl: grads_at_init(torch.float32, x, y, channels_last=cl))
                grad_spread = max(grad_spread, max(mnistcls_ref.rel_l2(g_, r_) for g_, r_ in zip(grads, ref_grads[b])))
            l32, _, z32 = run_order(order, lambda cl: trajectory(torch.float32, batches, x_te, channels_last=cl))
            loss_spread = max(loss_spread, max(abs(a - c) for a, c in zip(l32, losses64)))
            logit_spread = max(logit_spread, float((z32.double() - logits64).abs().max()))
            runs[order] = z32
        top2 = logits64.topk(2, dim=1).values
        decided = (top2[:, 0] - top2[:, 1]) > 100.0 * logit_spread
        left_out = int((~decided).sum())
        print(f"  grad_spread {grad_spread:.3e}, loss_spread {loss_spread:.3e}, logit_spread {logit_spread:.3e}; "
              f"{left_out} of {MNISTCLS_TEST} test digits have a top-two gap below 100 x logit_spread")
        agree = all(bool((runs[o].argmax(1)[decided] == logits64.argmax(1)[decided]).all()) for o in orders)
        if not (agree and left_out <= 0.02 * MNISTCLS_TEST):
            print("  an fp32 order misses the argmax condition on these digits: the next 1,536")
            continue
        # ---- is the 48-step comparison meaningful on these digits?  The four orders above are nearly the same arithmetic
        # (the same GEMM and convolution routines), so they can all fall on one side of a ReLU / pooling decision that any
        # other correct fp32 arithmetic may take the other way.  The reference's own fp32 run from weights one ulp away
        # is such an arithmetic: a block on which it leaves 4 x loss_spread, or changes a decided argmax, cannot tell a
        # correct fp32 implementation from a wrong one and is not used.
        moved_err, moved_agree = [], True
        for trial in range(MNISTCLS_MOVED_RUNS):
            lm, _, zm = trajectory(torch.float32, batches, x_te, state=one_ulp_off(trial))
            moved_err.append(max(abs(a - c) for a, c in zip(lm, losses64)))
            moved_agree = moved_agree and bool((zm.argmax(1)[decided] == logits64.argmax(1)[decided]).all())
        print(f"  fp32 from weights one ulp away: worst loss distance to fp64 {['%.2e' % e for e in moved_err]} "
              f"(4 x loss_spread {4 * loss_spread:.2e}), decided argmax kept: {moved_agree}")
        out["moved_loss_err"] = np.asarray(moved_err)
        if moved_agree and max(moved_err) <= 4.0 * loss_spread:
            break
        print("  the trajectory on these digits is not stable under one ulp: the next 1,536")
    else:
        raise AssertionError("no block of digits on which the fp32 reference is stable and meets the argmax condition")
    out["grad_spread"], out["loss_spread"], out["logit_spread"] = np.float64(grad_spread), np.float64(loss_spread), \
        np.float64(logit_spread)
    out["accuracy"], out["left_out"] = np.float64(acc64), np.int64(left_out)
    save("g20_mnist_digits", images=imgs, labels=lab)
    save("g20_mnistcls", **out)
    save("g20_mnistcls_grads", **grads_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--skip-long", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(os.cpu_count())
    ddpm = import_reference()
    os.makedirs(GOLD, exist_ok=True)
    todo = [("G0", g0_inventory), ("G1", g1), ("G2", g2), ("G3", g3), ("G4", g4), ("G6", g6),
            ("G7", g7), ("G8", g8), ("G9", g9), ("G10", g10), ("G12", g12), ("G14", g14), ("G15", g15), ("G17", g17), ("G18", g18), ("G19", g19), ("G20", g20), ("G5", g5), ("G11", g11), ("G13", g13), ("G16", g16)]
    only = set(filter(None, a.only.split(",")))
    for name, fn in todo:
        if only and name not in only:
            continue
        if a.skip_long and name in ("G5", "G11", "G13", "G16"):
            continue
        t0 = time.time()
        fn(ddpm)
        print(f"  [{name} done in {time.time()-t0:.1f}s]")


if __name__ == "__main__":
    main()
