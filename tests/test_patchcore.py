"""PatchCore, host side (no GPU): the wide_resnet50_2 trunk's names and shapes, load_patchcore, the blur kernel, feature
sizes, the restatement of the reference against itself where it pins a convention, and the evalio PatchCore helpers
(test.py:200-375) against transcriptions of the reference's branches."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import checkpoint, evalio, weights
from localdiffusion_hallucination_amd.patchcore import EMBED_DIM, PatchCore, conv_out, feature_sizes, gaussian_kernel1d

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patchcore_ref as ref  # noqa: E402


def _wrn50_2_inventory():
    """The torchvision wide_resnet50_2 state_dict entries up to layer3, written out from the architecture."""
    inv = {"conv1.weight": (64, 3, 7, 7)}
    for k in ("weight", "bias", "running_mean", "running_var"):
        inv["bn1." + k] = (64,)
    inv["bn1.num_batches_tracked"] = ()
    cin = 64
    for li, (n, planes) in enumerate(((3, 64), (4, 128), (6, 256))):
        width, cout = planes * 2, planes * 4
        for i in range(n):
            p = f"layer{li + 1}.{i}."
            inv[p + "conv1.weight"] = (width, cin if i == 0 else cout, 1, 1)
            inv[p + "conv2.weight"] = (width, width, 3, 3)
            inv[p + "conv3.weight"] = (cout, width, 1, 1)
            for b, c in (("bn1.", width), ("bn2.", width), ("bn3.", cout)):
                for k in ("weight", "bias", "running_mean", "running_var"):
                    inv[p + b + k] = (c,)
                inv[p + b + "num_batches_tracked"] = ()
            if i == 0:
                inv[p + "downsample.0.weight"] = (cout, cin, 1, 1)
                for k in ("weight", "bias", "running_mean", "running_var"):
                    inv[p + "downsample.1." + k] = (cout,)
                inv[p + "downsample.1.num_batches_tracked"] = ()
        cin = cout
    return inv


def test_state_dict_names_and_shapes():
    m = PatchCore((84, 84))
    sd = m.state_dict()
    inv = _wrn50_2_inventory()
    fe = {k[len("feature_extractor."):]: tuple(v.shape) for k, v in sd.items() if k.startswith("feature_extractor.")}
    assert fe == inv
    assert set(sd) == {"feature_extractor." + k for k in inv} | {"memory_bank"}
    assert dict(weights.patchcore_param_shapes()) == inv
    assert list(weights.patchcore_param_shapes()) == list(fe)             # the module's order


def test_constructor_rejects_what_has_no_kernels():
    with pytest.raises(ValueError):
        PatchCore((84, 84), backbone="efficientnet_b4")
    with pytest.raises(ValueError):
        PatchCore((84, 84), layers=("layer1", "layer2"))
    with pytest.raises(ValueError):
        PatchCore((84, 84), tiler=object())
    assert ldh.PatchCore is PatchCore


def _procedural_sd():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_patchcore_state_dict(0).items()}


@pytest.mark.parametrize("prefix", ["", "feature_extractor.", "feature_extractor.feature_extractor."])
def test_load_patchcore_prefixes(prefix, tmp_path):
    sd = _procedural_sd()
    full = {prefix + k: v for k, v in sd.items()}
    full[prefix + "layer4.0.conv1.weight"] = torch.zeros(512, 1024, 1, 1)     # unused parts of the backbone
    full[prefix + "fc.weight"] = torch.zeros(1000, 2048)
    full[prefix + "fc.bias"] = torch.zeros(1000)
    bank = np.random.default_rng(0).standard_normal((37, EMBED_DIM)).astype(np.float32)
    np.save(tmp_path / "bank.npy", bank)
    torch.save(full, tmp_path / "wrn.pt")
    m = PatchCore((84, 84))
    info = checkpoint.load_patchcore(str(tmp_path / "wrn.pt"), str(tmp_path / "bank.npy"), m)
    assert info == {"n_tensors": len(sd), "bank_rows": 37}
    own = m.feature_extractor.state_dict()
    assert all(torch.equal(own[k], sd[k]) for k in sd)
    assert torch.equal(m.memory_bank, torch.from_numpy(bank))


def test_load_patchcore_rejects_a_different_backbone():
    sd = _procedural_sd()
    sd.pop("layer3.5.conv3.weight")
    with pytest.raises(RuntimeError):
        checkpoint.load_patchcore(sd, np.zeros((3, EMBED_DIM), np.float32), PatchCore((84, 84)))


def test_memory_bank_round_trips_through_state_dict():
    m = PatchCore((84, 84))
    m.set_memory_bank(np.ones((5, EMBED_DIM), np.float32))
    m2 = PatchCore((84, 84))
    m2.load_state_dict(m.state_dict())
    assert m2.memory_bank.shape == (5, EMBED_DIM)
    with pytest.raises(ValueError):
        m.set_memory_bank(np.ones((5, 100), np.float32))


def test_gaussian_kernel():
    g = gaussian_kernel1d()
    assert g.numel() == 33 == 2 * int(4 * 4.0 + 0.5) + 1
    assert abs(float(g.sum()) - 1.0) < 1e-6 and int(g.argmax()) == 16
    assert torch.allclose(g, g.flip(0))
    k2 = ref.gaussian_kernel2d()
    assert k2.shape == (33, 33) and abs(float(k2.sum()) - 1.0) < 1e-6
    assert torch.allclose(k2, g[:, None] * g[None, :], atol=1e-9)


@pytest.mark.parametrize("H,W", [(84, 84), (224, 224), (45, 37), (100, 61), (17, 17)])
def test_feature_sizes_match_torch(H, W):
    sd = _procedural_sd()
    x = torch.zeros(1, 3, H, W)
    with torch.no_grad():
        f = ref.features(sd, x)
    (h2, w2), (h3, w3) = feature_sizes(H, W)
    assert f["layer2"].shape[2:] == (h2, w2) and f["layer3"].shape[2:] == (h3, w3)
    assert f["layer2"].shape[1] == 512 and f["layer3"].shape[1] == 1024


def test_feature_sizes_of_the_reference_inputs():
    assert feature_sizes(84, 84) == ((11, 11), (6, 6))
    assert feature_sizes(224, 224) == ((28, 28), (14, 14))
    assert conv_out(21, 3, 2, 1) == 11 and conv_out(21, 1, 2, 0) == 11 and conv_out(11, 3, 2, 1) == 6


def test_procedural_weights_keep_activations_order_one():
    sd = _procedural_sd()
    x = torch.from_numpy(np.random.default_rng(1).uniform(-2, 2, (1, 3, 84, 84)).astype(np.float32))
    with torch.no_grad():
        f = ref.features(sd, x)
    for name in ("layer2", "layer3"):
        s = float(f[name].std())
        assert 0.1 < s < 3.0, (name, s)
    assert all(np.isfinite(np.asarray(v)).all() for v in weights.procedural_patchcore_state_dict(0).values())


# ------------------------------------------------------------------------------------------------ evalio
def _transcribed_mask(anomaly_map, rule, img_size=None):
    """test.py:245-375, the branch of ``rule``, as the reference writes it."""
    if img_size is not None and rule in ("8to3", "8to5", "transistor", "toothbrush", "grid"):
        anomaly_map = F.interpolate(anomaly_map, size=(img_size, img_size), mode='bilinear', align_corners=False)
    if rule == '8to3':
        if anomaly_map.max() > 37.0:
            if anomaly_map.max() > 44:
                threshold = 41.7
            elif anomaly_map.max() > 40.0:
                threshold = 38.2
            else:
                threshold = 35.0
            binary_mask = (anomaly_map.cpu() > threshold).float()
            map_pred = torch.clip(anomaly_map.cpu(), min=threshold-anomaly_map.std(), max=threshold)
            mask_pred = (map_pred - map_pred.min()) / (threshold - map_pred.min())
            mask_pred = mask_pred **2
        else:
            mask_pred = torch.ones_like(anomaly_map.cpu())
            binary_mask = torch.ones_like(anomaly_map.cpu())
    elif rule == '8to5':
        if anomaly_map.max() > 58.5:
            if anomaly_map.max() > 71.0:
                threshold = 61.0
            elif anomaly_map.max() > 65:
                threshold = 57.0
            else:
                threshold = 55.0
            binary_mask = (anomaly_map.cpu() > threshold).float()
            map_pred = torch.clip(anomaly_map.cpu(), min=threshold-anomaly_map.std(), max=threshold)
            mask_pred = (map_pred - map_pred.min()) / (threshold - map_pred.min())
            mask_pred = mask_pred **2
        else:
            mask_pred = torch.ones_like(anomaly_map.cpu())
            binary_mask = torch.ones_like(anomaly_map.cpu())
    elif rule == 't12flair':
        if anomaly_map.max() > 43:
            if anomaly_map.max() > 60:
                threshold = anomaly_map.max()-12
            elif anomaly_map.max() > 51:
                threshold = 47
            elif anomaly_map.max() > 48.5:
                threshold = 44
            else:
                threshold = 42
            binary_mask = (anomaly_map.cpu() > threshold).float()
            map_pred = torch.clip(anomaly_map.cpu(), min=threshold-anomaly_map.std(), max=threshold)
            mask_pred = (map_pred - map_pred.min()) / (threshold - map_pred.min())
            mask_pred = mask_pred **2
        else:
            mask_pred = torch.ones_like(anomaly_map.cpu())
            binary_mask = torch.ones_like(anomaly_map.cpu())
    elif rule == 'flair2t1':
        if anomaly_map.max() > 43:
            if anomaly_map.max() > 60:
                threshold = 47
            elif anomaly_map.max() > 50:
                threshold = 43
            else:
                threshold = 42
            binary_mask = (anomaly_map.cpu() > threshold).float()
            map_pred = torch.clip(anomaly_map.cpu(), min=threshold-anomaly_map.std(), max=threshold)
            mask_pred = (map_pred - map_pred.min()) / (threshold - map_pred.min())
            mask_pred = mask_pred **2
        else:
            mask_pred = torch.ones_like(anomaly_map.cpu())
            binary_mask = torch.ones_like(anomaly_map.cpu())
    elif rule == 'transistor':
        if anomaly_map.max() > 32:
            if anomaly_map.max() > 40.0:
                threshold = 33.5
            elif anomaly_map.max() > 36.8:
                threshold = anomaly_map.max() - 2*anomaly_map.cpu().std()
            elif anomaly_map.max() > 35.0:
                threshold = anomaly_map.max() - 1*anomaly_map.cpu().std()
            else:
                threshold = 29.5
            binary_mask = (anomaly_map.cpu() > threshold).float()
            map_pred = torch.clip(anomaly_map.cpu(), min=threshold-0.5*anomaly_map.cpu().std(), max=threshold)
            mask_pred = (map_pred - map_pred.min()) / (threshold - map_pred.min())
            mask_pred = mask_pred**2
        else:
            mask_pred = torch.ones_like(anomaly_map.cpu())
            binary_mask = torch.ones_like(anomaly_map.cpu())
    elif rule == 'toothbrush':
        if anomaly_map.max() > 35:
            if anomaly_map.max() > 49:
                threshold = 40.0
            else:
                threshold = 28.0
            binary_mask = (anomaly_map.cpu() > threshold).float()
            map_pred = torch.clip(anomaly_map.cpu(), min=anomaly_map.cpu().min(), max=threshold)
            mask_pred = (map_pred - map_pred.min()) / (threshold - map_pred.min())
            mask_pred = mask_pred**2
        else:
            mask_pred = torch.ones_like(anomaly_map.cpu())
            binary_mask = torch.ones_like(anomaly_map.cpu())
    elif rule == 'grid':
        if anomaly_map.max() > 27:
            if anomaly_map.max() > 40:
                threshold = 35.0
            elif anomaly_map.max() > 35.0:
                threshold = 30.0
            else:
                threshold = 26.5
            binary_mask = (anomaly_map.cpu() > threshold).float()
            map_pred = torch.clip(anomaly_map.cpu(), min=anomaly_map.cpu().min(), max=threshold)
            mask_pred = (map_pred - map_pred.min()) / (threshold - map_pred.min())
            mask_pred = mask_pred**2
        else:
            mask_pred = torch.ones_like(anomaly_map.cpu())
            binary_mask = torch.ones_like(anomaly_map.cpu())
    return mask_pred, binary_mask


# every cut of every rule, from both sides: the map's max is placed just below / above it
_CUTS = {"8to3": (37.0, 40.0, 44.0), "8to5": (58.5, 65.0, 71.0), "t12flair": (43.0, 48.5, 51.0, 60.0),
         "flair2t1": (43.0, 50.0, 60.0), "transistor": (32.0, 35.0, 36.8, 40.0), "toothbrush": (35.0, 49.0),
         "grid": (27.0, 35.0, 40.0)}


def _crafted_map(mx, key, size=28):
    g = torch.Generator().manual_seed(key)
    a = torch.rand(1, 1, size, size, generator=g) * 0.8 * mx
    a[0, 0, size // 3, size // 2] = mx
    return a


@pytest.mark.parametrize("rule", sorted(_CUTS))
def test_patchcore_ood_mask_matches_the_reference_branches(rule):
    n = 0
    for cut in _CUTS[rule]:
        for mx in (cut - 0.3, cut + 0.3):
            a = _crafted_map(mx, n)
            n += 1
            got = evalio.patchcore_ood_mask(a, rule)
            want = _transcribed_mask(a.clone(), rule)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (rule, mx)
            fell_back = bool((want[0] == 1).all())
            assert fell_back == (mx < _CUTS[rule][0]), (rule, mx)


@pytest.mark.parametrize("rule", ["8to3", "grid", "t12flair"])
def test_patchcore_ood_mask_resizes_mnist_and_mvtec_maps(rule):
    a = _crafted_map(45.0, 99, size=84)
    got = evalio.patchcore_ood_mask(a, rule, img_size=28)
    want = _transcribed_mask(a.clone(), rule, img_size=28)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[0].shape == ((1, 1, 84, 84) if rule == "t12flair" else (1, 1, 28, 28))
    with pytest.raises(ValueError):
        evalio.patchcore_ood_mask(a, "nope")


def _normalize(x):
    mean = torch.tensor([0.485, 0.456, 0.406]).view(-1, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(-1, 1, 1)
    return (x - mean) / std


@pytest.mark.parametrize("data,shape,hi", [("mnist", (2, 1, 28, 28), 2.0), ("mnist", (1, 1, 28, 28), 1.0),
                                           ("mvtec_grid", (1, 3, 64, 64), 2.0)])
def test_patchcore_preprocess_mnist_mvtec(data, shape, hi):
    lr = torch.from_numpy(np.random.default_rng(3).uniform(0, hi, shape).astype(np.float32))
    got = evalio.patchcore_preprocess(lr, data)
    lr_ad = lr.repeat(1, 3, 1, 1) if lr.shape[1] != 3 else lr.clone()              # test.py:200-238, 243
    if lr_ad.max() > 1.0:
        lr_ad = lr_ad / 2
    size = 224 if "mvtec" in data else 84
    lr_ad = F.interpolate(lr_ad, size=(size, size), mode='bilinear', align_corners=False)
    assert torch.equal(got, _normalize(lr_ad)) and got.shape == (shape[0], 3, size, size)


@pytest.mark.parametrize("translate_zero", [True, False])
def test_patchcore_preprocess_mri(translate_zero):
    mean_t1, std_t1 = 812.5, 640.0
    lr = torch.from_numpy(np.random.default_rng(4).uniform(0, 4, (1, 1, 32, 32)).astype(np.float32))
    got = evalio.patchcore_preprocess(lr, "mri", mean_t1, std_t1, translate_zero=translate_zero)
    lr_ad = lr.repeat(1, 3, 1, 1)
    if translate_zero:
        mini = (0 - mean_t1) / std_t1
        lr_ad = lr_ad - torch.abs(torch.tensor(mini))
    lr_ad = lr_ad[:, 0] * std_t1 + mean_t1
    lr_ad = lr_ad / 4096.0
    lr_ad = lr_ad.repeat(1, 3, 1, 1)
    assert torch.equal(got, _normalize(lr_ad)) and got.shape == (1, 3, 32, 32)
    with pytest.raises(ValueError):
        evalio.patchcore_preprocess(lr, "mri")
