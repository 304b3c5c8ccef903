"""Checkpoint ingestion for the reference's training artefacts.

``Trainer.save`` (/root/reference/ddpm.py:1495-1507) writes ``results/<project>/model-<milestone>.pt``
as a dict  {'step', 'model', 'opt', 'ema', 'scaler'}:
  * ``data['model']``  = ``GaussianDiffusion.state_dict()``: 13 schedule buffers + ``model.<unet key>``;
  * ``data['ema']``    = ``ema_pytorch.EMA.state_dict()``: the same keys twice, under ``online_model.`` and
    ``ema_model.``, plus ``initted`` / ``step`` scalars.  Sampling uses the EMA copy
    (``trainer.ema.ema_model``, /root/reference/test.py:144-147,393).
``Trainer.load`` (:1509-1527) restores them by name -- which is why this package keeps the reference's
parameter names.  No checkpoint ships with the reference; the format is pinned by a file written by the reference's
own ``Trainer.save`` in the build container (tools/make_goldens.py g12 -> tests/golden/g12_trainer_save_manifest.json:
every key with shape and dtype), which this module reads and whose layout ``save_reference_checkpoint`` reproduces
(also checked there: the reference's ``Trainer.load`` restores a file written here).
"""
import torch

_EMA_PREFIX = "ema_model."
_ONLINE_PREFIX = "online_model."


def _read(path_or_dict, trust_pickle=False):
    """Files are read with torch's restricted unpickler (``weights_only=True``): what ``Trainer.save`` writes --
    tensors, ints, strings, plain containers -- needs nothing else (checked against a file written by the
    reference's own ``Trainer.save``, tools/make_goldens.py g12).  A file that the restricted loader rejects is NOT
    retried with the full unpickler (arbitrary code execution) unless the caller says ``trust_pickle=True``;
    I/O errors and corrupt files propagate as they are."""
    if isinstance(path_or_dict, dict):
        return path_or_dict
    if trust_pickle:
        return torch.load(path_or_dict, map_location="cpu", weights_only=False)
    import pickle
    try:
        return torch.load(path_or_dict, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        raise RuntimeError(f"{path_or_dict}: rejected by the restricted unpickler ({e}); pass trust_pickle=True "
                           "only for a file whose origin you trust") from e


def extract_state_dict(data, use_ema=True):
    """-> (state_dict for GaussianDiffusion, source tag).  Accepts the Trainer.save dict, a bare
    GaussianDiffusion state_dict, or a bare Unet state_dict."""
    if "ema" in data and use_ema and isinstance(data["ema"], dict):
        sd = {k[len(_EMA_PREFIX):]: v for k, v in data["ema"].items() if k.startswith(_EMA_PREFIX)}
        if sd:
            return sd, "ema"
        sd = {k[len(_ONLINE_PREFIX):]: v for k, v in data["ema"].items() if k.startswith(_ONLINE_PREFIX)}
        if sd:
            return sd, "ema.online"
    if "model" in data and isinstance(data["model"], dict):
        return dict(data["model"]), "model"
    return dict(data), "bare"


def load_reference_checkpoint(path_or_dict, diffusion, use_ema=True, strict=True, trust_pickle=False):
    """Load a reference checkpoint into ``diffusion`` (a ``GaussianDiffusion`` of this package, or a
    ``Unet``).  Returns {'step', 'source', 'missing', 'unexpected'}."""
    data = _read(path_or_dict, trust_pickle)
    sd, source = extract_state_dict(data, use_ema)
    own = diffusion.state_dict()
    if not any(k in own for k in sd) and any(("model." + k) in own for k in sd):
        sd = {"model." + k: v for k, v in sd.items()}                  # bare Unet dict into a GaussianDiffusion
    if not any(k in own for k in sd) and any(k.startswith("model.") and k[6:] in own for k in sd):
        sd = {k[6:]: v for k, v in sd.items() if k.startswith("model.")}   # diffusion dict into a bare Unet
    missing = [k for k in own if k not in sd]
    unexpected = [k for k in sd if k not in own]
    bad = [k for k in sd if k in own and tuple(sd[k].shape) != tuple(own[k].shape)]
    if bad:
        raise RuntimeError(f"checkpoint tensors with the wrong shape: {bad[:5]}")
    if strict and (missing or unexpected):
        raise RuntimeError(f"checkpoint does not match the model: missing {missing[:5]} unexpected {unexpected[:5]}")
    keep = {k: v.to(own[k].dtype) for k, v in sd.items() if k in own}
    diffusion.load_state_dict(keep, strict=False)
    if hasattr(diffusion, "model") and hasattr(diffusion.model, "invalidate"):
        diffusion.model.invalidate()                                   # repack kernel-layout weights on next use
    step = data.get("step", None) if isinstance(data, dict) else None
    return {"step": int(step) if step is not None else None, "source": source, "missing": missing,
            "unexpected": unexpected}


def adam_param_groups(n_params, lr=1e-4, betas=(0.9, 0.99), eps=1e-8):
    """The ``param_groups`` of ``torch.optim.Adam(params, lr=lr, betas=betas, eps=eps).state_dict()`` over ``n_params``
    parameters (the defaults are the reference trainer's, ddpm.py:1261,1265,1444)."""
    return [{"lr": float(lr), "betas": (float(betas[0]), float(betas[1])), "eps": float(eps), "weight_decay": 0, "amsgrad": False,
             "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "params": list(range(n_params))}]


def save_reference_checkpoint(diffusion, path, step=0):
    """Write ``diffusion`` in the reference's Trainer.save layout (model == ema copy; no optimizer state)."""
    sd = {k: v.detach().cpu() for k, v in diffusion.state_dict().items()}
    ema = {_ONLINE_PREFIX + k: v for k, v in sd.items()}
    ema.update({_EMA_PREFIX + k: v for k, v in sd.items()})
    ema["initted"] = torch.tensor(True)              # ema_pytorch registers both as 0-d buffers
    ema["step"] = torch.tensor(int(step))
    # 'opt': a fresh Adam state in torch's state_dict layout (no moments yet) over the model's parameters, with the
    # reference trainer's defaults (ddpm.py:1261,1265,1444): Trainer.load hands it to opt.load_state_dict (:1521)
    n_params = sum(1 for _ in diffusion.parameters())
    opt = {"state": {}, "param_groups": adam_param_groups(n_params)}
    torch.save({"step": int(step), "model": sd, "opt": opt, "ema": ema, "scaler": None}, path)


def load_seg_checkpoint(path_or_dict, seg, trust_pickle=False):
    """Load the segmentation U-Net's weights into ``seg`` (a ``SegUNet``): a bare ``state_dict`` as ``train_seg.py`` saves
    it and ``test.py:219`` reads it (``seg_model.load_state_dict(torch.load(path))``), BatchNorm running statistics and
    ``num_batches_tracked`` included.  Same restricted unpickler as ``load_reference_checkpoint``; names and shapes must
    match exactly (RuntimeError otherwise).  Returns {'n_tensors'}."""
    data = _read(path_or_dict, trust_pickle)
    if not isinstance(data, dict):
        raise RuntimeError(f"segmentation checkpoint: expected a state_dict, got {type(data).__name__}")
    sd = {k[7:] if k.startswith("module.") else k: v for k, v in data.items()}     # (an nn.DataParallel wrapper's prefix)
    own = seg.state_dict()
    bad = [k for k in sd if k in own and tuple(sd[k].shape) != tuple(own[k].shape)]
    if bad:
        raise RuntimeError(f"checkpoint tensors with the wrong shape: {bad[:5]}")
    missing = [k for k in own if k not in sd]
    unexpected = [k for k in sd if k not in own]
    if missing or unexpected:
        raise RuntimeError(f"checkpoint does not match the model: missing {missing[:5]} unexpected {unexpected[:5]}")
    seg.load_state_dict({k: v.to(own[k].dtype) for k, v in sd.items()})
    return {"n_tensors": len(sd)}


def load_mnist_classifier(path_or_dict, model, trust_pickle=False):
    """Load the digit classifier's weights into ``model`` (a ``MnistClassifier``): a bare ``state_dict`` as
    ``train_mnist_cls.py:116`` saves it (``torch.save(model.state_dict(), path)``) and as ``MnistClassifierTrainer.fit``
    writes it.  Same restricted unpickler as ``load_reference_checkpoint``; names and shapes must match exactly
    (RuntimeError otherwise).  Returns {'n_tensors'}."""
    data = _read(path_or_dict, trust_pickle)
    if not isinstance(data, dict):
        raise RuntimeError(f"digit classifier checkpoint: expected a state_dict, got {type(data).__name__}")
    sd = {k[7:] if k.startswith("module.") else k: v for k, v in data.items()}     # (an nn.DataParallel wrapper's prefix)
    own = model.state_dict()
    bad = [k for k in sd if k in own and tuple(sd[k].shape) != tuple(own[k].shape)]
    if bad:
        raise RuntimeError(f"checkpoint tensors with the wrong shape: {bad[:5]}")
    missing = [k for k in own if k not in sd]
    unexpected = [k for k in sd if k not in own]
    if missing or unexpected:
        raise RuntimeError(f"checkpoint does not match the model: missing {missing[:5]} unexpected {unexpected[:5]}")
    model.load_state_dict({k: torch.as_tensor(v).to(own[k].dtype) for k, v in sd.items()})
    return {"n_tensors": len(sd)}


_PC_PREFIXES = ("feature_extractor.feature_extractor.", "feature_extractor.", "module.")


def save_patchcore_bank(model, path):
    """``np.save`` of the model's memory bank as fp32 [M, 1536] (anomaly_model_train.py:376-385): the file that
    ``load_patchcore(..., memory_bank_npy=path, ...)`` and test.py:169-175 read back."""
    import numpy as np
    bank = model.memory_bank.detach().to("cpu", torch.float32).numpy()
    if bank.ndim != 2 or bank.shape[0] < 1:
        raise ValueError(f"save_patchcore_bank: the model's memory bank {bank.shape} is empty")
    np.save(path, np.ascontiguousarray(bank))


def load_patchcore(backbone_sd, memory_bank_npy, model, trust_pickle=False, knn_precision=None):
    """Load a ``PatchCore``: the ``wide_resnet50_2`` weights and the memory bank (test.py:157-175).

    ``backbone_sd`` is a state_dict (or a file holding one) of torchvision's / timm's ``wide_resnet50_2``, bare or under
    anomalib's ``feature_extractor.`` / ``feature_extractor.feature_extractor.`` prefixes; ``layer4.*`` and ``fc.*`` are
    dropped (layers 2 and 3 do not use them), and so is a ``memory_bank`` entry when ``memory_bank_npy`` is given.
    ``memory_bank_npy`` is a ``.npy`` path (``np.load``ed as test.py:169-175 does) or an array [M, 1536], or None to take
    the state_dict's ``memory_bank``.  Names and shapes of the trunk must match exactly (RuntimeError otherwise).
    ``knn_precision`` (``"fp32"`` / ``"fp16"``, None: leave the model's) is set on the model before the bank is.
    Returns {'n_tensors', 'bank_rows'}."""
    import numpy as np
    data = _read(backbone_sd, trust_pickle)
    if not isinstance(data, dict):
        raise RuntimeError(f"PatchCore backbone: expected a state_dict, got {type(data).__name__}")
    sd, bank = {}, None
    for k, v in data.items():
        for p in _PC_PREFIXES:
            if k.startswith(p):
                k = k[len(p):]
                break
        if k == "memory_bank":
            bank = v
        elif not k.startswith(("layer4.", "fc.")):
            sd[k] = v
    own = model.feature_extractor.state_dict()
    bad = [k for k in sd if k in own and tuple(sd[k].shape) != tuple(own[k].shape)]
    if bad:
        raise RuntimeError(f"PatchCore backbone tensors with the wrong shape: {bad[:5]}")
    missing = [k for k in own if k not in sd]
    unexpected = [k for k in sd if k not in own]
    if missing or unexpected:
        raise RuntimeError(f"PatchCore backbone does not match wide_resnet50_2: missing {missing[:5]} "
                           f"unexpected {unexpected[:5]}")
    model.feature_extractor.load_state_dict({k: torch.as_tensor(v).to(own[k].dtype) for k, v in sd.items()})
    model.invalidate()
    if knn_precision is not None:
        model.knn_precision = knn_precision
    if memory_bank_npy is not None:
        bank = np.load(memory_bank_npy) if isinstance(memory_bank_npy, (str, bytes)) or hasattr(memory_bank_npy, "__fspath__") \
            else memory_bank_npy
    if bank is None:
        raise RuntimeError("PatchCore: no memory bank (pass memory_bank_npy, or a state_dict with 'memory_bank')")
    model.set_memory_bank(bank)
    return {"n_tensors": len(sd), "bank_rows": int(model.memory_bank.shape[0])}


def load_patchcore_classifier(backbone_sd, memory_bank_npy, config, obj, threshold=None, calibration=None, device="cuda",
                              return_map=True, trust_pickle=False, knn_precision="fp32"):
    """Build the hallucination gate (models.py:257-294): a ``PatchCore`` of the mode's input size (84 x 84 for mnist,
    224 x 224 otherwise, ``num_neighbors=9``), loaded by ``load_patchcore`` and moved to ``device`` in ``eval()``, inside
    a ``PatchCoreClassifier``.  ``memory_bank_npy=None`` takes the ``memory_bank`` entry of ``backbone_sd``, the form of
    the reference's mnist checkpoint (a whole-module state_dict, models.py:279); its mvtec / mri banks are ``.npy`` files
    (:281-287).  ``threshold`` / ``calibration`` as in ``PatchCoreClassifier``; ``knn_precision`` as ``PatchCore``'s."""
    from .classifier import PatchCoreClassifier, gate_input_size
    from .patchcore import PatchCore
    S = gate_input_size(str(config["data"]))
    model = PatchCore((S, S), layers=("layer2", "layer3"), backbone="wide_resnet50_2", num_neighbors=9,
                      knn_precision=knn_precision)
    load_patchcore(backbone_sd, memory_bank_npy, model, trust_pickle=trust_pickle)
    model = model.to(device).eval()
    return PatchCoreClassifier(config, obj, model, threshold=threshold, calibration=calibration, return_map=return_map)
