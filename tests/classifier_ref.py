"""Plain-torch restatement of the reference's hallucination gate (``Classifier_PatchCore.forward``, models.py:404-430)
on top of tests/patchcore_ref.py: the oracle of tests/test_hip_classifier.py.  Only tensor ops and F.interpolate; runs on
the CPU in the dtype of its input, so the same code evaluated in fp64 is the yardstick for the fp32 rounding."""
import torch
import torch.nn.functional as F

import patchcore_ref

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def input_size(mode):
    return 84 if "mnist" in mode else 224


def mri_affine(x, config, obj):
    """The MRI branch: x - mini with mini = (0 - mean) / std (not - |mini|), * std + mean, / 4096."""
    key = "flair" if obj == "flair" else "t1"
    mean, std = config["mean_" + key], config["std_" + key]
    mini = (0 - mean) / std
    x = x - mini
    x = x * std + mean
    return x / 4096.0


def preprocess(x, config, obj, per_sample_max=False, size=None):
    """x [B, 1 or 3, H, W] -> PatchCore's input [B, 3, S, S].  ``per_sample_max``: the halving decided per sample (a
    batch of independent B = 1 calls) instead of on the whole tensor, which is what the reference's forward does."""
    mode = config["data"]
    if x.shape[1] != 3:
        x = x.repeat(1, 3, 1, 1)
    if "mvtec" in mode or "mnist" in mode:
        if per_sample_max:
            over = x.reshape(x.shape[0], -1).max(1).values > 1.0
            x = torch.where(over.view(-1, 1, 1, 1), x / 2.0, x)
        elif x.max() > 1.0:
            x = x / 2.0
    else:
        x = mri_affine(x, config, obj)
    S = input_size(mode) if size is None else size
    x = F.interpolate(x, size=(S, S), mode="bilinear", align_corners=False)
    mean = torch.tensor(IMAGENET_MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=x.dtype).view(1, 3, 1, 1)
    return (x - mean) / std


def resize_back(amap, H, W):
    return F.interpolate(amap, size=(H, W), mode="bilinear", align_corners=False)


def classifier_forward(sd, bank, x0, config, obj, threshold, num_neighbors=9, per_sample_max=False):
    """-> (decision [B] of 0 / 1, anomaly_map [B, 1, H, W], pred_score [B], PatchCore's input)."""
    with torch.no_grad():
        x = preprocess(x0.float(), config, obj, per_sample_max)
        S = x.shape[-1]
        out = patchcore_ref.patchcore_forward(sd, bank, x, (S, S), num_neighbors)
        amap = resize_back(out["anomaly_map"], x0.shape[-2], x0.shape[-1])
        score = out["pred_score"]
    return (score > threshold).to(torch.int32), amap, score, x


def gate(sd, bank, config, obj, threshold, num_neighbors=9, record=None):
    """A callable for a sampler's ``.classifier``: x0 -> (1 or 0, map, score); appends each score to ``record``."""
    def call(x0):
        d, amap, score, _ = classifier_forward(sd, bank, x0.detach().cpu(), config, obj, threshold, num_neighbors)
        if record is not None:
            record.append(float(score[0]))
        return int(d[0]), amap, score
    return call
