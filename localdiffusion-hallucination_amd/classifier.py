"""The reference's hallucination gate (``models.Classifier_PatchCore``, models.py:257-430) on the HIP kernels of
``csrc/classifier.hip`` around ``PatchCore``: the real / hallucinated decision that ``fusion()`` (ddpm.py:883-916) asks
for on the fused x0 at every joint step until one prediction is accepted.

``PatchCoreClassifier`` is what goes into ``GaussianDiffusion.classifier``.  A call is

* the preprocessing of models.py:404-424 in two launches (one in the MRI mode): C = 1 read as three channels, the whole
  tensor halved when its max is above 1.0 (mnist / mvtec*) or de-normalised with the config's statistics (mri), bilinear
  resize to PatchCore's input size, ImageNet ``Normalize`` -- the max stays in device memory;
* ``PatchCore`` (trunk, embedding, kNN, image score; the blurred map only when it is asked for);
* the bilinear resize of the anomaly map back to the image size and the decision ``pred_score > threshold`` on the
  device, in one launch.

``predict`` never synchronises with the host; ``forward`` copies the 4-byte decision back, the one round trip of a call
(the reference makes two, ``hr.max() > 1.0`` and ``pred_score > threshold``).  ``calc_threshold`` / ``youden_threshold``
restate the calibration of models.py:338-402 (``sklearn.metrics.roc_curve`` + the maximum of TPR - FPR) without sklearn.
Not covered: the reference's dataset construction and its hard-coded bank paths (``checkpoint.load_patchcore_classifier``
takes the files).
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _cabi as cabi

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
MRI_STATS = ("mean_flair", "std_flair", "mean_t1", "std_t1")


def gate_input_size(mode):
    """PatchCore's input side for config['data'] (models.py:272-275): 84 for mnist, 224 otherwise."""
    return 84 if "mnist" in mode else 224


def youden_threshold(scores, labels):
    """The threshold of models.py:392-401: ``fpr, tpr, thresholds = sklearn.metrics.roc_curve(labels + 1, scores,
    pos_label=2)`` (``drop_intermediate=True``), then ``thresholds[np.argmax(tpr - fpr)]``.  labels: 0 = normal, 1 =
    anomalous.  Pure numpy; reproduces sklearn's curve point for point -- the points collinear with their neighbours are
    dropped before the maximum is taken, because TPR - FPR values that are equal on paper can differ in the last bit and
    the first maximum wins.  ``thresholds[0]`` is +inf (sklearn >= 1.3) and a legal result: no score exceeds it.
    ValueError unless both classes are present."""
    s = np.asarray(scores).reshape(-1)
    y = np.asarray(labels).reshape(-1)
    if s.size != y.size or s.size == 0:
        raise ValueError(f"youden_threshold: {s.size} scores, {y.size} labels")
    if not np.all(np.isfinite(s.astype(np.float64))):
        raise ValueError("youden_threshold: scores must be finite")
    if not np.all((y == 0) | (y == 1)):
        raise ValueError("youden_threshold: labels must be 0 (normal) or 1 (anomalous)")
    pos = y == 1
    if pos.all() or not pos.any():
        raise ValueError("youden_threshold: the calibration set needs both normal and anomalous images")
    order = np.argsort(s, kind="mergesort")[::-1]               # descending; ties in reversed input order, as sklearn
    s, pos = s[order], pos[order]
    idx = np.r_[np.where(np.diff(s))[0], s.size - 1]            # last index of every run of equal scores
    tps = np.cumsum(pos * 1.0, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    thr = s[idx]
    if len(fps) > 2:                                            # drop_intermediate: keep the corners of the curve
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thr = fps[keep], tps[keep], thr[keep]
    tps, fps, thr = np.r_[0, tps], np.r_[0, fps], np.r_[np.inf, thr]
    fpr, tpr = fps / fps[-1], tps / tps[-1]
    return float(thr[np.argmax(tpr - fpr)])


class PatchCoreClassifier(nn.Module):
    """``PatchCoreClassifier(config, obj, patchcore, threshold=None, calibration=None, return_map=True)``.

    ``config['data']`` selects the mode as the reference does: ``'mnist' in mode`` / ``'mvtec' in mode`` halve the tensor
    when its max is above 1.0, every other mode is the MRI branch, which de-normalises with ``mean_flair`` / ``std_flair``
    (``obj == 'flair'``) or ``mean_t1`` / ``std_t1`` from ``config``.  ``patchcore`` is a prepared ``PatchCore`` (weights
    and memory bank loaded, on the GPU, in ``eval()``) whose square ``input_size`` is the mode's (84 for mnist, 224
    otherwise).  ``threshold``, or ``calibration=(images, labels)`` for ``calc_threshold``: one of the two is required
    (the reference would read its authors' test set from a fixed path).  ``knn_precision`` (``"fp32"`` / ``"fp16"``) is
    set on ``patchcore`` (see ``PatchCore.knn_precision``; also readable and assignable here afterwards).

    ``classifier(x0)`` returns the reference's triple ``(decision, anomaly_map, pred_score)``: a Python int 1 / 0
    (``pred_score > threshold``), the map [B, 1, H, W] on the device (``None`` with ``return_map=False``: then neither the
    blur nor the resize back is launched) and the score as a device tensor.  B must be 1, as in the reference;
    ``predict`` takes any B and returns device tensors only.

    The map is resized to x0's own H x W.  The reference's ``forward`` reads ``self.img_size``, which only its
    ``calc_threshold`` sets (to the width of the calibration images), so with a threshold passed in it raises
    ``AttributeError``; x0's size is what ``calc_threshold`` would have found for a data set of that size."""

    def __init__(self, config, obj, patchcore, threshold=None, calibration=None, return_map=True, knn_precision=None):
        super().__init__()
        if knn_precision is not None:                  # passed through to PatchCore, which checks it; None: leave its own
            patchcore.knn_precision = knn_precision
        self.config, self.mode, self.obj = config, str(config["data"]), obj
        self.halve = ("mvtec" in self.mode) or ("mnist" in self.mode)
        if not self.halve:
            missing = [k for k in MRI_STATS if k not in config]
            if missing:
                raise ValueError(f"PatchCoreClassifier: data {self.mode!r} is the MRI branch and needs {missing} in config")
            mean, std = (config["mean_flair"], config["std_flair"]) if obj == "flair" else (config["mean_t1"], config["std_t1"])
            if float(std) == 0.0:
                raise ValueError("PatchCoreClassifier: std is 0")
            self.affine = (float((0 - mean) / std), float(std), float(mean), 4096.0)     # ((x - mini) * std + mean) / 4096
        else:
            self.affine = (0.0, 1.0, 0.0, 1.0)
        S = gate_input_size(self.mode)
        size = tuple(int(v) for v in getattr(patchcore, "input_size", ()))
        if size != (S, S):
            raise ValueError(f"PatchCoreClassifier: data {self.mode!r} runs PatchCore at {S}x{S}, this one has input_size {size}")
        self.patchcore = patchcore
        self.size = S
        self.return_map = bool(return_map)
        self._plans = {}
        if threshold is None and calibration is None:
            raise ValueError("PatchCoreClassifier: pass threshold=, or calibration=(images, labels) to compute it "
                             "(there is no default calibration set)")
        self.threshold = None if threshold is None else float(threshold)
        if threshold is None:
            self.calc_threshold(*calibration)

    @property
    def knn_precision(self):
        return self.patchcore.knn_precision

    @knn_precision.setter
    def knn_precision(self, value):
        self.patchcore.knn_precision = value

    # ------------------------------------------------------------------ buffers
    def _plan(self, B, H, W, dev):
        key = (B, H, W, str(dev))
        plan = self._plans.get(key)
        if plan is None:
            S = self.size
            plan = {"x": torch.empty((B, 3, S, S), dtype=torch.float32, device=dev),
                    "words": torch.zeros((2, B), dtype=torch.int32, device=dev),      # two sets of max words, see predict
                    "phase": 0,
                    "decision": torch.empty(B, dtype=torch.int32, device=dev),
                    "map": torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)}
            self._plans[key] = plan
        return plan

    def _check(self, x0):
        if not torch.is_tensor(x0) or x0.dim() != 4 or x0.shape[1] not in (1, 3) or x0.shape[0] < 1:
            raise ValueError(f"PatchCoreClassifier: input {tuple(getattr(x0, 'shape', ()))}, expected [B, 1 or 3, H, W]")
        if self.threshold is None:
            raise RuntimeError("PatchCoreClassifier: no threshold yet")
        if not torch.cuda.is_available():
            raise RuntimeError("PatchCoreClassifier needs a GPU (HIP kernels only; there is no CPU fallback)")
        if not x0.is_cuda:
            raise ValueError("PatchCoreClassifier: the input must be a CUDA tensor on PatchCore's device")
        return x0.detach().to(torch.float32).contiguous()

    # ------------------------------------------------------------------ launches
    def preprocess(self, x0, per_sample_max=False):
        """x0 [B, 1 or 3, H, W] on the GPU -> PatchCore's input [B, 3, S, S] (models.py:405-424), a view of the plan's
        buffer: the next call with the same shape overwrites it."""
        x0 = self._check(x0)
        B, C, H, W = x0.shape
        dev = x0.device
        plan = self._plan(B, H, W, dev)
        lib = cabi.lib()
        st = torch.cuda.current_stream(dev).cuda_stream
        a = cabi.ClfResizeArgs()
        a.x, a.out = x0.data_ptr(), plan["x"].data_ptr()
        a.B, a.Cin, a.Cout, a.Hi, a.Wi, a.Ho, a.Wo = B, C, 3, H, W, self.size, self.size
        if self.halve:
            # call i accumulates the max into set i & 1 of the words (zero on entry); its resize launch clears the other
            # set, last read by the resize of call i - 1 on this stream: no launch of its own to reset a word
            words, ph = plan["words"], plan["phase"]
            groups = B if per_sample_max else 1
            try:
                cabi.check(lib.ld_clf_max(x0.data_ptr(), groups, x0.numel() // groups, words[ph].data_ptr(), st), "clf_max")
                a.mode, a.max_words, a.per_sample = cabi.CLF_HALVE, words[ph].data_ptr(), int(bool(per_sample_max))
                a.zero_words, a.n_zero = words[1 - ph].data_ptr(), B
                self._fill_normalize(a)
                cabi.check(lib.ld_clf_resize(ctypes.byref(a), st), "clf_resize")
            except Exception:
                self._plans.pop((B, H, W, str(dev)), None)             # the words may be half-used: start from a clean plan
                raise
            plan["phase"] = 1 - ph
        else:
            a.mode = cabi.CLF_AFFINE
            a.sub, a.mul, a.add, a.div = self.affine
            self._fill_normalize(a)
            cabi.check(lib.ld_clf_resize(ctypes.byref(a), st), "clf_resize")
        return plan["x"]

    @staticmethod
    def _fill_normalize(a):
        a.normalize = 1
        for c in range(3):
            a.mean[c], a.std[c] = IMAGENET_MEAN[c], IMAGENET_STD[c]

    def predict(self, x0, per_sample_max=False, return_map=None):
        """x0 [B, 1 or 3, H, W] fp32 on the GPU, any B -> (decision [B] int32, anomaly_map [B, 1, H, W] or None,
        pred_score [B]), all on the device, without any host synchronisation.  ``per_sample_max=False`` decides the
        halving on the max of the whole tensor, as the reference's ``forward`` does; ``True`` on each sample's own max,
        which makes a batch equal to its B = 1 calls (the reference calibrates with batch size 1).  ``decision`` and the
        map live in per-shape buffers that the next call with the same shape overwrites."""
        want_map = self.return_map if return_map is None else bool(return_map)
        x = self.preprocess(x0, per_sample_max)
        B, _, H, W = x0.shape
        dev = x.device
        plan = self._plan(B, H, W, dev)
        lib = cabi.lib()
        pc = self.patchcore
        pred, scores, (h, w) = pc.score(x)
        st = torch.cuda.current_stream(dev).cuda_stream
        decision = plan["decision"]
        if not want_map:
            cabi.check(lib.ld_clf_decide(pred.data_ptr(), self.threshold, decision.data_ptr(), B, st), "clf_decide")
            return decision, None, pred
        amap = pc.anomaly_map_of(scores, B, h, w)
        a = cabi.ClfResizeArgs()
        a.x, a.out = amap.data_ptr(), plan["map"].data_ptr()
        a.B, a.Cin, a.Cout, a.Hi, a.Wi, a.Ho, a.Wo = B, 1, 1, self.size, self.size, H, W
        a.mode = cabi.CLF_PLAIN
        a.pred, a.threshold, a.decision, a.n_decision = pred.data_ptr(), self.threshold, decision.data_ptr(), B
        cabi.check(lib.ld_clf_resize(ctypes.byref(a), st), "clf_resize")
        return decision, plan["map"], pred

    def forward(self, x0):
        """The reference's ``forward`` (models.py:404-430): -> (1 or 0, anomaly_map or None, pred_score)."""
        if torch.is_tensor(x0) and x0.dim() == 4 and x0.shape[0] != 1:
            raise ValueError(f"PatchCoreClassifier: the gate is a batch-1 model (`if pred_score > threshold`), got B = "
                             f"{x0.shape[0]}; predict() scores a batch")
        decision, amap, pred = self.predict(x0)
        return int(decision.item()), amap, pred

    # ------------------------------------------------------------------ calibration
    def scores(self, images, batch_size=8):
        """pred_score of every calibration image, each preprocessed on its own (``per_sample_max=True``): images is a
        tensor / array [N, C, H, W] or an iterable of such batches.  -> float32 numpy [N]."""
        dev = self.patchcore.feature_extractor.conv1.weight.device
        if torch.is_tensor(images) or isinstance(images, np.ndarray):
            t = torch.as_tensor(images)
            batches = (t[i:i + batch_size] for i in range(0, t.shape[0], batch_size))
        else:
            batches = (torch.as_tensor(b) for b in images)
        saved, self.threshold = self.threshold, (0.0 if self.threshold is None else self.threshold)
        try:
            out = [self.predict(b.to(dev, torch.float32), per_sample_max=True, return_map=False)[2] for b in batches]
        finally:
            self.threshold = saved
        if not out:
            raise ValueError("PatchCoreClassifier: no calibration images")
        return torch.cat(out).cpu().numpy()

    def calc_threshold(self, images, labels, batch_size=8):
        """models.py:338-402: score every calibration image and set ``threshold`` to the one that maximises TPR - FPR
        (``youden_threshold``).  labels: 0 = normal, 1 = anomalous (the reference's ``cls``).  Returns the threshold."""
        labels = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).reshape(-1)
        s = self.scores(images, batch_size)
        if s.size != labels.size:
            raise ValueError(f"PatchCoreClassifier.calc_threshold: {s.size} images, {labels.size} labels")
        self.threshold = youden_threshold(s, labels)
        return self.threshold
