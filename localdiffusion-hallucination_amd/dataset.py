"""Device-resident training data: the reference's ``data.py`` as ``Trainer`` uses it (ddpm.py:1321 / 1352 / 1377, 1538-1553), with
the store in device memory and a step's batches produced there by ``csrc/dataset.hip`` -- one launch per batch (two for mri with
``translate_zero``) from a few bytes of host-drawn parameters, so the host stays off the training step's critical path.

``DeviceDataset`` holds a raw store on the GPU and turns indices (and, under ``augmentations``, an angle and a flip bit per
sample: ``RandomRotation(15)`` + ``RandomVerticalFlip()``, data.py:372-376 / 783-786) into an ``(hr, lr)`` batch for the
denoiser, or an ``(input, target)`` / ``(input, label)`` batch for the two labelled trainers:

* ``DeviceDataset.mnist``  ``data.MNIST`` (data.py:814-836): u8 [N, S, S]; hr = 2 x / 255, lr from the even ROWS (data.py:825
  slices dims 0, 1, 2 of the [1, 1, S, S] image, as ``evalio.mnist_pairs`` pins), bilinear back to S rows;
* ``DeviceDataset.sr``     ``MvtecDatasetSR`` (data.py:287-307, ``train=True``, no ``denoise``, no ``mask_train``): u8 [N, C, S, S]
  already resized (the PIL ``Resize`` is a one-off host step); hr = (x / 255) 2, lr = nearest to S / 2, bilinear back.  The
  reference does not augment this data set; the angle and the flip are honoured as an extension when ``augmentations=True``;
* ``DeviceDataset.mri``    ``MedDataset_png`` (data.py:369-442): two fp32 stores [N, R, R]; centre crop, the SAME rotation and
  flip for both, (x - mean) / std, and with ``translate_zero`` + |min| of the cropped, transformed, normalised image;
* ``DeviceDataset.seg``    ``MedSegDataset`` (data.py:676-743, what ``train_seg.py:51-54`` and so ``SegTrainer`` read) behind the
  ``.mha`` decode: an fp32 store [N, R, R] and a u8 store of ``labels > 0``; centre crop, (x - mean) / std, target = 0 / 1.  The
  reference has its flips commented out (data.py:709-710); the angle and the flip -- the same for image and label -- are
  honoured as an extension when ``augmentations=True``.  ``evalio.lesion_slices`` is its slice filter (data.py:695-698);
* ``DeviceDataset.mnist_cls``  ``data.MNIST`` with its third return value, the label (what ``train_mnist_cls.py:68-71`` and so
  ``MnistClassifierTrainer`` read): the mnist store and a u8 store of the labels, validated on the host once; ``batch`` gives
  ``(x, label)`` with x = mnist's hr and label int64 [B].  No lr is made: the classifier never reads it.

The rotation is torchvision's tensor ``rotate`` (``NEAREST``, ``expand=False``, ``fill=None``) restated from its source; the
package is not available where this was built, so the restatement could not be run against it (it was checked against
``F.grid_sample`` on ``_gen_affine_grid``'s grid: tests/dataset_ref.py).  cos / sin are computed in double on the host and rounded
to fp32; every device operation is a single correctly rounded fp32 operation, so the mnist, mri, seg and mnist_cls batches are
those of the same chain on a CPU, bit for bit, and only the SR path's two-axis bilinear may differ by rounding (ATen may
contract it).

``BatchSource`` is the ``DataLoader``: ``plan(step)`` is a pure function of ``(seed, step)``, so a run resumed at step k, every
rank of a data-parallel run, and a test on the CPU all see the batches an uninterrupted single-GPU run sees at step k.
``SegTrainer.fit`` and ``MnistClassifierTrainer.fit`` take a source too and ask it for ``batches(epoch)``: all three trainers
take their batches the same way, from one seeded plan.

NOT covered: ``MvtecDatasetGray``, the salt-and-pepper ``denoise`` mode, ``mask_train`` / ``select_patch``, the PIL resize, the
nii / OCT / ImageNet loaders, the ``.mha`` decode in front of ``seg``, and a PatchCore bank built from a source.
"""
import math

import numpy as np
import torch

from . import _cabi as cabi
from . import rng

ROW_DTYPE = np.dtype([("src", "<i4"), ("cos_a", "<f4"), ("sin_a", "<f4"), ("flip", "<i4")])     # ld_ds_row
MAX_ANGLE = 15.0                                   # RandomRotation(15): uniform in [-15, 15]
PLAN_STREAM = rng.fnv1a64("BatchSource.plan")      # the plan's streams start here: (PLAN_STREAM + 3 * step + k) mod 2^64


def cos_sin(angle_deg):
    """(cos a, sin a) of an angle in degrees: libm in double, rounded to fp32 -- what a table row carries."""
    a = math.radians(float(angle_deg))
    return np.float32(math.cos(a)), np.float32(math.sin(a))


def crop_offset(size, crop):
    """``CenterCrop``'s top = left: ``int(round((size - crop) / 2))``, Python's round (256 -> 224 starts at 16)."""
    return int(round((size - crop) / 2.0))


def table_rows(indices, n, angles_deg=None, flips=None):
    """The host side of a batch: the ``ld_ds_row`` table (a numpy structured array) for ``indices`` into a store of ``n``
    images.  ``ValueError`` for an empty batch, an index outside ``[0, n)``, or angles / flips of another length."""
    idx = np.asarray(indices)
    if idx.ndim != 1 or idx.size == 0:
        raise ValueError(f"DeviceDataset.batch: indices must be a non-empty 1-d sequence, got shape {idx.shape}")
    if not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"DeviceDataset.batch: indices must be integers, got {idx.dtype}")
    if int(idx.min()) < 0 or int(idx.max()) >= n:
        raise ValueError(f"DeviceDataset.batch: an index lies outside [0, {n}) (min {int(idx.min())}, max {int(idx.max())})")
    rows = np.zeros(idx.size, dtype=ROW_DTYPE)
    rows["src"], rows["cos_a"] = idx, 1.0
    if angles_deg is not None:
        ang = np.asarray(angles_deg, dtype=np.float64)
        if ang.shape != idx.shape or not np.isfinite(ang).all():
            raise ValueError(f"DeviceDataset.batch: {idx.size} indices need {idx.size} finite angles")
        cs = [cos_sin(a) for a in ang]
        rows["cos_a"], rows["sin_a"] = [c for c, _ in cs], [s for _, s in cs]
    if flips is not None:
        fl = np.asarray(flips)
        if fl.shape != idx.shape:
            raise ValueError(f"DeviceDataset.batch: {idx.size} indices need {idx.size} flips")
        rows["flip"] = fl.astype(bool)
    return rows


def _host_u8(images, ndim, what):
    a = images.detach().cpu().numpy() if torch.is_tensor(images) else np.asarray(images)
    if a.dtype != np.uint8 or a.ndim != ndim or a.shape[0] < 1 or a.shape[-1] != a.shape[-2]:
        raise ValueError(f"DeviceDataset.{what}: a uint8 array [N, {'C, ' if ndim == 4 else ''}S, S] with N >= 1, got {a.dtype} "
                         f"{a.shape}")
    if a.shape[-1] < 2 or a.shape[-1] % 2:
        raise ValueError(f"DeviceDataset.{what}: S = {a.shape[-1]} must be even (lr is made from every other row)")
    return torch.from_numpy(np.ascontiguousarray(a))


def _crop_arg(what, crop, size):
    if not isinstance(crop, int) or isinstance(crop, bool) or crop < 4 or crop > size:
        raise ValueError(f"DeviceDataset.{what}: crop = {crop!r} does not fit the {size} x {size} slices")
    if crop % 4:
        raise ValueError(f"DeviceDataset.{what}: crop = {crop} must be a multiple of 4")


class DeviceDataset:
    """A raw store on the GPU and the kernel that makes batches from it: ``(hr, lr)`` for ``mnist``, ``sr`` and ``mri``,
    ``(x, target)`` for ``seg``, ``(x, label)`` for ``mnist_cls``.  ``len()``, ``channels``, ``image_size`` (of a batch),
    ``kind`` and ``augmentations`` say what it is."""

    def __init__(self, kind, stores, channels, image_size, augmentations, device, **params):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"DeviceDataset: device {device}; the batches are made by HIP kernels only (there is no CPU path)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.kind, self.channels, self.image_size = kind, int(channels), int(image_size)
        self.augmentations, self.device, self.params = bool(augmentations), device, params
        self._n = int(stores[0].shape[0])
        self._stores = tuple(s.to(device) for s in stores)

    @classmethod
    def mnist(cls, images_u8, *, augmentations=False, device="cuda"):
        """``images_u8``: uint8 [N, S, S] (S = 28), the digits in file order (``evalio.select_digits``)."""
        x = _host_u8(images_u8, 3, "mnist")
        return cls("mnist", (x,), 1, x.shape[-1], augmentations, device)

    @classmethod
    def sr(cls, images_u8, *, augmentations=False, device="cuda"):
        """``images_u8``: uint8 [N, C, S, S], C = 1 or 3, already resized to the training size S (even)."""
        x = _host_u8(images_u8, 4, "sr")
        if x.shape[1] not in (1, 3):
            raise ValueError(f"DeviceDataset.sr: C = {x.shape[1]} (1 or 3)")
        return cls("sr", (x,), x.shape[1], x.shape[-1], augmentations, device)

    @classmethod
    def mri(cls, target, cond, *, mean_target, std_target, mean_cond, std_cond, translate_zero=True, crop=224,
            augmentations=False, device="cuda"):
        """``target`` / ``cond``: [N, R, R] slices of the image's and the condition's modality (converted to fp32, finite);
        the constants are the config's ``mean_* / std_*`` of the two modalities.  hr comes from ``target``, lr from ``cond``."""
        host = []
        for name, a in (("target", target), ("cond", cond)):
            a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
            if a.ndim != 3 or a.shape[0] < 1 or a.shape[1] != a.shape[2]:
                raise ValueError(f"DeviceDataset.mri: {name} must be [N, R, R] with N >= 1, got {a.shape}")
            a = np.ascontiguousarray(a, dtype=np.float32)
            if not np.isfinite(a).all():
                raise ValueError(f"DeviceDataset.mri: {name} holds a non-finite value (the minimum would not be torch's)")
            host.append(torch.from_numpy(a))
        if host[0].shape != host[1].shape:
            raise ValueError(f"DeviceDataset.mri: target {tuple(host[0].shape)} and cond {tuple(host[1].shape)} differ")
        size = int(host[0].shape[-1])
        _crop_arg("mri", crop, size)
        consts = {}
        for name, v in (("mean_target", mean_target), ("std_target", std_target), ("mean_cond", mean_cond), ("std_cond", std_cond)):
            v = float(np.float32(v))
            if not math.isfinite(v) or (name.startswith("std") and not v > 0.0):
                raise ValueError(f"DeviceDataset.mri: {name} = {v!r} must be finite{' and positive' if name.startswith('std') else ''}")
            consts[name] = v
        return cls("mri", tuple(host), 1, crop, augmentations, device, translate_zero=bool(translate_zero), size=size, **consts)

    @classmethod
    def seg(cls, images, labels, *, mean, std, crop=224, augmentations=False, device="cuda"):
        """``images``: [N, R, R] slices (converted to fp32, finite); ``labels``: [N, R, R] of any real or bool dtype, stored
        once as u8 of ``labels > 0``; ``mean`` / ``std``: the config's ``mean_flair`` / ``std_flair``.  ``batch`` gives
        ``(x, target)``, both fp32 [B, 1, crop, crop].  (``SegUNet`` wants multiples of 16: the trainer's own check.)"""
        img = images.detach().cpu().numpy() if torch.is_tensor(images) else np.asarray(images)
        lab = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
        if img.ndim != 3 or img.shape[0] < 1 or img.shape[1] != img.shape[2]:
            raise ValueError(f"DeviceDataset.seg: images must be [N, R, R] with N >= 1, got {img.shape}")
        if lab.shape != img.shape:
            raise ValueError(f"DeviceDataset.seg: images {img.shape} and labels {lab.shape} differ")
        if not (np.issubdtype(lab.dtype, np.integer) or np.issubdtype(lab.dtype, np.floating) or lab.dtype == np.bool_):
            raise ValueError(f"DeviceDataset.seg: labels must be real or bool, got {lab.dtype}")
        img = np.ascontiguousarray(img, dtype=np.float32)
        if not np.isfinite(img).all():
            raise ValueError("DeviceDataset.seg: images hold a non-finite value")
        if np.issubdtype(lab.dtype, np.floating) and np.isnan(lab).any():
            raise ValueError("DeviceDataset.seg: labels hold a NaN")
        size = int(img.shape[-1])
        _crop_arg("seg", crop, size)
        consts = {}
        for name, v in (("mean", mean), ("std", std)):
            v = float(np.float32(v))
            if not math.isfinite(v) or (name == "std" and not v > 0.0):
                raise ValueError(f"DeviceDataset.seg: {name} = {v!r} must be finite{' and positive' if name == 'std' else ''}")
            consts[name] = v
        lab = np.ascontiguousarray(lab > 0).astype(np.uint8)
        return cls("seg", (torch.from_numpy(img), torch.from_numpy(lab)), 1, crop, augmentations, device, size=size, **consts)

    @classmethod
    def mnist_cls(cls, images_u8, labels, *, augmentations=False, device="cuda"):
        """``images_u8``: uint8 [N, S, S] as for ``mnist``; ``labels``: an integer array [N], every value in 0..9 (checked here,
        once, so that ``MnistClassifierTrainer``'s ``bad_label`` flag never fires on a source).  ``batch`` gives ``(x, label)``:
        x = ``mnist``'s hr, label int64 [B] on the device."""
        x = _host_u8(images_u8, 3, "mnist_cls")
        y = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
        if y.ndim != 1 or y.shape[0] != x.shape[0]:
            raise ValueError(f"DeviceDataset.mnist_cls: {x.shape[0]} images need {x.shape[0]} labels, got shape {y.shape}")
        if not np.issubdtype(y.dtype, np.integer):
            raise ValueError(f"DeviceDataset.mnist_cls: labels must be integers, got {y.dtype}")
        if int(y.min()) < 0 or int(y.max()) > 9:
            raise ValueError(f"DeviceDataset.mnist_cls: a label lies outside 0..9 (min {int(y.min())}, max {int(y.max())})")
        return cls("mnist_cls", (x, torch.from_numpy(np.ascontiguousarray(y.astype(np.uint8)))), 1, x.shape[-1], augmentations, device)

    def __len__(self):
        return self._n

    def _out_spec(self, B):
        """(shape, dtype) of the two tensors ``batch`` returns."""
        shape = (B, self.channels, self.image_size, self.image_size)
        if self.kind == "mnist_cls":
            return (shape, torch.float32), ((B,), torch.int64)
        return (shape, torch.float32), (shape, torch.float32)

    def batch(self, indices, angles_deg=None, flips=None, out=None):
        """``(hr, lr)`` -- ``(x, target)`` for ``seg`` -- fp32 [B, channels, image_size, image_size], or ``(x, label)`` with
        label int64 [B] for ``mnist_cls``, on the device for the images ``indices`` (a sequence of
        ints, repeats allowed), sample k rotated by ``angles_deg[k]`` degrees (positive: counter-clockwise) and then flipped
        vertically where ``flips[k]``.  Without ``augmentations`` both must be ``None``.  ``ValueError`` -- before anything
        is uploaded or launched -- for an index outside ``[0, len)``, an empty batch, or parameters that do not fit.  The table
        goes up from pinned memory without waiting and the launch follows it on the current stream: no host synchronisation.
        ``out``: a ready pair of contiguous device tensors of the batch's shapes and dtypes to write into (two fp32 tensors;
        an fp32 and an int64 tensor for ``mnist_cls``), checked before anything is uploaded."""
        if not self.augmentations and (angles_deg is not None or flips is not None):
            raise ValueError("DeviceDataset.batch: angles / flips given, but the data set was built with augmentations=False")
        rows = table_rows(indices, self._n, angles_deg, flips)
        B, dev, lib = rows.size, self.device, cabi.lib()
        spec = self._out_spec(B)
        if out is not None:
            out = tuple(out)
            if len(out) != 2 or not all(torch.is_tensor(t) and t.dtype == dt and t.is_contiguous() and t.device == dev
                                        and tuple(t.shape) == shape for t, (shape, dt) in zip(out, spec)):
                if self.kind == "mnist_cls":
                    raise ValueError(f"DeviceDataset.batch: out must be a contiguous fp32 tensor {spec[0][0]} and a contiguous int64 "
                                     f"tensor {spec[1][0]} on {dev}")
                raise ValueError(f"DeviceDataset.batch: out must be two contiguous fp32 tensors {spec[0][0]} on {dev}")
        with torch.cuda.device(dev):
            pinned = torch.empty(rows.nbytes, dtype=torch.uint8, pin_memory=True)
            pinned.numpy()[:] = rows.view(np.uint8)
            table = pinned.to(dev, non_blocking=True)          # (the pinned block is not reused before the copy has run)
            hr, lr = out if out is not None else (torch.empty(shape, dtype=dt, device=dev) for shape, dt in spec)
            st = torch.cuda.current_stream(dev).cuda_stream
            if self.kind == "mnist":
                rc = lib.ld_ds_mnist_batch(self._stores[0].data_ptr(), self._n, self.image_size, table.data_ptr(), B,
                                           hr.data_ptr(), lr.data_ptr(), st)
            elif self.kind == "sr":
                rc = lib.ld_ds_sr_batch(self._stores[0].data_ptr(), self._n, self.channels, self.image_size, table.data_ptr(), B,
                                        hr.data_ptr(), lr.data_ptr(), st)
            elif self.kind == "seg":
                p = self.params
                rc = lib.ld_ds_seg_batch(self._stores[0].data_ptr(), self._stores[1].data_ptr(), self._n, p["size"], self.image_size,
                                         table.data_ptr(), B, p["mean"], p["std"], hr.data_ptr(), lr.data_ptr(), st)
            elif self.kind == "mnist_cls":
                rc = lib.ld_ds_mnist_cls_batch(self._stores[0].data_ptr(), self._stores[1].data_ptr(), self._n, self.image_size,
                                               table.data_ptr(), B, hr.data_ptr(), lr.data_ptr(), st)
            else:
                p = self.params
                work = torch.empty(B * 2 * cabi.DS_MIN_PARTS, dtype=torch.float32, device=dev) if p["translate_zero"] else None
                rc = lib.ld_ds_mri_batch(self._stores[0].data_ptr(), self._stores[1].data_ptr(), self._n, p["size"], self.image_size,
                                         table.data_ptr(), B, p["mean_target"], p["std_target"], p["mean_cond"], p["std_cond"],
                                         int(p["translate_zero"]), cabi.ptr(work), hr.data_ptr(), lr.data_ptr(), st)
            cabi.check(rc, f"ds_{self.kind}_batch")
        return hr, lr


class StepBatches:
    """What ``BatchSource.batches(step)`` returns: sized (``len()``, ``sizes``), and lazy -- iterating asks the data set for
    batch k + 1 only after batch k has been handed out."""

    def __init__(self, dataset, batch_size, n_batches, plan):
        self.dataset, self.batch_size, self.n_batches, self.plan = dataset, batch_size, n_batches, plan
        total = len(plan["indices"])
        self.sizes = [min(batch_size, total - k * batch_size) for k in range(n_batches)]

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        idx, ang, fl = self.plan["indices"], self.plan["angles_deg"], self.plan["flips"]
        for k in range(self.n_batches):
            sl = slice(k * self.batch_size, k * self.batch_size + self.sizes[k])
            yield self.dataset.batch(idx[sl], None if ang is None else ang[sl], None if fl is None else fl[sl])


class BatchSource:
    """``BatchSource(dataset, batch_size, *, shuffle=True, seed=42, drop_last=False)``: the ``DataLoader`` of ddpm.py:1321 /
    1352 / 1377 over a ``DeviceDataset`` (anything with ``len()``, ``augmentations`` and ``batch(indices, angles_deg, flips)``).
    ``len(source)`` is the number of batches of a step; the last one is ragged unless ``drop_last``.

    A validation set is ``BatchSource(unaugmented_dataset, batch_size, shuffle=False)``, whose ``list(source.batches(0))`` may
    be materialised once and handed to ``DenoiserTrainer.evaluate``."""

    def __init__(self, dataset, batch_size, *, shuffle=True, seed=42, drop_last=False):
        if not isinstance(batch_size, int) or isinstance(batch_size, bool) or batch_size < 1:
            raise ValueError(f"BatchSource: batch_size = {batch_size!r} must be an int of at least 1")
        n = len(dataset)
        self.dataset, self.batch_size, self.shuffle, self.seed = dataset, batch_size, bool(shuffle), int(seed)
        self.drop_last = bool(drop_last)
        self.n_batches = n // batch_size if drop_last else -(-n // batch_size)
        if self.n_batches < 1:
            raise ValueError(f"BatchSource: {n} images make no batch of {batch_size}" + (" with drop_last" if drop_last else ""))

    def __len__(self):
        return self.n_batches

    def plan(self, step):
        """What step ``step`` trains on: ``{"indices": int64 [M], "angles_deg": float64 [M] or None, "flips": bool [M] or
        None}``, M = the images of the step's batches in order (``len(dataset)``, or ``len(source) * batch_size`` with
        ``drop_last``); batch k is positions ``[k * batch_size, (k + 1) * batch_size)``.  A PURE FUNCTION of ``(seed, step)``,
        built on ``rng``'s counter generator (``rng.bits64(n, seed, stream)``, n = ``len(dataset)``) with three streams
        derived from the step, ``stream_k = (fnv1a64("BatchSource.plan") + 3 * step + k) mod 2^64``:

        * k = 0, the permutation (``shuffle``; else the identity): the stable argsort of the stream's n 64-bit words;
        * k = 1, the angles (``dataset.augmentations``; else None): position p gets ``-15 + 30 * (word_p >> 11) * 2^-53``
          degrees, uniform in [-15, 15) (the sign convention does not change the distribution: the interval is symmetric);
        * k = 2, the flips (likewise): position p flips when the top bit of ``word_p`` is set.

        Angle and flip belong to the POSITION in the shuffled order, not to the image."""
        step = int(step)
        if step < 0:
            raise ValueError(f"BatchSource.plan: step = {step}")
        n = len(self.dataset)
        streams = [(PLAN_STREAM + 3 * step + k) & ((1 << 64) - 1) for k in range(3)]
        if self.shuffle:
            perm = np.argsort(rng.bits64(n, self.seed, streams[0]), kind="stable").astype(np.int64)
        else:
            perm = np.arange(n, dtype=np.int64)
        m = self.n_batches * self.batch_size if self.drop_last else n
        angles = flips = None
        if self.dataset.augmentations:
            u = (rng.bits64(n, self.seed, streams[1]) >> np.uint64(11)).astype(np.float64) * (2.0 ** -53)
            angles = (-MAX_ANGLE + 2.0 * MAX_ANGLE * u)[:m]
            flips = ((rng.bits64(n, self.seed, streams[2]) >> np.uint64(63)) != 0)[:m]
        return {"indices": perm[:m], "angles_deg": angles, "flips": flips}

    def batches(self, step):
        """The step's batches, each what the data set's ``batch`` returns: a sized, lazy iterable (``StepBatches``)."""
        return StepBatches(self.dataset, self.batch_size, self.n_batches, self.plan(step))


def epoch_batches(batches, epoch=0):
    """What a trainer's ``fit`` walks: a ``BatchSource``'s lazy ``batches(epoch)``, a callable's ``batches(epoch)``, else the
    sequence itself.  Evaluation passes no epoch: a source is walked as ``batches(0)`` every time."""
    if isinstance(batches, BatchSource):
        return batches.batches(epoch)
    return batches(epoch) if callable(batches) else batches
