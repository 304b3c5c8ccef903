"""Pure-torch CPU restatements of the two labelled ``__getitem__``s that ``DeviceDataset.seg`` and ``DeviceDataset.mnist_cls``
replace (the reference's ``MedSegDataset``, data.py:676-743, and ``MNIST`` with its label, data.py:814-836), defined through
the yardsticks of tests/dataset_ref.py.  Nothing here reads the reference tree or touches a GPU.

``seg_batch``: the image goes through ``dataset_ref.mri_batch`` without ``translate_zero`` -- centre crop, rotation, flip,
``(x - mean) / std``; the fill of the rotation's corners comes before the normalisation -- and the target is the same call on
``(labels > 0)`` as fp32 with mean 0 and std 1: ``(v - 0) / 1`` of 0.0 / 1.0 is exact, so the target holds 0.0 and 1.0 only.
``mnist_cls_batch``: ``dataset_ref.mnist_batch``'s hr and the labels of the chosen digits as int64."""
import numpy as np
import torch

import dataset_ref as D


def seg_batch(images, labels, indices, angles_deg=None, flips=None, *, mean, std, crop):
    """-> (x, target), both fp32 [B, 1, crop, crop]."""
    images = np.asarray(images, dtype=np.float32)
    x = D.mri_batch(images, images, indices, angles_deg, flips, mean_target=mean, std_target=std, mean_cond=mean, std_cond=std,
                    translate_zero=False, crop=crop)[0]
    binary = (np.asarray(labels) > 0).astype(np.float32)
    target = D.mri_batch(binary, binary, indices, angles_deg, flips, mean_target=0.0, std_target=1.0, mean_cond=0.0, std_cond=1.0,
                         translate_zero=False, crop=crop)[0]
    return x, target


def mnist_cls_batch(store, labels, indices, angles_deg=None, flips=None):
    """-> (x fp32 [B, 1, S, S], label int64 [B])."""
    x = D.mnist_batch(store, indices, angles_deg, flips)[0]
    label = torch.from_numpy(np.asarray(labels)[np.asarray(indices, dtype=np.int64)].astype(np.int64))
    return x, label
