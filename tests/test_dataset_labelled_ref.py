"""CPU checks under the GPU tests of tests/test_hip_dataset_labelled.py: the two labelled yardsticks
(tests/dataset_labelled_ref.py) equal the plain spelling of what they restate, ``evalio.lesion_slices`` is the reference's slice
filter, the C ABI declares, binds and exports the two entry points, and enough candidate angles pass the tie screen at every
size the GPU tests use -- so that a GPU test can fail only for the kernels' reasons."""
import os
import re

import numpy as np
import pytest
import torch

from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import evalio, rng

import dataset_labelled_ref as L
import dataset_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG_KW = dict(mean=412.7, std=151.3)
SEG_SIZES = ((24, 16), (20, 20), (21, 16), (23, 16))      # (R, crop); the last two: half-to-even offsets (2.5 -> 2, 3.5 -> 4)
GPU_TEST_SIZES = (16, 20, 28, 32, 36)                     # every H = W the GPU tests rotate at
NEW_ENTRY_POINTS = ("ld_ds_seg_batch", "ld_ds_mnist_cls_batch")


def seg_stores(R):
    images = rng.uniform((5, R, R), 77, 100 + R, 0.0, 4096.0)
    pick = (rng.bits64(5 * R * R, 77, 300 + R) >> np.uint64(32)) % np.uint64(6)
    labels = np.array([0, 0, 0, 1, 2, 4], dtype=np.uint8)[pick.astype(np.int64)].reshape(5, R, R)
    return images, labels


@pytest.mark.parametrize("R, crop", SEG_SIZES)
def test_seg_batch_without_parameters_is_the_plain_spelling(R, crop):
    images, labels = seg_stores(R)
    idx = [4, 1, 1, 0]
    top = {(24, 16): 4, (20, 20): 0, (21, 16): 2, (23, 16): 4}[(R, crop)]
    assert D.crop_offset(R, crop) == top
    x, target = L.seg_batch(images, labels, idx, crop=crop, **SEG_KW)
    assert x.shape == target.shape == (4, 1, crop, crop) and x.dtype == target.dtype == torch.float32
    img = torch.from_numpy(images)[idx][:, None, top:top + crop, top:top + crop]
    assert torch.equal(x, (img - SEG_KW["mean"]) / SEG_KW["std"])
    want = (torch.from_numpy(labels)[idx][:, None, top:top + crop, top:top + crop] > 0).float()
    assert torch.equal(target, want)
    assert 0.2 < float(want.mean()) < 0.8                  # about half background


def test_seg_batch_rotates_image_and_label_alike():
    images, labels = seg_stores(24)
    x, target = L.seg_batch(images, labels, [2, 3], [90.0, 90.0], [0, 0], crop=16, **SEG_KW)
    px, pt = L.seg_batch(images, labels, [2, 3], crop=16, **SEG_KW)
    assert torch.equal(x, torch.rot90(px, 1, (2, 3))) and torch.equal(target, torch.rot90(pt, 1, (2, 3)))
    x, target = L.seg_batch(images, labels, [2], [15.0], [1], crop=16, **SEG_KW)
    assert set(target.unique().tolist()) <= {0.0, 1.0}
    assert float(x[0, 0, 0, 0]) == float((torch.tensor(0.0) - SEG_KW["mean"]) / SEG_KW["std"])    # a corner: filled, then normalised


def test_mnist_cls_batch_is_mnist_pairs_and_the_labels():
    store = (rng.bits64(7 * 28 * 28, 77, 1) >> np.uint64(56)).astype(np.uint8).reshape(7, 28, 28)
    labels = np.array([3, 9, 0, 7, 3, 5, 1])
    idx = [3, 0, 6, 3, 5]
    x, label = L.mnist_cls_batch(store, labels, idx)
    assert torch.equal(x, evalio.mnist_pairs(store[idx])[0])
    assert label.dtype == torch.int64 and label.tolist() == [7, 3, 1, 7, 5]


def test_lesion_slices_on_a_hand_made_stack():
    stack = np.zeros((5, 4, 4), dtype=np.int16)
    stack[1] = 3                                           # full: one value throughout
    stack[2, 1, 2] = 1                                     # mixed
    stack[4, :2] = 2                                       # mixed, no 1 in it
    got = evalio.lesion_slices(stack)
    assert got.dtype == np.int64 and got.tolist() == [2, 4]
    assert got.tolist() == [i for i in range(5) if len(np.unique(stack[i])) > 1]          # data.py:695-698
    assert evalio.lesion_slices(torch.from_numpy(stack)).tolist() == [2, 4]
    assert evalio.lesion_slices(np.zeros((3, 2, 2), dtype=bool)).tolist() == []
    with pytest.raises(ValueError):
        evalio.lesion_slices(np.zeros((4, 4)))


def test_the_c_abi_declares_binds_and_exports_both_entry_points():
    src = open(os.path.join(ROOT, "include", "localdiff_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = cabi.lib()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/localdiff_hip.h"
        assert name in cabi.EXPORTS, f"{name} is not bound in _cabi.py"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    # refused before anything is launched: no GPU is needed to be told so
    assert lib.ld_ds_seg_batch(None, None, 1, 8, 8, None, 1, 0.0, 1.0, None, None, None) == -1
    assert b"ld_ds_seg_batch" in lib.ld_last_error()
    assert lib.ld_ds_mnist_cls_batch(None, None, 1, 8, None, 1, None, None, None) == -1
    assert b"ld_ds_mnist_cls_batch" in lib.ld_last_error()


def test_enough_screened_angles_at_every_size_the_gpu_tests_use():
    kept = {S: len(D.screened_angles(S, S)) for S in GPU_TEST_SIZES}
    assert kept == {16: 20, 20: 20, 28: 19, 32: 19, 36: 18}, kept
    assert min(kept.values()) >= 16
