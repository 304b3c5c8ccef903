"""Pure-torch CPU restatements of the three ``__getitem__``s that ``DeviceDataset`` replaces (the reference's data.py), and of
the augmentation in front of them.  Nothing here reads the reference tree or touches a GPU.

The rotation is torchvision's tensor ``rotate`` (``NEAREST``, ``expand=False``, ``fill=None``: ``F.rotate`` ->
``_get_inverse_affine_matrix(center 0, -angle)`` = [cos a, -sin a, 0, sin a, cos a, 0] -> ``_gen_affine_grid`` ->
``grid_sample(mode="nearest", padding_mode="zeros", align_corners=False)``), restated from its source because the package is not
installed where this was written -- so it has not been run against the package.  It is here in two forms:

* ``rotate_grid``: ``_gen_affine_grid``'s arithmetic (fp32 linspace base grid, bmm with theta / (W / 2, H / 2)) into
  ``F.grid_sample``;
* ``rotate_direct``: for output pixel (i, j), xo = j - (W-1)/2, yo = i - (H-1)/2, sx = cos a xo - sin a yo + (W-1)/2,
  sy = sin a xo + cos a yo + (H-1)/2 in fp64, the source pixel (round(sy), round(sx)) half to even, 0 outside.

Both, and the kernel (the same formula in fp32), pick the same source pixel wherever no coordinate comes close to a
half-integer: ``tie_margin`` measures how close, ``screened_angles`` keeps the candidates with a margin above 1e-4 -- about
100 x the fp32 error of a coordinate at these sizes (|coordinate| < 32: half an ulp is 1.9e-6, four roundings) -- so on the
screened angles every comparison can be exact.  cos a and sin a are the fp32 roundings of libm's doubles everywhere, as in a
table row.  A positive angle is counter-clockwise: +90 degrees is ``torch.rot90(x, 1, (2, 3))``.  ``RandomVerticalFlip`` comes
after the rotation and reverses the rows.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

# fixed candidates: 0, the ends of RandomRotation(15)'s interval, small angles, negative angles
CANDIDATE_ANGLES = (0.0, 15.0, -15.0, 0.5, -0.5, 1.0, -1.0, 2.5, -3.7, 5.0,
                    -6.3, 7.77, -8.1, 9.9, -10.25, 11.3, 12.6, -13.4, 14.2, -14.9)
MARGIN = 1e-4


def cos_sin(angle_deg):
    a = math.radians(float(angle_deg))
    return float(np.float32(math.cos(a))), float(np.float32(math.sin(a)))


def _source_coords(angle_deg, H, W):
    c, s = cos_sin(angle_deg)
    i = torch.arange(H, dtype=torch.float64)[:, None]
    j = torch.arange(W, dtype=torch.float64)[None, :]
    xo, yo = j - (W - 1) / 2, i - (H - 1) / 2
    return c * xo - s * yo + (W - 1) / 2, s * xo + c * yo + (H - 1) / 2


def tie_margin(angle_deg, H, W):
    """The smallest distance, in fp64, of any output pixel's sx or sy from a half-integer."""
    sx, sy = _source_coords(angle_deg, H, W)
    both = torch.cat([sx.reshape(-1), sy.reshape(-1)])
    return float(((both - torch.floor(both)) - 0.5).abs().min())


def screened_angles(H, W):
    return [a for a in CANDIDATE_ANGLES if tie_margin(a, H, W) > MARGIN]


def rotate_direct(x, angle_deg):
    """x [..., H, W] -> the rotated image, the direct fp64 form."""
    H, W = x.shape[-2:]
    sx, sy = _source_coords(angle_deg, H, W)
    rx, ry = torch.round(sx).long(), torch.round(sy).long()               # (torch.round: half to even)
    inside = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    got = x[..., ry.clamp(0, H - 1), rx.clamp(0, W - 1)]
    return torch.where(inside, got, torch.zeros((), dtype=x.dtype))


def rotate_grid(x, angle_deg):
    """x [N, C, H, W] fp32 -> the rotated image, torchvision's ``_gen_affine_grid`` + ``grid_sample`` form."""
    N, _, H, W = x.shape
    c, s = cos_sin(angle_deg)
    theta = torch.tensor([c, -s, 0.0, s, c, 0.0], dtype=torch.float32).reshape(1, 2, 3)
    d = 0.5
    base = torch.empty(1, H, W, 3, dtype=torch.float32)
    base[..., 0].copy_(torch.linspace(-W * 0.5 + d, W * 0.5 + d - 1, steps=W))
    base[..., 1].copy_(torch.linspace(-H * 0.5 + d, H * 0.5 + d - 1, steps=H).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float32)
    grid = base.view(1, H * W, 3).bmm(rescaled).view(1, H, W, 2)
    return F.grid_sample(x, grid.expand(N, H, W, 2), mode="nearest", padding_mode="zeros", align_corners=False)


def augment(x, angle_deg=None, flip=False, form="direct"):
    """``Compose([RandomRotation, RandomVerticalFlip])`` with the drawn parameters given: x [N, C, H, W] fp32."""
    if angle_deg is not None:
        x = rotate_direct(x, angle_deg) if form == "direct" else rotate_grid(x, angle_deg)
    return torch.flip(x, dims=(-2,)) if flip else x


def mnist_item(img_u8, angle_deg=None, flip=False, form="direct"):
    """``MNIST.__getitem__`` (data.py:814-836): u8 [S, S] -> (hr, lr) fp32 [1, S, S]."""
    img = torch.tensor(np.asarray(img_u8)).float().unsqueeze(0)          # np2tensor (data.py:797-799)
    img = augment(img[None], angle_deg, flip, form)[0]                    # transform (data.py:779-795)
    img = img.unsqueeze(0)                                                # data.py:822-823
    down = img[:, ::2, ::2]                                               # data.py:825: dims 0, 1, 2 -- the ROWS only
    down = F.interpolate(down, size=(img.shape[-1], img.shape[-1]), mode="bilinear", align_corners=False)
    down, img = 2 * (down / 255.0), 2 * (img / 255.0)                     # normalize (data.py:808-809, 828-829)
    return img.squeeze(0), down.squeeze(0)


def sr_item(img_u8, angle_deg=None, flip=False, form="direct"):
    """``MvtecDatasetSR.__getitem__`` (data.py:287-307; train, no denoise, no mask_train) behind its PIL resize: u8 [C, S, S]
    -> (hr, lr) fp32 [C, S, S].  ``ToTensor`` is u8 / 255; angle and flip are the extension (the reference does not augment)."""
    img = torch.tensor(np.asarray(img_u8)).float().div(255)               # ToTensor (data.py:280-284)
    img = augment(img[None], angle_deg, flip, form)[0]
    img = img * 2                                                         # data.py:297
    size = img.shape[-1] // 2
    down = F.interpolate(img.unsqueeze(0), size=(size, size), mode="nearest")                 # data.py:299-300
    down = F.interpolate(down, size=(img.shape[-1], img.shape[-1]), mode="bilinear", align_corners=False)
    return img, down.squeeze(0)


def crop_offset(size, crop):
    return int(round((size - crop) / 2.0))                                # torchvision's center_crop


def mri_item(target, cond, *, mean_target, std_target, mean_cond, std_cond, translate_zero=True, crop=224, angle_deg=None,
             flip=False, form="direct"):
    """``MedDataset_png.__getitem__`` (data.py:420-442) behind the PNG decode: fp32 [R, R] x 2 -> (target', cond') [1, crop,
    crop].  ``transform`` (data.py:369-398): CenterCrop, then the SAME rotation and flip for both (the reference reseeds the
    generator in front of each); ``normalize`` (data.py:400-410): (x - mean) / std, then + |min| of that image."""
    out = []
    top = crop_offset(target.shape[-1], crop)
    for x, mean, std in ((target, mean_target, std_target), (cond, mean_cond, std_cond)):
        x = torch.as_tensor(x, dtype=torch.float32).unsqueeze(0)          # np2tensor (data.py:412-415)
        x = x[:, top:top + crop, top:top + crop]
        x = augment(x[None], angle_deg, flip, form)[0]
        x = (x - mean) / std
        if translate_zero:
            x = x + torch.abs(x.min())
        out.append(x)
    return tuple(out)


def _stack(items):
    return torch.stack([a for a, _ in items]), torch.stack([b for _, b in items])


def _params(n, angles_deg, flips):
    return ([None] * n if angles_deg is None else list(angles_deg)), ([False] * n if flips is None else list(flips))


def mnist_batch(store, indices, angles_deg=None, flips=None, form="direct"):
    ang, fl = _params(len(indices), angles_deg, flips)
    return _stack([mnist_item(store[i], a, bool(f), form) for i, a, f in zip(indices, ang, fl)])


def sr_batch(store, indices, angles_deg=None, flips=None, form="direct"):
    ang, fl = _params(len(indices), angles_deg, flips)
    return _stack([sr_item(store[i], a, bool(f), form) for i, a, f in zip(indices, ang, fl)])


def mri_batch(target, cond, indices, angles_deg=None, flips=None, form="direct", **kw):
    ang, fl = _params(len(indices), angles_deg, flips)
    return _stack([mri_item(target[i], cond[i], angle_deg=a, flip=bool(f), form=form, **kw) for i, a, f in zip(indices, ang, fl)])
