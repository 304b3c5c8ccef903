"""CPU-side checks of the trainable Downsample, Upsample and Conv2d (no GPU needed): the public surface, the reference's
state_dict names and shapes, the constructors' limits, the C ABI's declarations, bindings and refusals, and the torch
restatements the GPU tests compare the layout kernels with.  (The Downsample weight packing's round trip runs on the pack
kernels, which need a GPU: it is in test_hip_resample_grad.py.)"""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import weights

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ld_dn_space_to_depth", "ld_dn_depth_to_space", "ld_dn_upsample2x", "ld_dn_upsample2x_backward", "ld_dn_im2col",
               "ld_dn_head_forward", "ld_dn_head_splits", "ld_dn_head_work_bytes", "ld_dn_head_backward"]


def build(kind, cin, cout):
    if kind == "down":
        return ldh.Downsample(cin, cout)
    if kind == "up":
        return ldh.Upsample(cin, cout)
    k = {"conv3": 3, "stem": 7, "head": 1}[kind]
    return ldh.Conv2d(cin, cout, k, padding=k // 2)


def test_public_surface():
    for name in ("Downsample", "Upsample", "Conv2d"):
        assert name in ldh.__all__
        assert getattr(ldh, name).__module__.endswith(".resample")
        assert issubclass(getattr(ldh, name), ldh.ResnetBlock.__mro__[1])          # a TrainableModule


@pytest.mark.parametrize("prefix", list(R.IN_UNET))
def test_state_dict_names_and_shapes_are_the_unets(prefix):
    """The layer's state_dict is the reference Unet's under its prefix, for the five layers of a cfg3-like config."""
    kind, cin, cout = R.IN_UNET[prefix]
    full = weights.unet_param_shapes(R.CFG)
    want = {k[len(prefix) + 1:]: v for k, v in full.items() if k.startswith(prefix + ".")}
    assert want and dict(R.key_shapes(kind, cin, cout)) == want
    mod = build(kind, cin, cout)
    got = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    assert list(got) == list(want) and got == want
    mod.load_state_dict(R.make_layer(kind, cin, cout))                           # a slice of a checkpoint loads by name


def test_dim_out_defaults_to_dim():
    assert tuple(ldh.Downsample(32).state_dict()["1.weight"].shape) == (32, 128, 1, 1)
    assert tuple(ldh.Upsample(64).state_dict()["1.weight"].shape) == (64, 64, 3, 3)


@pytest.mark.parametrize("make", [lambda: ldh.Downsample(48, 64), lambda: ldh.Downsample(64, 48), lambda: ldh.Upsample(48, 64),
                                  lambda: ldh.Upsample(64, 16), lambda: ldh.Conv2d(48, 64, 3, padding=1),
                                  lambda: ldh.Conv2d(64, 48, 3, padding=1), lambda: ldh.Conv2d(3, 48, 7, padding=3),
                                  lambda: ldh.Conv2d(48, 1, 1)])
def test_constructors_refuse_channel_counts_that_are_no_multiple_of_32(make):
    with pytest.raises(ValueError, match="32"):
        make()


@pytest.mark.parametrize("args,kw", [((32, 32, 5), dict(padding=2)), ((32, 16, 1), {}), ((5, 32, 7), dict(padding=3)),
                                     ((32, 32, 3), {}), ((32, 32, 3), dict(padding=2)), ((3, 32, 7), dict(padding=1)),
                                     ((32, 1, 1), dict(padding=1)), ((0, 32, 7), dict(padding=3)), ((32, 0, 1), {}),
                                     ((32, 9, 1), {})])
def test_conv2d_refuses_what_is_not_one_of_the_three_uses(args, kw):
    """A 5x5 kernel, out_channels 16 at kernel_size 1, the stem with 5 input channels, a padding that is not the use's: the
    message names the three uses."""
    with pytest.raises(ValueError) as e:
        ldh.Conv2d(*args, **kw)
    msg = str(e.value)
    assert "init_conv" in msg and "final_conv" in msg and "downs.-1.3" in msg


def test_modules_refuse_without_touching_a_gpu():
    for mod, c in ((ldh.Downsample(32, 64), 32), (ldh.Upsample(32, 64), 32), (ldh.Conv2d(32, 32, 3, padding=1), 32),
                   (ldh.Conv2d(3, 32, 7, padding=3), 3), (ldh.Conv2d(32, 3, 1), 32)):
        name = type(mod).__name__
        with pytest.raises(ValueError, match=name + ".*CPU"):
            mod(torch.zeros(1, c, 4, 4))
        with pytest.raises(ValueError, match=name + ".*float32"):
            mod(torch.zeros(1, c, 4, 4, dtype=torch.float16))
        with pytest.raises(ValueError, match=name):
            mod(torch.zeros(1, c + 1, 4, 4))
    with pytest.raises(ValueError, match="even"):
        ldh.Downsample(32)(torch.zeros(1, 32, 5, 4))
    with pytest.raises(ValueError, match="even"):
        ldh.Downsample(32)(torch.zeros(1, 32, 4, 6)[..., :5])
    with pytest.raises(ValueError, match="no input gradient"):
        ldh.Conv2d(1, 32, 7, padding=3)(torch.zeros(1, 1, 4, 4, requires_grad=True))


def test_header_declares_and_cabi_binds_the_new_symbols():
    src = open(os.path.join(ROOT, "include", "localdiff_hip.h")).read()
    assert "fourth slice" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = cabi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in the header"
        assert name in cabi.EXPORTS and hasattr(lib, name)
    build_sh = open(os.path.join(ROOT, "localdiffusion-hallucination_amd", "csrc", "build.sh")).read()
    assert "resample_grad" in build_sh


def test_argument_validation_needs_no_gpu():
    """Every new entry point returns -1 with a message for null pointers, misaligned pointers and bad sizes, before anything
    is launched (the pointers are host memory: a launch would fault)."""
    lib = cabi.lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    p += -p % 16
    err = lib.ld_last_error
    for fn in (lib.ld_dn_space_to_depth, lib.ld_dn_depth_to_space, lib.ld_dn_upsample2x, lib.ld_dn_upsample2x_backward):
        assert fn(None, p, 1, 4, 4, 32, 64, None) == -1 and b"null" in err()
        assert fn(p, None, 1, 4, 4, 32, 64, None) == -1 and b"null" in err()
        assert fn(p + 4, p, 1, 4, 4, 32, 64, None) == -1 and b"aligned" in err()
        assert fn(p, p + 8, 1, 4, 4, 32, 64, None) == -1 and b"aligned" in err()
        for shape in ((0, 4, 4, 32, 64), (1, 0, 4, 32, 64), (1, 4, -1, 32, 64), (1, 4, 4, 0, 64), (1, 4, 4, 30, 64),
                      (1, 4, 4, 64, 32), (1, 4, 4, 32, 62)):
            assert fn(p, p, *shape, None) == -1 and b"ldc" in err(), shape
    assert lib.ld_dn_im2col(None, p, 1, 1, 4, 4, 16, 16, 4, 1, 64, None) == -1 and b"null" in err()
    assert lib.ld_dn_im2col(p, None, 1, 1, 4, 4, 16, 16, 4, 1, 64, None) == -1 and b"null" in err()
    assert lib.ld_dn_im2col(p, p + 4, 1, 1, 4, 4, 16, 16, 4, 1, 64, None) == -1 and b"aligned" in err()
    assert lib.ld_dn_im2col(p, p, 1, 5, 4, 4, 80, 16, 4, 1, 256, None) == -1 and b"Cin" in err()
    assert lib.ld_dn_im2col(p, p, 1, 0, 4, 4, 16, 16, 4, 1, 64, None) == -1
    assert lib.ld_dn_im2col(p, p, 1, 2, 4, 4, 32, 16, 4, 1, 64, None) == -1                  # ldk < 98
    assert lib.ld_dn_im2col(p, p, 1, 1, 4, 4, 16, 16, 4, 1, 50, None) == -1                  # ldk no multiple of 4
    assert lib.ld_dn_im2col(p, p, 1, 1, 4, 4, 16, 16, -4, 1, 64, None) == -1 and b"stride" in err()
    assert lib.ld_dn_im2col(p, p, 0, 1, 4, 4, 16, 16, 4, 1, 64, None) == -1
    assert lib.ld_dn_head_forward(p, p, p, None, 1, 4, 4, 32, 64, 1, None) == -1 and b"null" in err()
    assert lib.ld_dn_head_forward(None, p, p, p, 1, 4, 4, 32, 64, 1, None) == -1 and b"null" in err()
    assert lib.ld_dn_head_forward(p + 4, p, p, p, 1, 4, 4, 32, 64, 1, None) == -1 and b"aligned" in err()
    for shape in ((1, 4, 4, 32, 64, 0), (1, 4, 4, 32, 64, 9), (1, 4, 4, 48, 64, 1), (1, 4, 4, 64, 32, 1), (1, 4, 4, 32, 48, 1),
                  (0, 4, 4, 32, 64, 1), (1, 4, 0, 32, 64, 1)):
        assert lib.ld_dn_head_forward(p, p, p, p, *shape, None) == -1 and b"O=" in err(), shape
        assert lib.ld_dn_head_backward(p, p, p, p, p, p, p, *shape, None) == -1 and b"O=" in err(), shape
    assert lib.ld_dn_head_backward(p, p, p, None, p, p, p, 1, 4, 4, 32, 64, 1, None) == -1 and b"null" in err()
    assert lib.ld_dn_head_backward(p, p, p, p, p, p, None, 1, 4, 4, 32, 64, 1, None) == -1 and b"null" in err()
    assert lib.ld_dn_head_backward(p, p, p, p, p, p, p + 4, 1, 4, 4, 32, 64, 1, None) == -1 and b"aligned" in err()
    assert lib.ld_dn_head_backward(p, p, p, p + 4, p, p, p, 1, 4, 4, 32, 64, 1, None) == -1 and b"aligned" in err()
    big = 1 << 20
    for fn in (lib.ld_dn_space_to_depth, lib.ld_dn_depth_to_space, lib.ld_dn_upsample2x, lib.ld_dn_upsample2x_backward):
        assert fn(p, p, 1 << 30, big, big, 1 << 20, 1 << 20, None) == -1 and b"ldc" in err()  # B H W C would leave int64
        assert fn(p, p, 1, big, big, 32, 64, None) == -1                                      # 2^40 pixels
        assert fn(p, p, 1, 4, 4, 32, (1 << 16) + 64, None) == -1
    assert lib.ld_dn_im2col(p, p, 1 << 30, 1, big, big, 16, 16, 4, 1, 64, None) == -1
    assert lib.ld_dn_head_forward(p, p, p, p, 1 << 30, big, big, 32, 64, 1, None) == -1
    assert lib.ld_dn_head_forward(p, p, p, p, 1, 4, 4, 2048 + 32, 2048 + 64, 1, None) == -1 and b"2048" in err()
    assert lib.ld_dn_head_backward(p, p, p, p, p, p, p, 1 << 30, big, big, 32, 64, 1, None) == -1
    assert all(v == 0.0 for v in buf)                                                        # nothing was written


def test_head_split_and_work_size():
    """The split depends on the pixel count alone: one part up to 32 pixels, at most 512 parts of a multiple of 32 pixels."""
    lib = cabi.lib()
    assert lib.ld_dn_head_splits(2, 5, 3) == 1 and lib.ld_dn_head_splits(1, 14, 14) == 7 and lib.ld_dn_head_splits(1, 33, 31) == 32
    assert lib.ld_dn_head_splits(8, 256, 256) == 512 and lib.ld_dn_head_splits(3, 100, 100) == 469    # 64 pixels a part
    assert lib.ld_dn_head_splits(0, 4, 4) == 0
    assert int(lib.ld_dn_head_work_bytes(1, 33, 31, 96, 6)) == 32 * 6 * 97 * 8
    assert int(lib.ld_dn_head_work_bytes(1, 33, 31, 96, 9)) == 0 and int(lib.ld_dn_head_work_bytes(1, 33, 31, 48, 1)) == 0


def test_the_torch_restatements_of_the_layout_kernels():
    """A check of the yardstick, not of the feature (it runs tests/resample_ref.py alone and passes without the new modules):
    what the GPU tests compare the layout kernels with is the reference's own arithmetic: (p1 p2 c) is a column
    permutation of the reference's (c p1 p2), depth_to_space inverts space_to_depth, the window sum is autograd's gradient of
    the nearest upsampling, and the 1x1 convolution over im2col's columns with the OIHW weight as it lies in memory is the
    7x7 convolution."""
    x = R.uniform((2, 8, 6, 10), 1)
    s = R.space_to_depth(x)
    ref = x.reshape(2, 8, 3, 2, 5, 2).permute(0, 1, 3, 5, 2, 4).reshape(2, 32, 3, 5)                  # ddpm.py:121
    assert torch.equal(s.reshape(2, 3, 5, 4, 8).permute(0, 4, 3, 1, 2).reshape(2, 32, 3, 5), ref)
    assert torch.equal(R.depth_to_space(s, 8), x)
    g = R.uniform((2, 8, 6, 10), 2).double().requires_grad_(True)
    up = R.upsample2x(g)
    (dg,) = torch.autograd.grad(up, [g], grad_outputs=torch.ones_like(up) * R.uniform(tuple(up.shape), 3).double())
    assert R.rel_err(R.window_sum(R.uniform(tuple(up.shape), 3).double()), dg) < 1e-15
    img, w = R.uniform((2, 3, 9, 11), 4).double(), R.uniform((32, 3, 7, 7), 5).double()
    cols = R.im2col(img, 192)
    assert bool((cols[..., 147:] == 0).all())
    out = (cols[..., :147] @ w.reshape(32, 147).t()).permute(0, 3, 1, 2)
    assert R.rel_err(out, F.conv2d(img, w, padding=3)) < 1e-14
