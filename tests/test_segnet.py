"""CPU-side checks of the segmentation U-Net (the OOD-mask producer in front of sample()): a functional restatement of
the reference forward (unet_model.py:140-243) pinned to golden G18, the state_dict inventory, checkpoint loading, the
test.py preprocessing constant and the C-ABI's argument validation."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import checkpoint, evalio, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def g18():
    return np.load(os.path.join(GOLD, "g18_segunet.npz"))


def g18_state_dict():
    """The weights G18 was made with: procedural tensors + the calibrated running statistics / head bias it stores."""
    g = g18()
    names = weights.seg_param_shapes()
    calib = {k: g[k] for k in g.files if k in names}
    return {k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_seg_state_dict(int(g["seed"]), calib).items()}


def restated_forward(sd, x):
    """unet_model.UNet(bilinear=False).forward in eval mode, op by op."""
    def dconv(p, h):
        for i in (0, 3):
            h = F.conv2d(h, sd[f"{p}double_conv.{i}.weight"], padding=1)
            bn = f"{p}double_conv.{i + 1}."
            h = F.batch_norm(h, sd[bn + "running_mean"], sd[bn + "running_var"], sd[bn + "weight"], sd[bn + "bias"],
                             training=False, eps=1e-5)
            h = F.relu(h)
        return h
    skips = [dconv("inc.", x)]
    for i in range(1, 5):
        skips.append(dconv(f"down{i}.maxpool_conv.1.", F.max_pool2d(skips[-1], 2)))
    h = skips[-1]
    for i in range(1, 5):
        up = F.conv_transpose2d(h, sd[f"up{i}.up.weight"], sd[f"up{i}.up.bias"], stride=2)
        h = dconv(f"up{i}.conv.", torch.cat([skips[4 - i], up], dim=1))
    return F.conv2d(h, sd["outc.conv.weight"], sd["outc.conv.bias"])


def test_restated_forward_matches_reference_golden():
    g, sd = g18(), g18_state_dict()
    with torch.no_grad():
        for x_key, l_key in (("x32", "logits32"), ("x64", "logits64"), ("lr128", "logits128"), ("lr256", "logits256")):
            x = torch.from_numpy(g[x_key])
            if x_key.startswith("lr"):
                x = evalio.seg_preprocess(x, float(g["mean_t1"]), float(g["std_t1"]))
            ref = torch.from_numpy(g[l_key])
            got = restated_forward(sd, x)
            assert got.shape == ref.shape
            err = float((got - ref).abs().max()) / float(ref.abs().max())
            assert err < 1e-5, (x_key, err)
    for H in (128, 256):                       # the stored masks are test.py's sigmoid > 0.5 of the stored logits
        assert np.array_equal(g[f"mask{H}"], (torch.sigmoid(torch.from_numpy(g[f"logits{H}"])) > 0.5).float().numpy())
    lg = g["logits128"]                        # the end-to-end slice has both classes and no pixel near the threshold
    assert 0.02 < g["mask128"].mean() < 0.98 and np.abs(lg).min() > 1e-4 * np.abs(lg).max()


def test_state_dict_matches_reference_inventory():
    inv = [ln.split(" ", 1) for ln in open(os.path.join(GOLD, "g18_segunet_inventory.txt")).read().splitlines()]
    sd = ldh.SegUNet().state_dict()
    assert len(inv) == 118 and list(sd.keys()) == [n for n, _ in inv]
    for name, rest in inv:
        shape, dtype = rest.rsplit(" ", 1)
        assert str(list(sd[name].shape)) == shape and str(sd[name].dtype).replace("torch.", "") == dtype, name
    shapes = weights.seg_param_shapes()
    assert list(shapes) == list(sd) and all(tuple(sd[k].shape) == v for k, v in shapes.items())
    n_params = sum(p.numel() for p in ldh.SegUNet().parameters())
    assert round(n_params / 1e6, 1) == 31.0


def test_unsupported_configurations_say_what_is_missing():
    with pytest.raises(ValueError, match="bilinear"):
        ldh.SegUNet(bilinear=True)
    with pytest.raises(ValueError, match="n_classes"):
        ldh.SegUNet(n_classes=2)
    with pytest.raises(ValueError, match="n_channels"):
        ldh.SegUNet(n_channels=2)
    with pytest.raises(ValueError, match="compute_dtype"):
        ldh.SegUNet(compute_dtype="fp8")
    net = ldh.SegUNet().eval()
    with pytest.raises(ValueError, match="multiples of 16"):
        net(torch.zeros(1, 1, 40, 48))
    with pytest.raises(ValueError, match=r"\[B, 1, H, W\]"):
        net(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="eval"):
        ldh.SegUNet()(torch.zeros(1, 1, 32, 32))


def test_load_seg_checkpoint_reference_format(tmp_path):
    sd = g18_state_dict()                      # bare state_dict as train_seg.py saves it (num_batches_tracked included)
    assert sd["inc.double_conv.1.num_batches_tracked"].dtype == torch.int64
    path = str(tmp_path / "t1seg.pth")
    torch.save(sd, path)
    net = ldh.SegUNet()
    info = checkpoint.load_seg_checkpoint(path, net)
    assert info["n_tensors"] == 118
    own = net.state_dict()
    for k, v in sd.items():
        assert torch.equal(own[k], v), k
    bad = dict(sd)
    del bad["up2.up.bias"]
    with pytest.raises(RuntimeError, match="missing"):
        checkpoint.load_seg_checkpoint(bad, ldh.SegUNet())
    bad = dict(sd, extra=torch.zeros(1))
    with pytest.raises(RuntimeError, match="unexpected"):
        checkpoint.load_seg_checkpoint(bad, ldh.SegUNet())
    bad = dict(sd)
    bad["outc.conv.weight"] = torch.zeros(2, 64, 1, 1)
    with pytest.raises(RuntimeError, match="wrong shape"):
        checkpoint.load_seg_checkpoint(bad, ldh.SegUNet())


def test_seg_preprocessing_constant_from_config():
    mean_t1, std_t1 = 610.7180906353575, 1018.7631901605115          # config.yaml:55-56
    lr = torch.linspace(0.0, 3.0, 16).reshape(1, 1, 4, 4)
    got = evalio.seg_preprocess(lr, mean_t1, std_t1)
    ref = lr - torch.abs(torch.tensor((0 - mean_t1) / std_t1))       # test.py:215-216
    assert torch.equal(got, ref)
    assert abs(float(lr[0, 0, 0, 0] - got[0, 0, 0, 0]) - 610.7180906353575 / 1018.7631901605115) < 1e-7
    with pytest.raises(NameError, match="mini"):
        evalio.seg_preprocess(lr, mean_t1, std_t1, translate_zero=False)
    with pytest.raises(NameError, match="translate_zero"):
        evalio.seg_ood_mask(None, lr, mean_t1, std_t1, translate_zero=False)


def test_seg_argument_validation_needs_no_gpu():
    lib = cabi.lib()
    a = cabi.SegConvArgs()
    a.src0 = a.src1 = a.weight = a.out = 16
    a.C0, a.C1, a.mode, a.ksize, a.B, a.H, a.W, a.Cout, a.dtype = 64, 64, cabi.SEG_SRC_CAT_D2S, 3, 1, 16, 16, 64, 0
    a.H = 15                                                             # odd H with a depth-to-space source
    assert lib.ld_seg_conv(C.byref(a), None) == -1 and b"even" in lib.ld_last_error()
    a.H, a.Cout = 16, 48                                                 # Cout not a multiple of 32 (the kernel tiles 64)
    assert lib.ld_seg_conv(C.byref(a), None) == -1 and b"Cout" in lib.ld_last_error()
    a.Cout, a.C0 = 64, 40                                                # an input channel count the tiles cannot take
    assert lib.ld_seg_conv(C.byref(a), None) == -1 and b"C0" in lib.ld_last_error()
    a.C0, a.mode, a.ksize = 64, cabi.SEG_SRC_POOL, 1
    assert lib.ld_seg_conv(C.byref(a), None) == -1 and b"ksize" in lib.ld_last_error()
    a.ksize, a.dtype = 3, 5
    assert lib.ld_seg_conv(C.byref(a), None) == -1 and b"dtype" in lib.ld_last_error()
    assert lib.ld_seg_conv_image(16, 16, 16, 16, 16, 1, 2, 16, 16, 0, None) == -1 and b"Cin" in lib.ld_last_error()
    assert lib.ld_seg_head(16, 16, 16, 16, None, None, 1, 16, 16, 62, 0, None) == -1
    assert lib.ld_seg_head(16, 16, 16, None, None, None, 1, 16, 16, 64, 0, None) == -1


def test_seg_entry_points_are_exported():
    lib = cabi.lib()
    for n in ("ld_seg_conv", "ld_seg_conv_image", "ld_seg_head", "ld_seg_pack_weight", "ld_seg_pack_convt"):
        assert n in cabi.EXPORTS and hasattr(lib, n), n
