"""The segmentation U-Net (OOD-mask producer) on the GPU: every kernel mode against torch fp32 ops at every level of the
net, the whole net against the reference's logits (golden G18), and the mask path end to end (seg_ood_mask -> sample ->
tools/run_seg_eval.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import localdiffusion_hallucination_amd as ldh                              # noqa: E402
from localdiffusion_hallucination_amd import _cabi as cabi                  # noqa: E402
from localdiffusion_hallucination_amd import evalio, rng, weights           # noqa: E402

from hip_helpers import DEV, RTOL, TDT, nchw, nhwc, rel_err, st             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DTYPES = ["fp32", "bf16", "fp16"]
# whole-net logits, max-abs error / max |logit| of G18.  16-bit storage: about twice the worst of the four G18 inputs on
# the first MI355X measurement (bf16 2.3e-2, fp16 2.4e-3; fp32 measured 4.5e-6)
NET_TOL = {"fp32": 1e-4, "bf16": 5e-2, "fp16": 5e-3}


def rnd(shape, key, lo=-1.0, hi=1.0):
    return torch.from_numpy(rng.uniform(shape, 1818, key, lo, hi))


def stored(x, dtype):
    """NCHW fp32 -> the values a tensor of that storage type holds (fp32 NCHW, cpu)."""
    return x.to(TDT[dtype]).float()


def bn_params(c, key):
    gamma, beta = 1.0 + 0.1 * rnd((c,), key), 0.1 * rnd((c,), key + 1)
    mean, var = 0.2 * rnd((c,), key + 2), 0.5 + rnd((c,), key + 3, 0.0, 1.0)
    s = gamma / torch.sqrt(var + 1e-5)
    return (gamma, beta, mean, var), s, beta - mean * s


def ref_conv_bn_relu(x, w, bn):
    gamma, beta, mean, var = bn
    return F.relu(F.batch_norm(F.conv2d(x, w, padding=1), mean, var, gamma, beta, training=False, eps=1e-5))


def pack3(w):
    w = w.to(DEV).contiguous()
    out = torch.empty(w.numel(), dtype=torch.float32, device=DEV)
    cabi.check(cabi.lib().ld_seg_pack_weight(w.data_ptr(), out.data_ptr(), w.shape[0], w.shape[1], 3, st()), "pack")
    return out


def seg_conv(src0, c0, mode, wp, s, t, B, H, W, cout, dtype, src1=None, c1=0, ksize=3, relu=1):
    out = torch.empty((B, H, W, cout), dtype=TDT[dtype], device=DEV)
    a = cabi.SegConvArgs()
    a.src0, a.src1, a.C0, a.C1, a.mode, a.ksize = src0.data_ptr(), cabi.ptr(src1), c0, c1, mode, ksize
    a.weight, a.scale, a.shift, a.relu = wp.data_ptr(), cabi.ptr(s), cabi.ptr(t), relu
    a.out, a.B, a.H, a.W, a.Cout, a.dtype = out.data_ptr(), B, H, W, cout, cabi.dtype_code(dtype)
    cabi.check(cabi.lib().ld_seg_conv(C.byref(a), st()), "seg_conv")
    return out


# (H of the conv's output, Cin, Cout): the DoubleConvs of a 256^2 net, first convolution of each Down read through the pool
LEVELS = [(256, 64, 64), (128, 64, 128), (64, 128, 256), (32, 256, 512), (16, 512, 1024)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,cin,cout", LEVELS)
def test_conv_bn_relu_per_level(dtype, H, cin, cout):
    B = 1
    pool = H < 256                              # Down: 2x2 max-pool of the [2H, 2W, cin] map on load; inc's 2nd conv: plain
    Hs = 2 * H if pool else H
    x = stored(F.relu(rnd((B, cin, Hs, Hs), H)), dtype)
    w = rnd((cout, cin, 3, 3), H + 1) / np.sqrt(cin * 9)
    bn, s, t = bn_params(cout, 10 * H)
    xin = F.max_pool2d(x, 2) if pool else x
    ref = ref_conv_bn_relu(xin, w, bn)
    got = seg_conv(nhwc(x, dtype), cin, cabi.SEG_SRC_POOL if pool else cabi.SEG_SRC_PLAIN, pack3(w), s.to(DEV),
                   t.to(DEV), B, H, H, cout, dtype)
    e = rel_err(nchw(got), ref)
    print(f"conv3x3+BN+ReLU {dtype} {H}^2 {cin}->{cout} pool={pool}: rel err {e:.2e}")
    assert e <= RTOL[dtype], e
    if pool:                                    # second convolution of the same DoubleConv: plain source, Cin = Cout
        w2 = rnd((cout, cout, 3, 3), H + 2) / np.sqrt(cout * 9)
        bn2, s2, t2 = bn_params(cout, 10 * H + 5)
        ref2 = ref_conv_bn_relu(stored(nchw(got), dtype), w2, bn2)
        got2 = seg_conv(got, cout, cabi.SEG_SRC_PLAIN, pack3(w2), s2.to(DEV), t2.to(DEV), B, H, H, cout, dtype)
        assert rel_err(nchw(got2), ref2) <= RTOL[dtype]


# (H of the Up's output, Cin of the ConvTranspose2d): up1..up4 of a 256^2 net; up1 is the 1024-channel concat
UPS = [(32, 1024), (64, 512), (128, 256), (256, 128)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,cin", UPS)
def test_convT_gemm_and_depth_to_space_concat(dtype, H, cin):
    B, cout = 2 if H <= 64 else 1, cin // 2
    low = stored(F.relu(rnd((B, cin, H // 2, H // 2), cin)), dtype)
    skip = stored(F.relu(rnd((B, cout, H, H), cin + 1)), dtype)
    wt, bt = rnd((cin, cout, 2, 2), cin + 2) / np.sqrt(cin), rnd((cout,), cin + 3) / np.sqrt(cin)
    up_ref = F.conv_transpose2d(low, wt, bt, stride=2)
    wtp = torch.empty(cin * 4 * cout, device=DEV)
    btp = torch.empty(4 * cout, device=DEV)
    wtd, btd = wt.to(DEV).contiguous(), bt.to(DEV)
    cabi.check(cabi.lib().ld_seg_pack_convt(wtd.data_ptr(), btd.data_ptr(), wtp.data_ptr(), btp.data_ptr(), cin, cout, st()),
               "pack_convt")
    up = seg_conv(nhwc(low, dtype), cin, cabi.SEG_SRC_PLAIN, wtp, None, btp, B, H // 2, H // 2, 4 * cout, dtype, ksize=1,
                  relu=0)
    # the GEMM output in (p1, p2, c) channel order, rearranged to the ConvTranspose2d's image
    up_img = up.float().reshape(B, H // 2, H // 2, 2, 2, cout).permute(0, 5, 1, 3, 2, 4).reshape(B, cout, H, H).cpu()
    e_up = rel_err(up_img, up_ref)
    assert e_up <= RTOL[dtype], e_up
    w = rnd((cout, cin, 3, 3), cin + 4) / np.sqrt(cin * 9)
    bn, s, t = bn_params(cout, cin + 5)
    ref = ref_conv_bn_relu(torch.cat([skip, stored(up_img, dtype)], dim=1), w, bn)     # unet_model.py:200-201
    got = seg_conv(nhwc(skip, dtype), cout, cabi.SEG_SRC_CAT_D2S, pack3(w), s.to(DEV), t.to(DEV), B, H, H, cout, dtype,
                   src1=up, c1=cout)
    e = rel_err(nchw(got), ref)
    print(f"up {dtype} {H}^2 cat({cout}+{cout}): convT rel err {e_up:.2e}, conv rel err {e:.2e}")
    assert e <= RTOL[dtype], e


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin", [1, 3])
def test_first_conv_64_wide(dtype, cin):
    B, H = 2, 256
    x = rnd((B, cin, H, H), 50 + cin, -1.0, 3.0)
    w = rnd((64, cin, 3, 3), 60 + cin) / np.sqrt(cin * 9)
    bn, s, t = bn_params(64, 70 + cin)
    ref = ref_conv_bn_relu(x, w, bn)
    out = torch.empty((B, H, H, 64), dtype=TDT[dtype], device=DEV)
    xd, wd, sd, td = x.to(DEV).contiguous(), w.to(DEV).contiguous(), s.to(DEV), t.to(DEV)
    cabi.check(cabi.lib().ld_seg_conv_image(xd.data_ptr(), wd.data_ptr(), sd.data_ptr(), td.data_ptr(), out.data_ptr(),
                                            B, cin, H, H, cabi.dtype_code(dtype), st()), "seg_conv_image")
    assert rel_err(nchw(out), ref) <= RTOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_head_logits_sigmoid_mask(dtype):
    B, H = 2, 64
    x = stored(F.relu(rnd((B, 64, H, H), 80)), dtype)
    w, b = rnd((1, 64, 1, 1), 81) / 8.0, torch.tensor([-0.4])
    ref = F.conv2d(x, w, b)
    outs = [torch.empty((B, 1, H, H), device=DEV) for _ in range(3)]
    wd, bd = w.reshape(-1).to(DEV).contiguous(), b.to(DEV)
    xd = nhwc(x, dtype)
    cabi.check(cabi.lib().ld_seg_head(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), *(o.data_ptr() for o in outs),
                                      B, H, H, 64, cabi.dtype_code(dtype), st()), "seg_head")
    logits, prob, mask = (o.cpu() for o in outs)
    assert rel_err(logits, ref) <= 2e-5
    assert torch.allclose(prob, torch.sigmoid(logits), atol=1e-6, rtol=0)
    assert torch.equal(mask, (prob > 0.5).float())
    assert 0 < float(mask.mean()) < 1


def g18_net(dtype):
    g = np.load(os.path.join(GOLD, "g18_segunet.npz"))
    names = weights.seg_param_shapes()
    sd = weights.procedural_seg_state_dict(int(g["seed"]), {k: g[k] for k in g.files if k in names})
    net = ldh.SegUNet(compute_dtype=dtype)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net.to(DEV).eval(), g


def g18_inputs(g):
    for x_key, l_key in (("x32", "logits32"), ("x64", "logits64"), ("lr128", "logits128"), ("lr256", "logits256")):
        x = torch.from_numpy(g[x_key])
        if x_key.startswith("lr"):
            x = evalio.seg_preprocess(x, float(g["mean_t1"]), float(g["std_t1"]))
        yield x_key, x, g[l_key]


@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_net_against_reference_golden(dtype):
    net, g = g18_net(dtype)
    errs = []
    for key, x, ref in g18_inputs(g):
        got, (prob, binary, logits2) = net(x.to(DEV)), net.predict_mask(x.to(DEV), return_logits=True)
        got, logits2, binary = got.cpu().numpy(), logits2.cpu().numpy(), binary.cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got, logits2)
        err = float(np.abs(got - ref).max())
        scale = float(np.abs(ref).max())
        errs.append(err / scale)
        print(f"SegUNet {dtype} {key} {tuple(ref.shape)}: logits max-abs err {err:.3e} = {err / scale:.2e} of max |logit|")
        assert err <= NET_TOL[dtype] * scale, (key, err, scale)
        ref_mask = (ref > 0).astype(np.float32)          # sigmoid(l) > 0.5 <=> l > 0 at these magnitudes
        bound = 1e-4 * scale if dtype == "fp32" else err
        sure = np.abs(ref) > bound
        assert np.array_equal(binary[sure], ref_mask[sure]), (key, int((binary != ref_mask)[sure].sum()))
    print(f"SegUNet {dtype}: worst relative logit error {max(errs):.2e} (bound {NET_TOL[dtype]:.0e})")


def test_plan_cache_invalidation():
    net, g = g18_net("fp32")
    x = torch.from_numpy(g["x64"]).to(DEV)
    a = net(x)
    assert len(net._plans) == 1
    net.set_compute_dtype("bf16")
    assert len(net._plans) == 0
    b = net(x)
    net.set_compute_dtype("fp32")
    sd = net.state_dict()
    sd["outc.conv.bias"] = sd["outc.conv.bias"] + 1.0
    net.load_state_dict(sd)
    assert net._prep is None and not net._plans
    c = net(x)
    assert torch.allclose(c, a + 1.0, atol=1e-5) and not torch.equal(a, b)


def test_seg_ood_mask_and_branched_sampling_end_to_end(tmp_path):
    net, g = g18_net("fp32")
    lr = torch.from_numpy(g["lr128"]).to(DEV)
    mask_pred, binary = evalio.seg_ood_mask(net, lr, float(g["mean_t1"]), float(g["std_t1"]))
    assert mask_pred.shape == (1, 1, 128, 128) and mask_pred.is_cuda
    assert torch.equal(binary.cpu(), torch.from_numpy(g["mask128"])) and torch.equal(mask_pred, binary)
    # cfg2's denoiser and shape, branch + fusion, a short DDIM run: the mask made on the GPU drives the same sample
    unet = ldh.Unet(dim=32, init_dim=32, mode="mri")
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in weights.procedural_state_dict(unet.cfg, 0).items()})
    config = dict(branch_out=True, start_intermediate=True, start_timestep=2, data="mri", mask_x=True, mask_cond=False,
                  ood_AD=True, ood_confidence=False, classifier=False, use_gt=False, use_gt_timestep=100)
    gd = ldh.GaussianDiffusion(config, unet, image_size=128, timesteps=100, beta_schedule="sigmoid", objective="pred_x0",
                               auto_normalize=False, sampling_timesteps=5).to(DEV)
    gd.noise_source = "host"
    outs = []
    for m in (mask_pred, torch.from_numpy(g["mask128"]).to(DEV)):
        out = gd.sample(lr, None, batch_size=1, mask=m, min_max_val=(0.0, 4.0))
        outs.append((torch.stack(out) if isinstance(out, list) else out).cpu())
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
    # the driver: two .npy slices in, the four test.py arrays out
    lr2 = np.concatenate([g["lr128"], g["lr128"][:, :, ::-1].copy()])
    np.save(tmp_path / "lr.npy", lr2)
    np.save(tmp_path / "hr.npy", lr2)
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_seg_eval.py"), "--lr", str(tmp_path / "lr.npy"),
                        "--hr", str(tmp_path / "hr.npy"), "--timesteps", "20", "--ddim", "4", "--out", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for name in ("hr_all", "lr_all", "pred_all", "ad_masks"):
        arr = np.load(out_dir / f"{name}.npy")
        assert arr.shape[0] == 2 and np.isfinite(arr).all(), name
    masks = np.load(out_dir / "ad_masks.npy")
    assert masks.shape == (2, 1, 128, 128) and set(np.unique(masks)) <= {0.0, 1.0}
