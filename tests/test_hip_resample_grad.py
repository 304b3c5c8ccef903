"""GPU tests of the fourth slice of the denoiser's backward pass: the layout, im2col and head kernels of
csrc/resample_grad.hip one by one, then ``Downsample``, ``Upsample`` and ``Conv2d`` as wholes, under torch.autograd, in a
small U under the training loss's gradient and under Adam.

Yardstick: torch.autograd in fp64 on the CPU through oracle.unet_ref.pixel_unshuffle_conv / upsample_conv and F.conv2d
(tests/resample_ref.py).  The pure copies are held to torch.equal against their torch restatement, the 2 x 2 window sum to
torch.equal against the same four terms added in torch in fp32 in the documented order, everything behind a sum over pixels
or channels to max(1e-5, 4 d) of the fp64 value, d = fp32 eager torch's own distance to it (resblock_ref.reduction_bound).
Every buffer handed to a kernel is filled with NaN first, padding included, and padding must come out as zero.  Every test
prints HIP's and torch's distances; the docstrings quote those of one MI355X run (docs/findings.md, 125)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi

from hip_helpers import DEV, NAN, nans, pad64, padded, st, unpadded
import resample_ref as R
import resblock_ref

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def work(nbytes):
    assert int(nbytes) > 0
    return nans(int(nbytes) // 8, dtype=F64)


def pad_is_zero(t, c):
    return t.shape[-1] == c or bool((t[..., c:] == 0).all())


# ------------------------------------------------------------------------------------------------ 1. the layout kernels
# (B, C, ldc, H, W) with H x W the small map: space-to-depth's output, the upsampling's input.  Non-square, so that a swap of
# H and W or of p1 and p2 shows.
S2D_CASES = [(2, 32, 64, 3, 5), (1, 96, 128, 7, 7), (2, 64, 64, 4, 4)]
UP_CASES = [(2, 32, 64, 3, 5), (1, 96, 128, 7, 7), (1, 256, 256, 4, 4)]


@pytest.mark.parametrize("B,Cc,ldc,H,W", S2D_CASES)
def test_space_to_depth_and_back(B, Cc, ldc, H, W):
    """ld_dn_space_to_depth is bit-equal to the torch rearrangement in the (p1 p2 c) order and never reads x's padding (NaN);
    ld_dn_depth_to_space of the result returns x's real channels bit for bit, with zeros in the padding.  MI355X: bit-equal
    in all three cases."""
    lib = cabi.lib()
    x = R.uniform((B, Cc, 2 * H, 2 * W), 100 + Cc + H)
    xp, out = padded(x, ldc), nans(B, H, W, 4 * Cc)
    cabi.check(lib.ld_dn_space_to_depth(xp.data_ptr(), out.data_ptr(), B, H, W, Cc, ldc, st()), "dn_space_to_depth")
    assert torch.equal(out.cpu(), R.space_to_depth(x))
    g = R.uniform((B, H, W, 4 * Cc), 200 + Cc + H)                                # a gradient of its own, too
    for src, want in ((out, x), (g.to(DEV), R.depth_to_space(g, Cc))):
        dx = nans(B, 2 * H, 2 * W, ldc)
        cabi.check(lib.ld_dn_depth_to_space(src.data_ptr(), dx.data_ptr(), B, H, W, Cc, ldc, st()), "dn_depth_to_space")
        assert torch.equal(unpadded(dx, Cc), want) and pad_is_zero(dx, Cc)
    print(f"s2d B{B} C{Cc} ldc{ldc} {H}x{W}: bit-equal to torch, both ways")


@pytest.mark.parametrize("B,Cc,ldc,H,W", UP_CASES)
def test_upsample2x_and_its_backward(B, Cc, ldc, H, W):
    """ld_dn_upsample2x is bit-equal to F.interpolate(nearest, x2); ld_dn_upsample2x_backward to ((g00 + g01) + g10) + g11
    added in torch in fp32.  The inputs' padding holds NaN and is never read; the outputs' is zero.  MI355X: bit-equal in all
    three cases."""
    lib = cabi.lib()
    x, g = R.uniform((B, Cc, H, W), 300 + Cc + H), R.uniform((B, Cc, 2 * H, 2 * W), 400 + Cc + H)
    xp, gp = padded(x, ldc), padded(g, ldc)
    up, dx = nans(B, 2 * H, 2 * W, ldc), nans(B, H, W, ldc)
    cabi.check(lib.ld_dn_upsample2x(xp.data_ptr(), up.data_ptr(), B, H, W, Cc, ldc, st()), "dn_upsample2x")
    cabi.check(lib.ld_dn_upsample2x_backward(gp.data_ptr(), dx.data_ptr(), B, H, W, Cc, ldc, st()), "dn_upsample2x_backward")
    assert torch.equal(unpadded(up, Cc), R.upsample2x(x)) and pad_is_zero(up, Cc)
    assert torch.equal(unpadded(dx, Cc), R.window_sum(g)) and pad_is_zero(dx, Cc)
    print(f"upsample B{B} C{Cc} ldc{ldc} {H}x{W}: bit-equal to torch, forward and window sum")


@pytest.mark.parametrize("B,cin,H,W", [(2, 1, 5, 3), (1, 3, 9, 11), (2, 1, 16, 16)])
def test_im2col(B, cin, H, W):
    """ld_dn_im2col is bit-equal to F.unfold(x, 7, padding=3) rearranged, with zeros in the padded columns, from a contiguous
    image and from a strided view of a larger one.  At 5 x 3 every window hangs over the border.  MI355X: bit-equal."""
    lib = cabi.lib()
    ldk = pad64(49 * cin)
    x = R.uniform((B, cin, H, W), 500 + cin + H)
    want = R.im2col(x, ldk)
    big = nans(B, cin + 1, H + 2, W + 3)
    big[:, 1:, 1:H + 1, 2:W + 2] = x.to(DEV)
    for src in (x.to(DEV), big[:, 1:, 1:H + 1, 2:W + 2]):
        out = nans(B, H, W, ldk)
        sb, sc, sh, sw = src.stride()
        cabi.check(lib.ld_dn_im2col(src.data_ptr(), out.data_ptr(), B, cin, H, W, sb, sc, sh, sw, ldk, st()), "dn_im2col")
        assert torch.equal(out.cpu(), want)
    assert bool((want[..., 49 * cin:] == 0).all())
    print(f"im2col B{B} cin{cin} {H}x{W}: bit-equal to F.unfold, {ldk - 49 * cin} zero columns")


# ------------------------------------------------------------------------------------------------ 2. the head kernels
@functools.lru_cache(maxsize=None)
def head_inputs(B, Cc, O, H, W):
    """Inputs and the two references of one case (computed once, never changed)."""
    key = 7 * Cc + 100 * O + H
    sd = R.make_layer("head", Cc, O, key=key)
    x, dout = R.uniform((B, Cc, H, W), 600 + key), R.uniform((B, O, H, W), 700 + key) / (B * H * W)
    return sd, x, dout, R.yardstick("head", sd, x, dout, F32), R.yardstick("head", sd, x, dout, F64)


def hip_head(sd, x, dout, ldc):
    B, Cc, H, W = x.shape
    O = dout.shape[1]
    lib = cabi.lib()
    xp, w, b, dz = padded(x, ldc), sd["weight"].to(DEV), sd["bias"].to(DEV), dout.to(DEV)
    out, dx, dw, db = nans(B, O, H, W), nans(B, H, W, ldc), nans(O, Cc, 1, 1), nans(O)
    cabi.check(lib.ld_dn_head_forward(xp.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), B, H, W, Cc, ldc, O, st()),
               "dn_head_forward")
    cabi.check(lib.ld_dn_head_backward(dz.data_ptr(), xp.data_ptr(), w.data_ptr(),
                                       work(lib.ld_dn_head_work_bytes(B, H, W, Cc, O)).data_ptr(), dw.data_ptr(), db.data_ptr(),
                                       dx.data_ptr(), B, H, W, Cc, ldc, O, st()), "dn_head_backward")
    return out, dx, dw, db


@pytest.mark.parametrize("B,H,W", [(2, 5, 3), (2, 14, 14), (1, 33, 31)])
@pytest.mark.parametrize("O", [1, 2, 3, 6])
@pytest.mark.parametrize("Cc,ldc", [(32, 64), (64, 64), (96, 128)])
def test_head_forward_and_backward(Cc, ldc, O, B, H, W):
    """ld_dn_head_forward / ld_dn_head_backward against autograd through F.conv2d: out (NCHW), dx, dw, db under the reduction
    bound; dx's padding is zero although x's holds NaN; a second call gives the same bits.  30 pixels are fewer than a wave,
    1,023 pixels are 32 parts of the split.  MI355X, largest rel err to fp64 over the 36 cases, HIP / fp32 eager torch: out 1.4e-7
    / 4.8e-7, dx 1.3e-7 / 1.1e-7, dw 5.6e-8 / 5.1e-7, db 4.8e-8 / 1.2e-6 (bound 1e-5)."""
    sd, x, dout, (o32, g32), (o64, g64) = head_inputs(B, Cc, O, H, W)
    out, dx, dw, db = hip_head(sd, x, dout, ldc)
    tag = f"head B{B} C{Cc} O{O} {H}x{W}"
    splits = int(cabi.lib().ld_dn_head_splits(B, H, W))
    print(f"{tag}: {splits} parts")
    if H * W > 1000:
        assert splits >= 2
    R.reduction_bound(out.cpu(), o64, o32, tag + " out")
    R.reduction_bound(unpadded(dx, Cc), g64["x"], g32["x"], tag + " dx")
    R.reduction_bound(dw.cpu(), g64["weight"], g32["weight"], tag + " dw")
    R.reduction_bound(db.cpu(), g64["bias"], g32["bias"], tag + " db")
    assert pad_is_zero(dx, Cc)
    for a, b in zip((out, dx, dw, db), hip_head(sd, x, dout, ldc)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3. the modules
def build(kind, cin, cout, sd=None):
    if kind == "down":
        mod = ldh.Downsample(cin, cout)
    elif kind == "up":
        mod = ldh.Upsample(cin, cout)
    else:
        k = {"conv3": 3, "stem": 7, "head": 1}[kind]
        mod = ldh.Conv2d(cin, cout, k, padding=k // 2)
    if sd is not None:
        mod.load_state_dict(sd)
    return mod.to(DEV)


def hip_forward_backward(mod, x, dout, x_grad=True):
    xd = x.to(DEV).requires_grad_(x_grad)
    mod.zero_grad(set_to_none=True)
    out = mod(xd)
    out.backward(dout.to(DEV))
    grads = {"x": xd.grad} if x_grad else {}
    grads.update({k: p.grad for k, p in mod.named_parameters() if p.grad is not None})
    return out.detach(), grads


MODULE_CASES = [("down", 2, 32, 32, 6, 10), ("down", 1, 32, 64, 14, 14), ("down", 2, 64, 128, 8, 8), ("down", 1, 96, 32, 10, 6),
                ("up", 2, 32, 32, 3, 5), ("up", 1, 64, 32, 7, 7), ("up", 1, 256, 128, 4, 4), ("up", 2, 96, 64, 5, 5),
                ("conv3", 2, 32, 32, 5, 3), ("conv3", 1, 128, 256, 4, 4), ("conv3", 2, 96, 64, 7, 7),
                ("stem", 2, 1, 32, 5, 3), ("stem", 1, 3, 64, 9, 11), ("stem", 2, 1, 32, 16, 16),
                ("head", 2, 32, 1, 5, 3), ("head", 1, 64, 3, 14, 14), ("head", 1, 96, 6, 33, 31)]


@pytest.mark.parametrize("kind,B,cin,cout,H,W", MODULE_CASES)
def test_module_forward_and_every_gradient(kind, B, cin, cout, H, W):
    """Forward and the gradients of x (but for the stem, which has none) and of the two parameters against the yardstick,
    dout = uniform / (B H W of the output).  The same call again, and again with every buffer the module allocates filled
    with NaN first, gives the same bits.  The head's result is NCHW and contiguous; the others' a channels_last view.
    MI355X, largest rel err to fp64, HIP / fp32 eager torch (bound 1e-5): Downsample out 4.4e-7 / 8.7e-7, dx 3.8e-7 / 3.8e-7,
    dw 2.0e-7 / 2.4e-7, db 3.2e-8 / 9.4e-8; Upsample out 1.2e-6 / 3.0e-7, dx 1.0e-6 / 2.8e-7, dw 1.8e-7 / 4.8e-7, db 3.4e-8 /
    1.6e-7; 3x3 out 8.6e-7 / 3.3e-7, dx 1.1e-6 / 2.8e-7, dw 1.9e-7 / 2.1e-7, db 3.3e-8 / 2.7e-7; stem out 5.7e-7 / 4.7e-7, dw
    1.6e-7 / 3.2e-7, db 3.4e-8 / 4.7e-7; head out 1.4e-7 / 4.8e-7, dx 1.2e-7 / 8.2e-8, dw 4.9e-8 / 2.9e-7, db 3.2e-8 / 3.9e-7."""
    sd = R.make_layer(kind, cin, cout, key=cin + cout)
    x = R.uniform((B, cin, H, W), 11 * cin + H)
    oshape = tuple(R.forward(kind, sd, x).shape)
    assert oshape == (B, cout, {"down": H // 2, "up": 2 * H}.get(kind, H), {"down": W // 2, "up": 2 * W}.get(kind, W))
    dout = R.uniform(oshape, 17 * cin + H) / (B * oshape[2] * oshape[3])
    x_grad = kind != "stem"
    mod = build(kind, cin, cout, sd)
    out, grads = hip_forward_backward(mod, x, dout, x_grad)
    (o32, g32), (o64, g64) = (R.yardstick(kind, sd, x, dout, dt, x_grad) for dt in (F32, F64))
    tag = f"{kind} B{B} {cin}->{cout} {H}x{W}"
    assert tuple(out.shape) == oshape
    assert out.is_contiguous() if kind == "head" else out.permute(0, 2, 3, 1).stride(-1) == 1
    assert set(grads) == set(g64), set(grads) ^ set(g64)
    R.reduction_bound(out.cpu(), o64, o32, tag + " out")
    for k in g64:
        assert grads[k].shape == g64[k].shape, k
        R.reduction_bound(grads[k].cpu(), g64[k], g32[k], f"{tag} d {k}")
    for fill in (None, NAN):
        mod.debug_fill = fill
        out2, grads2 = hip_forward_backward(mod, x, dout, x_grad)
        assert torch.equal(out, out2)
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), (k, fill)


def test_module_refusals_on_the_gpu():
    """An odd H or W for Downsample, an x that requires grad for the stem, a parameter on another device: ValueError under the
    module's own name."""
    down, stem = build("down", 32, 32), build("stem", 1, 32)
    with pytest.raises(ValueError, match="Downsample.*even"):
        down(torch.zeros(1, 32, 5, 4, device=DEV))
    with pytest.raises(ValueError, match="Downsample.*even"):
        down(torch.zeros(1, 32, 4, 7, device=DEV))
    with pytest.raises(ValueError, match="Conv2d.*no input gradient"):
        stem(torch.zeros(1, 1, 4, 4, device=DEV, requires_grad=True))
    assert stem(torch.zeros(1, 1, 4, 4, device=DEV)).requires_grad                     # data in: fine
    for mod, c in ((ldh.Downsample(32), 32), (ldh.Upsample(32), 32), (ldh.Conv2d(32, 2, 1), 32)):
        with pytest.raises(ValueError, match=type(mod).__name__ + ".*parameter"):
            mod(torch.zeros(1, c, 4, 4, device=DEV))
        with pytest.raises(ValueError, match=type(mod).__name__ + ".*float32"):
            mod.to(DEV)(torch.zeros(1, c, 4, 4, device=DEV, dtype=torch.float16))


def test_downsample_weight_packing_round_trip():
    """The reference's columns (c p1 p2) are packed to the kernels' (p1 p2 c) for the forward ([cop][4 dim]) and transposed for
    the data gradient ([4 dim][cop]); ld_dn_gather3 with the strides the weight gradient is gathered with gives the parameter
    back exactly; rows and columns of the padded output channels are zero."""
    dim, dim_out = 32, 96
    mod = build("down", dim, dim_out, R.make_layer("down", dim, dim_out, key=3))
    p = mod._packed_for(torch.device(DEV, torch.cuda.current_device()))
    w = mod.state_dict()["1.weight"]
    cop = pad64(dim_out)
    want = torch.zeros(cop, 4 * dim, device=DEV)
    want[:dim_out] = w.reshape(dim_out, dim, 4).permute(0, 2, 1).reshape(dim_out, 4 * dim)
    assert torch.equal(p.wf.reshape(cop, 4 * dim), want) and torch.equal(p.wd.reshape(4 * dim, cop), want.t())
    back = nans(dim_out, 4 * dim, 1, 1)
    cabi.check(cabi.lib().ld_dn_gather3(p.wf.data_ptr(), back.data_ptr(), dim_out, dim, 4, 0, 4 * dim, 1, dim, st()), "gather3")
    assert torch.equal(back, w)


# ------------------------------------------------------------------------------------------------ 4. autograd behaviour
@pytest.mark.parametrize("kind,cin,cout", [("down", 32, 64), ("up", 32, 64), ("conv3", 32, 64), ("head", 32, 2)])
def test_autograd_contract(kind, cin, cout):
    """backward twice accumulates into .grad; a no_grad forward equals the grad-mode forward bit for bit and needs no
    gradient; autograd.grad works; an in-place change of a parameter (its _version moves) rebuilds the packed weights."""
    sd = R.make_layer(kind, cin, cout, key=31)
    x = R.uniform((2, cin, 6, 8), 81)
    dout = R.uniform(tuple(R.forward(kind, sd, x).shape), 83)
    mod = build(kind, cin, cout, sd)
    out, g1 = hip_forward_backward(mod, x, dout)
    g1 = {k: v.clone() for k, v in g1.items()}
    mod(x.to(DEV)).backward(dout.to(DEV))                                   # a second backward without zero_grad
    for k, p in mod.named_parameters():
        assert torch.equal(p.grad, 2 * g1[k]), k
    with torch.no_grad():
        quiet = mod(x.to(DEV))
    assert not quiet.requires_grad and torch.equal(quiet, out)
    weight = dict(mod.named_parameters())[[k for k in sd if k.endswith("weight")][0]]
    (gw,) = torch.autograd.grad(mod(x.to(DEV).requires_grad_(True)).sum(), [weight])
    assert gw.shape == weight.shape
    with torch.no_grad():
        weight.mul_(0.5)
        after = mod(x.to(DEV))
    assert not torch.equal(after, out)
    sd_new = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    assert R.rel_err(after.cpu(), R.forward(kind, sd_new, x, F64)) <= 1e-5


@pytest.mark.parametrize("kind,cout", [("down", 64), ("up", 32), ("conv3", 64), ("head", 3)])
def test_module_reads_channels_last_in_place(kind, cout):
    """A channels_last x with 64 channels is the kernels' NHWC already: same bits as from a contiguous x, x.grad included,
    and x itself is not written."""
    cin = 64
    sd = R.make_layer(kind, cin, cout, key=5)
    x = R.uniform((2, cin, 6, 4), 51)
    dout = R.uniform(tuple(R.forward(kind, sd, x).shape), 53)
    mod = build(kind, cin, cout, sd)
    out, grads = hip_forward_backward(mod, x, dout)
    xl = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    out2 = mod(xl)
    out2.backward(dout.to(DEV).contiguous(memory_format=torch.channels_last))
    assert torch.equal(out, out2) and torch.equal(grads["x"], xl.grad)
    for k, p in mod.named_parameters():
        assert torch.equal(grads[k], p.grad), k
    assert torch.equal(xl.detach().cpu(), x)                                # the input itself was not written


# ------------------------------------------------------------------------------------------------ 5. a small U, and Adam
def test_chain_of_a_small_u_under_the_loss_gradient():
    """stem(1 -> 32) -> ResnetBlock(32, 32) = s -> Downsample(32, 64) -> ResnetBlock(64, 64) -> Upsample(64, 32) -> cat with s
    -> ResnetBlock(64, 32) -> head(32 -> 1), the gradient of the pred_v training loss (ld_p_losses_grad) as the upstream
    gradient, at B = 2, 12 x 12, time_emb_dim 128, against the fp64 yardstick of the same chain: every parameter gradient of
    all seven modules.  The cat and the skip's fan-out are autograd's.  MI355X: over the 40 gradients at most 1.6e-6 (HIP) /
    8.8e-7 (fp32 eager torch) to fp64, bound 1e-5."""
    B, H, tdim = 2, 12, 128
    kinds = [("stem", 1, 32), ("block", 32, 32), ("down", 32, 64), ("block", 64, 64), ("up", 64, 32), ("block", 64, 32),
             ("head", 32, 1)]
    sds = [resblock_ref.make_block(ci, co, tdim, key=40 + i) if k == "block" else R.make_layer(k, ci, co, key=40 + i)
           for i, (k, ci, co) in enumerate(kinds)]
    mods = []
    for (k, ci, co), sd in zip(kinds, sds):
        if k == "block":
            m = ldh.ResnetBlock(ci, co, time_emb_dim=tdim)
            m.load_state_dict(sd)
            mods.append(m.to(DEV))
        else:
            mods.append(build(k, ci, co, sd))
    x, temb = R.uniform((B, 1, H, H), 61), R.uniform((B, tdim), 62)
    x0, nz = R.uniform((B, 1, H, H), 63), R.uniform((B, 1, H, H), 64)
    t = torch.tensor([0, 3])
    sab, s1m, lw = torch.tensor([0.99, 0.9, 0.7, 0.4]), torch.tensor([0.14, 0.43, 0.71, 0.92]), torch.tensor([1.0, 0.8, 0.5, 0.3])
    td = temb.to(DEV)
    s = mods[1](mods[0](x.to(DEV)), td)
    h = mods[4](mods[3](mods[2](s), td))
    out = mods[6](mods[5](torch.cat((h, s), dim=1), td))
    od = out.detach()
    assert od.is_contiguous() and tuple(od.shape) == (B, 1, H, H)
    up = nans(*od.shape)
    dev = [v.to(DEV) for v in (x0, nz, t.int(), sab, s1m, lw)]
    cabi.check(cabi.lib().ld_p_losses_grad(od.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                                           dev[3].data_ptr(), dev[4].data_ptr(), dev[5].data_ptr(), 1.0, up.data_ptr(), B,
                                           H * H, cabi.OBJ["pred_v"], st()), "p_losses_grad")
    out.backward(up)
    got = {f"{i}.{k}": p.grad for i, m in enumerate(mods) for k, p in m.named_parameters()}
    ref = {}
    for dt in (F32, F64):
        ls = [{k: v.to(dt).clone().requires_grad_(True) for k, v in sd.items()} for sd in sds]

        def blk(i, a):
            return R.unet_ref.resnet_block({"a." + k: v for k, v in ls[i].items()}, "a", a, temb.to(dt))
        ss = blk(1, R.apply("stem", ls[0], x.to(dt)))
        hh = R.apply("up", ls[4], blk(3, R.apply("down", ls[2], ss)))
        o = R.apply("head", ls[6], blk(5, torch.cat((hh, ss), dim=1)))
        ext = (slice(None), None, None, None)
        target = sab.to(dt)[t][ext] * nz.to(dt) - s1m.to(dt)[t][ext] * x0.to(dt)
        loss = (((o - target) ** 2).reshape(B, -1).mean(dim=1) * lw.to(dt)[t]).mean()
        names = [f"{i}.{k}" for i, l in enumerate(ls) for k in l]
        ref[dt] = dict(zip(names, torch.autograd.grad(loss, [v for l in ls for v in l.values()])))
    assert set(got) == set(ref[F64])
    for k in ref[F64]:
        assert got[k] is not None, k
        R.reduction_bound(got[k].cpu(), ref[F64][k], ref[F32][k], "chain d " + k)


def test_adam_lowers_a_fixed_mse_at_every_step():
    """Five steps of torch.optim.Adam(lr=1e-3) on Downsample(32, 64) -> Upsample(64, 32) on a fixed batch: the optimiser's
    in-place updates move the parameters' versions, the kernel-layout weights follow, and the loss falls at every step.
    MI355X: 0.382540 0.357395 0.336090 0.317946 0.302348 0.288736."""
    down, up = build("down", 32, 64, R.make_layer("down", 32, 64, key=41)), build("up", 64, 32, R.make_layer("up", 64, 32, key=42))
    x, target = R.uniform((2, 32, 8, 8), 91).to(DEV), R.uniform((2, 32, 8, 8), 93).to(DEV)
    opt = torch.optim.Adam(list(down.parameters()) + list(up.parameters()), lr=1e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = F.mse_loss(up(down(x)), target)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print("adam losses:", " ".join(f"{v:.6f}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_with_device_pointers():
    """Null or misaligned pointers and bad sizes return -1 and write nothing."""
    lib = cabi.lib()
    buf = torch.zeros(8192, device=DEV)
    p = buf.data_ptr()
    for fn in (lib.ld_dn_space_to_depth, lib.ld_dn_depth_to_space, lib.ld_dn_upsample2x, lib.ld_dn_upsample2x_backward):
        assert fn(p, None, 1, 2, 2, 32, 64, st()) == -1 and b"null" in lib.ld_last_error()
        assert fn(p, p + 4, 1, 2, 2, 32, 64, st()) == -1 and b"aligned" in lib.ld_last_error()
        assert fn(p, p, 1, 2, 2, 32, 16, st()) == -1
    assert lib.ld_dn_im2col(p, p + 4, 1, 1, 4, 4, 16, 16, 4, 1, 64, st()) == -1 and b"aligned" in lib.ld_last_error()
    assert lib.ld_dn_im2col(p, p, 1, 5, 4, 4, 80, 16, 4, 1, 256, st()) == -1
    assert lib.ld_dn_head_forward(p, p, p, p, 1, 4, 4, 32, 64, 9, st()) == -1
    assert lib.ld_dn_head_forward(p, p + 4, p, p, 1, 4, 4, 32, 64, 1, st()) == -1 and b"aligned" in lib.ld_last_error()
    assert lib.ld_dn_head_backward(p, p, p, p, p, p, None, 1, 4, 4, 32, 64, 1, st()) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_head_backward(p, p, p, p, p, p, p, 1, 4, 4, 48, 64, 1, st()) == -1
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
