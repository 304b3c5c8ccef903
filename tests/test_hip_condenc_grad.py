"""GPU tests of the fifth slice of the denoiser's backward pass: the GroupNorm -> ReLU and im2col kernels of
csrc/condenc_grad.hip one by one, then ``BasicBlock`` and ``ResUnet`` as wholes, against the real reference's recorded
activations, under torch.autograd, in a chain with a ``ResnetBlock`` under a loss and under Adam.

Yardstick: torch.autograd in fp64 on the CPU through tests/condenc_ref.py's restatement (equal to
oracle.unet_ref.cond_encoder bit for bit: test_condenc_grad.py).  Element-wise results are held to RTOL["fp32"] of fp32 torch,
everything behind a sum over pixels or channels to max(1e-5, 4 d) of the fp64 value, d = fp32 eager torch's own distance to it
(resblock_ref.reduction_bound).  The inputs of every comparison of a gradient meet the margin condition (condenc_ref: no
pre-ReLU value and no gap at the top of a pool window within 2e-5 of the tensor's range; asserted on the CPU in
test_condenc_grad.py), so no element is excluded anywhere.  Every buffer handed to a kernel is filled with NaN first, padding
included, and padding must come out as zero.  Every test prints HIP's and torch's distances; the docstrings quote those of one MI355X run
(docs/findings.md, 126)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import rng

from hip_helpers import DEV, NAN, RTOL, nans, pad64, padded, st, unpadded
import condenc_ref as R
import resblock_ref

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
G = R.GROUPS


def pad_is_zero(t, c):
    return t.shape[-1] == c or bool((t[..., c:] == 0).all())


# ------------------------------------------------------------------------------------------------ 1. the GroupNorm kernels
@functools.lru_cache(maxsize=None)
def gn_case(C, B, H, W, nop, relu):
    """Inputs and the two references of one case (computed once, never changed)."""
    t, dout = R.gn_inputs(C, B, H, W, nop, R.GN_KEYS[(C, B, H, W, nop)])
    return t, dout, R.gn_yardstick(t, dout, bool(relu), F32), R.gn_yardstick(t, dout, bool(relu), F64)


def hip_gn(t, dout, ldc, relu, in_place=False):
    """ld_dn_gnr_forward then ld_dn_gnr_backward on NaN-padded inputs; ``in_place``: dy is dout's buffer."""
    lib = cabi.lib()
    B, C, H, W = t["y"].shape
    two = "y2" in t
    dev = {k: (padded(v, ldc) if v.dim() == 4 else v.to(DEV)) for k, v in t.items()}
    nbytes = int(lib.ld_dn_gnr_work_bytes(B, H, W, C, G))
    assert nbytes > 0
    r = dict(out=nans(B, H, W, ldc), stat=nans(B, G, 2), stat2=nans(B, G, 2) if two else None)
    work = nans(nbytes // 8, dtype=F64)
    cabi.check(lib.ld_dn_gnr_forward(dev["y"].data_ptr(), dev["gamma"].data_ptr(), dev["beta"].data_ptr(), cabi.ptr(dev.get("y2")),
                                     cabi.ptr(dev.get("gamma2")), cabi.ptr(dev.get("beta2")), work.data_ptr(), r["stat"].data_ptr(),
                                     cabi.ptr(r["stat2"]), r["out"].data_ptr(), B, H, W, C, ldc, G, relu, st()), "dn_gnr_forward")
    dop = padded(dout, ldc)
    r.update(gamma=nans(C), beta=nans(C), y=dop if in_place else nans(B, H, W, ldc))
    if two:
        r.update(gamma2=nans(C), beta2=nans(C), y2=nans(B, H, W, ldc))
    work = nans(nbytes // 8, dtype=F64)
    cabi.check(lib.ld_dn_gnr_backward(dop.data_ptr(), r["out"].data_ptr() if relu else None, dev["y"].data_ptr(),
                                      r["stat"].data_ptr(), dev["gamma"].data_ptr(), cabi.ptr(dev.get("y2")), cabi.ptr(r["stat2"]),
                                      cabi.ptr(dev.get("gamma2")), work.data_ptr(), r["gamma"].data_ptr(), r["beta"].data_ptr(),
                                      r["y"].data_ptr(), cabi.ptr(r.get("gamma2")), cabi.ptr(r.get("beta2")), cabi.ptr(r.get("y2")),
                                      B, H, W, C, ldc, G, relu, st()), "dn_gnr_backward")
    return r


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("nop", [1, 2])
@pytest.mark.parametrize("C,ldc,B,H,W", R.GN_CASES)
def test_gn_forward_and_backward(C, ldc, B, H, W, nop, relu):
    """ld_dn_gnr_forward / ld_dn_gnr_backward at 2, 2, 4, 8 and 16 channels per group, with padding (32 of 64) and without, in
    the one- and the two-operand form, with and without the ReLU: out within RTOL of fp32 torch, the statistics and dgamma,
    dbeta, dy of each operand under the reduction bound; the inputs' padding holds NaN and is never read, the outputs' is
    zero; a second call gives the same bits, and so does dy written over dout.  30 pixels are fewer than a wave, 1,600 pixels
    at 32 channels are 100 runs merged in order.  MI355X, largest rel err to fp64 over the 44 cases, HIP / fp32 eager torch
    (bound 1e-5): mean 5.7e-8 / 2.0e-7, rstd 3.3e-8 / 8.8e-8, dgamma 1.0e-7 / 4.0e-7, dbeta 5.5e-8 / 2.9e-7, dy 2.0e-7 / 2.3e-7;
    out at most 2.1e-7 from fp32 torch (bound 2e-5)."""
    t, dout, (o32, g32, _), (o64, g64, _) = gn_case(C, B, H, W, nop, relu)
    r = hip_gn(t, dout, ldc, relu)
    tag = f"gn C{C}/{ldc} B{B} {H}x{W} operands {nop} relu {relu}"
    resblock_ref.elementwise_bound(unpadded(r["out"], C), o32, o64, tag + " out", rtol=RTOL["fp32"])
    assert pad_is_zero(r["out"], C)
    for sfx in ("", "2")[:nop]:
        s32, s64, got = R.gn_stats(t["y" + sfx], F32), R.gn_stats(t["y" + sfx], F64), r["stat" + sfx].cpu()
        R.reduction_bound(got[..., 0], s64[..., 0], s32[..., 0], f"{tag} mean{sfx}")
        R.reduction_bound(got[..., 1], s64[..., 1], s32[..., 1], f"{tag} rstd{sfx}")
        for k in ("gamma" + sfx, "beta" + sfx):
            R.reduction_bound(r[k].cpu(), g64[k], g32[k], f"{tag} d {k}")
        R.reduction_bound(unpadded(r["y" + sfx], C), g64["y" + sfx], g32["y" + sfx], f"{tag} d y{sfx}")
        assert pad_is_zero(r["y" + sfx], C)
    if nop == 2:
        assert torch.equal(r["beta"], r["beta2"])                                    # one masked gradient, one sum
    again, alias = hip_gn(t, dout, ldc, relu), hip_gn(t, dout, ldc, relu, in_place=True)
    for k, v in r.items():
        if v is not None:
            assert torch.equal(v, again[k]), k
            assert torch.equal(v, alias[k]), k


@pytest.mark.parametrize("B,cin,H,W", [(2, 1, 5, 7), (1, 3, 5, 7)])
def test_im2col3(B, cin, H, W):
    """ld_dn_im2col3 is bit-equal to F.unfold(x, 3, padding=1) rearranged, with zeros in the columns from 9 Cin on, from a
    contiguous image and from a strided view of a larger one; at 5 x 7 every window of the border hangs over it.  MI355X:
    bit-equal."""
    lib = cabi.lib()
    ldk = pad64(9 * cin)
    x = R.uniform((B, cin, H, W), 500 + cin + H)
    want = R.im2col3(x, ldk)
    big = nans(B, cin + 1, H + 2, W + 3)
    big[:, 1:, 1:H + 1, 2:W + 2] = x.to(DEV)
    view = big[:, 1:, 1:H + 1, 2:W + 2]
    assert not view.is_contiguous()
    for src in (x.to(DEV), view):
        out = nans(B, H, W, ldk)
        sb, sc, sh, sw = src.stride()
        cabi.check(lib.ld_dn_im2col3(src.data_ptr(), out.data_ptr(), B, cin, H, W, sb, sc, sh, sw, ldk, st()), "dn_im2col3")
        assert torch.equal(out.cpu(), want)
    assert bool((want[..., 9 * cin:] == 0).all())
    print(f"im2col3 B{B} cin{cin} {H}x{W}: bit-equal to F.unfold, {ldk - 9 * cin} zero columns")


# ------------------------------------------------------------------------------------------------ 2. the modules
def fill(mod, value):
    for m in mod.modules():
        if isinstance(m, ldh.BasicBlock):
            m.debug_fill = value


def hip_forward_backward(mod, x, dout, x_grad=True):
    xd = x.to(DEV).requires_grad_(x_grad)
    mod.zero_grad(set_to_none=True)
    out = mod(xd)
    out.backward(dout.to(DEV))
    grads = {"x": xd.grad} if x_grad else {}
    grads.update({k: p.grad for k, p in mod.named_parameters() if p.grad is not None})
    return out.detach(), grads


def compare(mod, x, dout, x_grad, ref32, ref64, tag, nparams):
    """Output and every gradient under the reduction bound; the same call again, and again with every buffer the module
    allocates filled with NaN first, gives the same bits."""
    fill(mod, NAN)
    out, grads = hip_forward_backward(mod, x, dout, x_grad)
    (o32, g32, _), (o64, g64, _) = ref32, ref64
    assert tuple(out.shape) == tuple(o64.shape) and out.permute(0, 2, 3, 1).stride(-1) == 1
    assert set(grads) == set(g64) and len(g64) == nparams + int(x_grad), set(grads) ^ set(g64)
    R.reduction_bound(out.cpu(), o64, o32, tag + " out")
    for k in g64:
        assert grads[k].shape == g64[k].shape, k
        R.reduction_bound(grads[k].cpu(), g64[k], g32[k], f"{tag} d {k}")
    for value in (NAN, None):
        fill(mod, value)
        out2, grads2 = hip_forward_backward(mod, x, dout, x_grad)
        assert torch.equal(out, out2)
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), (k, value)


@pytest.mark.parametrize("case", R.BLOCK_CASES)
def test_block_forward_and_every_gradient(case):
    """``BasicBlock`` against the yardstick: the output, dx (none for the two image blocks) and all twelve parameter
    gradients, dout = uniform / (B H W of the output); 2, 2, 4, 8 and 16 channels per group, with the pool and without, an
    odd W without it.  MI355X, largest rel err to fp64 over the five cases, HIP / fp32 eager torch (bound 1e-5): out 7.4e-7 /
    2.8e-7, dx 9.7e-7 / 3.3e-7, convolution weights 7.1e-7 / 3.7e-7 and biases 1.1e-6 / 4.5e-7, GroupNorm parameters 1.3e-6 /
    5.2e-7."""
    cin, cmid, cout, pool, B, H, W = case
    sd, x, dout = R.block_inputs(case, R.BLOCK_KEYS[case])
    x_grad = cin > 4
    mod = ldh.BasicBlock(cin, cmid, cout, pool=pool)
    mod.load_state_dict(sd)
    refs = [R.yardstick(sd, x, dout, dt, pool=pool, x_grad=x_grad) for dt in (F32, F64)]
    assert tuple(refs[1][0].shape) == (B, cout, H // 2 if pool else H, W // 2 if pool else W)
    compare(mod.to(DEV), x, dout, x_grad, *refs, f"block {cin}->{cmid}->{cout} pool {int(pool)} B{B} {H}x{W}", 12)


@pytest.mark.parametrize("case", R.ENCODER_CASES)
def test_resunet_forward_and_every_gradient(case):
    """``ResUnet`` on the procedural weights against the yardstick: the output and every parameter gradient (48, or 36 for
    'mnist', which returns after the third block).  MI355X, largest rel err to fp64 over the three cases, HIP / fp32 eager
    torch (bound 1e-5): out 7.5e-7 / 7.9e-7, convolution weights 1.3e-6 / 8.6e-7 and biases 1.2e-6 / 1.0e-6, GroupNorm parameters
    2.5e-6 / 1.1e-6."""
    data, B, H, W = case
    sd, x, dout = R.encoder_inputs(case, R.ENCODER_KEYS[case])
    net = ldh.ResUnet(data)
    net.load_state_dict(sd)
    refs = [R.yardstick(sd, x, dout, dt, data=data, x_grad=False) for dt in (F32, F64)]
    div, cout = (4, 128) if data == "mnist" else (8, 256)
    assert tuple(refs[1][0].shape) == (B, cout, H // div, W // div)
    compare(net.to(DEV), x, dout, False, *refs, f"ResUnet {data} B{B} {H}x{W}", len(sd))


@pytest.mark.parametrize("tag,data", [("mri64", "mri"), ("mnist28", "mnist"), ("mvtec32", "mvtec")])
def test_forward_against_the_references_recorded_activations(golden, tag, data):
    """The ``cond_model.`` slice of the procedural weights in ``ldh.ResUnet`` on the golden file's condition image: mean, norm
    and the 16 samples of the real reference's ``cond_model`` activation (tests/golden/g2_unet_forward.npz), to the
    tolerances test_oracle_golden.test_unet_forward holds the oracle to.  MI355X: means equal to six places, norms 127.0419,
    160.7145 (recorded 160.7146) and 90.9227, samples off by at most 2.4e-6, 4.3e-6 and 3.1e-6."""
    g = golden("g2_unet_forward")
    B, _, H, cin = [int(v) for v in g[f"{tag}_shape"]]
    rec = g[sorted(k for k in g.files if k.startswith(tag + "_t") and k.endswith("_tap_cond_model"))[0]]
    net = ldh.ResUnet(data)
    net.load_state_dict(R.encoder_state(data))
    fill(net, NAN)
    assert net.in_channels == cin
    cond = torch.from_numpy(rng.uniform((B, cin, H, H), 1, 101, 0.0, 2.0))
    with torch.no_grad():
        out = net.to(DEV)(cond.to(DEV)).float().cpu().contiguous()
    flat = out.flatten()
    samples = flat[torch.linspace(0, flat.numel() - 1, 16).long()]
    print(f"{tag}: mean {float(out.mean()):.6f} / {rec[0]:.6f}, norm {float(out.norm()):.4f} / {rec[1]:.4f}, samples off by "
          f"{float((samples - torch.from_numpy(rec[2:])).abs().max()):.2e}")
    assert abs(float(out.mean()) - rec[0]) < 1e-4
    assert abs(float(out.norm()) - rec[1]) < 1e-3 * max(1.0, rec[1])
    assert float((samples - torch.from_numpy(rec[2:])).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------ 3. autograd behaviour
@pytest.mark.parametrize("cin,cmid,cout,pool", [(32, 32, 64, True), (64, 64, 128, False), (1, 32, 32, True)])
def test_autograd_contract(cin, cmid, cout, pool):
    """backward twice accumulates into .grad; a no_grad forward equals the grad-mode forward bit for bit and needs no
    gradient; autograd.grad works; an in-place change of a parameter (its _version moves) rebuilds the packed weights; a
    channels_last x with 64 channels is read in place: same bits as from a contiguous x, x.grad included."""
    sd = R.make_block(cin, cmid, cout, key=31)
    x_grad = cin > 4
    x = R.uniform((2, cin, 6, 8), 81)
    dout = R.uniform(R.out_shape(sd, x, pool), 83)
    mod = ldh.BasicBlock(cin, cmid, cout, pool=pool)
    mod.load_state_dict(sd)
    mod = mod.to(DEV)
    out, g1 = hip_forward_backward(mod, x, dout, x_grad)
    g1 = {k: v.clone() for k, v in g1.items()}
    mod(x.to(DEV)).backward(dout.to(DEV))                                   # a second backward without zero_grad
    for k, p in mod.named_parameters():
        assert torch.equal(p.grad, 2 * g1[k]), k
    with torch.no_grad():
        quiet = mod(x.to(DEV))
    assert not quiet.requires_grad and torch.equal(quiet, out)
    weight = mod.convblock[3].weight
    (gw,) = torch.autograd.grad(mod(x.to(DEV).requires_grad_(x_grad)).sum(), [weight])
    assert gw.shape == weight.shape
    if cin % 64 == 0:
        xl = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        mod.zero_grad(set_to_none=True)
        out2 = mod(xl)
        out2.backward(dout.to(DEV).contiguous(memory_format=torch.channels_last))
        assert torch.equal(out, out2) and torch.equal(g1["x"], xl.grad)
        for k, p in mod.named_parameters():
            assert torch.equal(g1[k], p.grad), k
        assert torch.equal(xl.detach().cpu(), x)                            # the input itself was not written
    with torch.no_grad():
        weight.mul_(0.5)
        after = mod(x.to(DEV))
    assert not torch.equal(after, out)
    sd_new = {k: v.detach().cpu().double() for k, v in mod.state_dict().items()}
    with torch.no_grad():
        assert R.rel_err(after.cpu(), R.basic_block(sd_new, x.double(), pool)) <= 1e-5


def test_module_refusals_on_the_gpu():
    """An odd H or W with the pool, an image x that requires grad, a parameter on another device, a 16-bit x: ValueError
    under the module's own name."""
    blk = ldh.BasicBlock(32, 32, 64, pool=True).to(DEV)
    for shape in ((1, 32, 5, 4), (1, 32, 4, 7)):
        with pytest.raises(ValueError, match="BasicBlock.*even"):
            blk(torch.zeros(*shape, device=DEV))
    img = ldh.BasicBlock(1, 32, 32).to(DEV)
    with pytest.raises(ValueError, match="BasicBlock.*no input gradient"):
        img(torch.zeros(1, 1, 4, 4, device=DEV, requires_grad=True))
    assert img(torch.zeros(1, 1, 3, 5, device=DEV)).requires_grad                         # data in: fine, odd sizes too
    with pytest.raises(ValueError, match="BasicBlock.*parameter"):
        ldh.BasicBlock(32, 32, 64)(torch.zeros(1, 32, 4, 4, device=DEV))
    with pytest.raises(ValueError, match="BasicBlock.*float32"):
        blk(torch.zeros(1, 32, 4, 4, device=DEV, dtype=torch.float16))
    with pytest.raises(ValueError, match="ResUnet.*divisible"):
        ldh.ResUnet("mri").to(DEV)(torch.zeros(1, 1, 12, 16, device=DEV))


# ------------------------------------------------------------------------------------------------ 4. a chain, and Adam
def test_chain_with_a_resnet_block_under_a_loss():
    """ResUnet('mri') on [2, 1, 8, 16] -> feat [2, 256, 1, 2]; cat(feat', feat) -> ResnetBlock(512, 256) (conv_fusion's place
    and shape) -> MSE: every one of the encoder's 48 parameter gradients against the fp64 chain.  The cat and the loss are
    autograd's.  MI355X: at most 2.4e-6 (HIP) / 1.2e-6 (fp32 eager torch) to fp64, bound 1e-5."""
    sd, blk_sd, x, other, target = R.chain_inputs(R.CHAIN_KEYS["chain"])
    net, blk = ldh.ResUnet("mri"), ldh.ResnetBlock(512, 256)
    net.load_state_dict(sd)
    blk.load_state_dict(blk_sd)
    net, blk = net.to(DEV), blk.to(DEV)
    fill(net, NAN)
    loss = F.mse_loss(blk(torch.cat((other.to(DEV), net(x.to(DEV))), dim=1)), target.to(DEV))
    loss.backward()
    (l32, g32, _), (l64, g64, _) = (R.chain_yardstick(sd, blk_sd, x, other, target, dt) for dt in (F32, F64))
    print(f"chain loss: HIP {float(loss.detach()):.8f}, fp32 torch {l32:.8f}, fp64 {l64:.8f}")
    got = {k: p.grad for k, p in net.named_parameters()}
    assert set(got) == set(g64) and len(got) == 48
    for k in g64:
        assert got[k] is not None, k
        R.reduction_bound(got[k].cpu(), g64[k], g32[k], "chain d " + k)


def test_adam_lowers_a_fixed_mse_at_every_step():
    """Five steps of torch.optim.Adam(lr=1e-3) on ResUnet('mnist') on a fixed batch: the optimiser's in-place updates move the
    parameters' versions, the kernel-layout weights follow, and the loss falls at every step.  MI355X: 0.750136 0.430797
    0.268116 0.201627 0.176644 0.166439."""
    net = ldh.ResUnet("mnist")
    net.load_state_dict(R.encoder_state("mnist"))
    net = net.to(DEV)
    x, target = R.encoder_input("mnist", 2, 12, 12, 0).to(DEV), R.uniform((2, 128, 3, 3), 93, 0.0, 1.0).to(DEV)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = F.mse_loss(net(x), target)
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
    p, N = buf.data_ptr(), None
    shape = (1, 4, 4, 32, 64, 16, 1)
    assert lib.ld_dn_gnr_forward(p, p, p, N, N, N, p, p, N, N, *shape, st()) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_gnr_forward(p, p, p, p, N, N, p, p, N, p, *shape, st()) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_gnr_forward(p, p, p, N, N, N, p, p, N, p + 4, *shape, st()) == -1 and b"aligned" in lib.ld_last_error()
    assert lib.ld_dn_gnr_forward(p, p, p, N, N, N, p, p, N, p, 1, 4, 4, 48, 64, 16, 1, st()) == -1
    assert lib.ld_dn_gnr_forward(p, p, p, N, N, N, p, p, N, p, 1, 4, 4, 16, 64, 16, 1, st()) == -1
    for args in ((p, N, p, p, p, N, N, N, p, p, p, p, N, N, N),          # relu without the saved result
                 (p, p, p, p, p, N, N, N, p, p, p, N, N, N, N),          # no dy
                 (p, p, p, p, p, p, p, p, p, p, p, p, p, p, N)):         # two operands, no dy2
        assert lib.ld_dn_gnr_backward(*args, *shape, st()) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_gnr_backward(p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, *shape, st()) == -1     # dy2 == dy
    assert lib.ld_dn_gnr_backward(p, p, p, p, p, N, N, N, p, p, p, p + 8, N, N, N, *shape, st()) == -1 and \
        b"aligned" in lib.ld_last_error()
    assert lib.ld_dn_gnr_backward(p, p, p, p, p, N, N, N, p, p, p, p, N, N, N, 1, 4, 4, 32, 16, 16, 1, st()) == -1
    assert lib.ld_dn_im2col3(p, p + 4, 1, 1, 4, 4, 16, 16, 4, 1, 64, st()) == -1 and b"aligned" in lib.ld_last_error()
    assert lib.ld_dn_im2col3(p, p, 1, 5, 4, 4, 80, 16, 4, 1, 64, st()) == -1
    assert lib.ld_dn_im2col3(p, N, 1, 1, 4, 4, 16, 16, 4, 1, 64, st()) == -1 and b"null" in lib.ld_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
