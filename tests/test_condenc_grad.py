"""CPU-side checks of the trainable condition encoder, ``ldh.BasicBlock`` and ``ldh.ResUnet`` (no GPU needed): the public
surface, the reference's state_dict names, shapes and order, the constructors' and the inputs' refusals, the C ABI's
declarations, bindings and refusals, the torch restatement the GPU tests compare with against the oracle, and the margin
condition of every case whose gradients the GPU tests compare (tests/condenc_ref.py)."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import weights
from oracle import unet_ref

import condenc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ld_dn_gnr_work_bytes", "ld_dn_gnr_forward", "ld_dn_gnr_backward", "ld_dn_im2col3"]
F64 = torch.float64


def test_public_surface():
    for name in ("BasicBlock", "ResUnet"):
        assert name in ldh.__all__
        assert getattr(ldh, name).__module__.endswith(".condenc")
    assert issubclass(ldh.BasicBlock, ldh.ResnetBlock.__mro__[1])                   # a TrainableModule
    assert issubclass(ldh.ResUnet, torch.nn.Module) and not issubclass(ldh.ResUnet, ldh.ResnetBlock.__mro__[1])
    blk = ldh.BasicBlock(32, 32, 64)
    assert blk.debug_fill is None and callable(blk.invalidate)


@pytest.mark.parametrize("data", ["mri", "mnist", "mvtec"])
def test_state_dict_is_the_unets_cond_model(data):
    """Names, shapes and order of ``ResUnet(data).state_dict()`` are the reference Unet's under ``cond_model.``; the slice of
    a checkpoint loads by name; every block is the only member of an nn.Sequential of the reference's name."""
    cfg = R.CONFIGS[data]
    want = [(k[len("cond_model."):], v) for k, v in weights.unet_param_shapes(cfg).items() if k.startswith("cond_model.")]
    net = ldh.ResUnet(data)
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert got == want and len(want) == (48 if cfg.cond_has_mid else 36)
    assert net.in_channels == cfg.cond_in_channels and net.filters == [32, 32, 64, 128, 256]
    assert hasattr(net, "mid_conv") == cfg.cond_has_mid
    sd = R.encoder_state(data)
    net.load_state_dict(sd)
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    blocks = [net.residual_conv1, net.residual_conv2, net.residual_conv3] + ([net.mid_conv] if cfg.cond_has_mid else [])
    for seq in blocks:
        assert isinstance(seq, torch.nn.Sequential) and len(seq) == 1 and isinstance(seq[0], ldh.BasicBlock)
    assert [seq[0].pool for seq in blocks] == ([True, True, True, False] if cfg.cond_has_mid else [True, True, False])


def test_block_state_dict_names_and_shapes():
    for cin, mid, cout in ((1, 32, 32), (32, 32, 64), (128, 128, 256)):
        want = R.key_shapes(cin, mid, cout)
        assert len(want) == 12
        got = [(k, tuple(v.shape)) for k, v in ldh.BasicBlock(cin, mid, cout).state_dict().items()]
        assert got == list(want.items())
        ldh.BasicBlock(cin, mid, cout, pool=True).load_state_dict(R.make_block(cin, mid, cout))


def test_in_channels_and_exits_follow_the_reference():
    """unet_model.py:94-99 and :116-132: 'mvtecGray' has one channel although 'mvtec' is in its name; 'mnist' and 'mvtecSR'
    have three blocks; any other name is refused with the five named."""
    for data, cin, early in (("mri", 1, False), ("mnist", 1, True), ("mvtec", 3, False), ("mvtecGray", 1, False),
                             ("mvtecSR", 3, True)):
        net = ldh.ResUnet(data)
        assert (net.in_channels, net.early_exit, hasattr(net, "mid_conv")) == (cin, early, not early)
    assert ldh.ResUnet().data == "mri"
    for bad in ("MRI", "cifar", "", None, 3):
        with pytest.raises(ValueError) as e:
            ldh.ResUnet(bad)
        assert all(repr(d) in str(e.value) for d in ("mri", "mnist", "mvtec", "mvtecGray", "mvtecSR"))


@pytest.mark.parametrize("args,match", [((32, 48, 64), "32"), ((32, 32, 48), "32"), ((48, 32, 64), "input_dim"),
                                        ((5, 32, 32), "input_dim"), ((0, 32, 32), "input_dim"), ((32, 0, 64), "32"),
                                        ((32, 32, 0), "32"), ((32, 32, 32), "Identity"), ((64, 32, 64), "Identity"),
                                        ((32.0, 32, 64), "ints"), ((True, 32, 64), "ints")])
def test_constructor_refusals(args, match):
    with pytest.raises(ValueError, match=match):
        ldh.BasicBlock(*args)


def test_modules_refuse_without_touching_a_gpu():
    for mod, c in ((ldh.BasicBlock(32, 32, 64), 32), (ldh.BasicBlock(1, 32, 32), 1), (ldh.BasicBlock(3, 32, 32, pool=True), 3),
                   (ldh.ResUnet("mri"), 1), (ldh.ResUnet("mvtec"), 3), (ldh.ResUnet("mnist"), 1)):
        name = type(mod).__name__
        with pytest.raises(ValueError, match="CPU"):
            mod(torch.zeros(1, c, 8, 8))
        with pytest.raises(ValueError, match="float32"):
            mod(torch.zeros(1, c, 8, 8, dtype=torch.float16))
        with pytest.raises(ValueError, match=name):
            mod(torch.zeros(1, c + 1, 8, 8))
        with pytest.raises(ValueError, match=name):
            mod(torch.zeros(c, 8, 8))
    for bad in ((1, 32, 5, 4), (1, 32, 4, 7)):
        with pytest.raises(ValueError, match="BasicBlock.*even"):
            ldh.BasicBlock(32, 32, 64, pool=True)(torch.zeros(*bad))
    ldh.BasicBlock(32, 32, 64)                                                        # (odd sizes are fine without the pool)
    for data, bad in (("mri", (1, 1, 12, 16)), ("mri", (1, 1, 16, 20)), ("mnist", (1, 1, 6, 8)), ("mvtecSR", (1, 3, 8, 10)),
                      ("mvtec", (1, 3, 28, 32))):
        with pytest.raises(ValueError, match="ResUnet.*divisible"):
            ldh.ResUnet(data)(torch.zeros(*bad))
    for mod in (ldh.BasicBlock(1, 32, 32), ldh.ResUnet("mri")):
        with pytest.raises(ValueError, match="no input gradient"):
            mod(torch.zeros(1, 1, 8, 8, requires_grad=True))


def test_header_declares_and_cabi_binds_the_new_symbols():
    src = open(os.path.join(ROOT, "include", "localdiff_hip.h")).read()
    assert "fifth slice" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = cabi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in the header"
        assert name in cabi.EXPORTS and hasattr(lib, name)
    build_sh = open(os.path.join(ROOT, "localdiffusion-hallucination_amd", "csrc", "build.sh")).read()
    assert "condenc_grad" in build_sh


def test_argument_validation_needs_no_gpu():
    """Every new entry point returns -1 with a message for null pointers, misaligned pointers and bad sizes, before anything
    is launched (the pointers are host memory: a launch would fault)."""
    lib = cabi.lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    p += -p % 16
    err = lib.ld_last_error
    N = None

    def fwd(y=p, ga=p, be=p, y2=N, ga2=N, be2=N, work=p, stat=p, stat2=N, out=p, shape=(1, 4, 4, 32, 64, 16), relu=1):
        return lib.ld_dn_gnr_forward(y, ga, be, y2, ga2, be2, work, stat, stat2, out, *shape, relu, None)

    def bwd(dout=p, act=p, y=p, stat=p, ga=p, y2=N, stat2=N, ga2=N, work=p, dg=p, db=p, dy=p, dg2=N, db2=N, dy2=N,
            shape=(1, 4, 4, 32, 64, 16), relu=1):
        return lib.ld_dn_gnr_backward(dout, act, y, stat, ga, y2, stat2, ga2, work, dg, db, dy, dg2, db2, dy2, *shape, relu, None)

    two = dict(y2=p, ga2=p, be2=p, stat2=p)
    two_b = dict(y2=p, stat2=p, ga2=p, dg2=p, db2=p, dy2=p + 64)
    for k in ("y", "ga", "be", "work", "stat", "out"):
        assert fwd(**{k: N}) == -1 and b"null" in err(), k
    for k in two:                                                                         # the second operand: all or none
        assert fwd(**{**two, k: N}) == -1 and b"null" in err(), k
        assert fwd(**{k: p}) == -1 and b"null" in err(), k
    for k in ("y", "ga", "be", "out"):
        assert fwd(**{k: p + 4}) == -1 and b"aligned" in err(), k
    assert fwd(**{**two, "y2": p + 8}) == -1 and b"aligned" in err()
    assert fwd(work=p + 4) == -1 and b"aligned" in err()
    for k in ("dout", "y", "stat", "ga", "work", "dg", "db", "dy"):
        assert bwd(**{k: N}) == -1 and b"null" in err(), k
    assert bwd(act=N) == -1 and b"null" in err()                                          # relu without the saved result
    for k in two_b:
        assert bwd(**{**two_b, k: N}) == -1 and b"null" in err(), k
        assert bwd(**{k: p}) == -1 and b"null" in err(), k
    for k in ("dout", "act", "y", "ga", "dy"):
        assert bwd(**{k: p + 4}) == -1 and b"aligned" in err(), k
    assert bwd(**{**two_b, "dy2": p + 72}) == -1 and b"aligned" in err()
    assert bwd(**{**two_b, "dy2": p}) == -1 and b"of its own" in err()                    # dy2 may alias neither dy nor dout
    bad_shapes = ((0, 4, 4, 32, 64, 16), (1, 0, 4, 32, 64, 16), (1, 4, -1, 32, 64, 16), (1, 4, 4, 0, 64, 16),
                  (1, 4, 4, 32, 64, 0), (1, 4, 4, 48, 64, 16),      # 3 channels per group
                  (1, 4, 4, 16, 64, 16),                             # 1 channel per group
                  (1, 4, 4, 6, 64, 3),                               # 2 per group, but C no multiple of 4
                  (1, 4, 4, 40, 64, 16),                             # groups does not divide C
                  (1, 4, 4, 64, 32, 16), (1, 4, 4, 32, 62, 16), (1, 4, 4, 2048 + 32, 4096, 16), (1, 4, 4, 32, 4096 + 64, 16),
                  (32768, 4, 4, 32, 64, 16), (1 << 30, 1 << 20, 1 << 20, 32, 64, 16), (1, 1 << 20, 1 << 20, 32, 64, 16),
                  (1, (1 << 20) + 1, 1, 32, 64, 16))
    for shape in bad_shapes:
        assert fwd(shape=shape) == -1 and b"groups=" in err(), shape
        assert bwd(shape=shape) == -1 and b"groups=" in err(), shape
    for bad in ((0, 4, 4, 32, 16), (1, 4, 4, 48, 16), (1, 4, 4, 16, 16), (1, 4, 4, 6, 3), (1, 4, 4, 2048 + 32, 16),
                (32768, 4, 4, 32, 16), (1 << 30, 1 << 20, 1 << 20, 32, 16)):
        assert int(lib.ld_dn_gnr_work_bytes(*bad)) == 0, bad
    for good in ((2, 5, 6, 32, 16), (1, 12, 12, 256, 16), (1, 40, 40, 32, 16), (8, 256, 256, 32, 16)):
        assert int(lib.ld_dn_gnr_work_bytes(*good)) > 0
    im = lib.ld_dn_im2col3
    assert im(None, p, 1, 1, 4, 4, 16, 16, 4, 1, 64, None) == -1 and b"null" in err()
    assert im(p, None, 1, 1, 4, 4, 16, 16, 4, 1, 64, None) == -1 and b"null" in err()
    assert im(p, p + 4, 1, 1, 4, 4, 16, 16, 4, 1, 64, None) == -1 and b"aligned" in err()
    assert im(p, p, 1, 5, 4, 4, 80, 16, 4, 1, 64, None) == -1 and b"Cin" in err()
    assert im(p, p, 1, 0, 4, 4, 16, 16, 4, 1, 64, None) == -1
    assert im(p, p, 1, 3, 4, 4, 48, 16, 4, 1, 24, None) == -1                               # ldk < 27
    assert im(p, p, 1, 1, 4, 4, 16, 16, 4, 1, 50, None) == -1                               # ldk no multiple of 4
    assert im(p, p, 1, 1, 4, 4, 16, 16, -4, 1, 64, None) == -1 and b"stride" in err()
    assert im(p, p, 0, 1, 4, 4, 16, 16, 4, 1, 64, None) == -1
    assert im(p, p, 1 << 30, 1, 1 << 20, 1 << 20, 16, 16, 4, 1, 64, None) == -1
    assert im(p, p, 1, 1, 4, 4, 16, 16, 4, 1, 4096 + 64, None) == -1
    assert all(v == 0.0 for v in buf)                                                       # nothing was written


def test_work_bytes_cover_both_passes():
    """[2][B][runs][C][2] doubles for the forward's statistics, [B][runs][C][3] + [B][C][3] + [2][B][16][2] for the backward;
    30 pixels are two runs of at most 16, 1,600 pixels at B = 1, C = 32 are 100 runs of 16."""
    lib = cabi.lib()
    backward = 2 * 2 * 32 * 3 + 2 * 32 * 3 + 2 * 2 * 16 * 2
    assert int(lib.ld_dn_gnr_work_bytes(2, 5, 6, 32, 16)) == 8 * max(2 * 2 * 2 * 32 * 2, backward)
    assert int(lib.ld_dn_gnr_work_bytes(1, 40, 40, 32, 16)) == 8 * 2 * 100 * 32 * 2


def test_the_restatement_is_the_oracles_encoder():
    """A check of the yardstick, not of the feature's kernels: condenc_ref's forward equals oracle.unet_ref.cond_encoder bit
    for bit on the same weights and input, for the three configs, and a block equals oracle.unet_ref.basic_block; the 1x1
    convolution over im2col3's columns with the OIHW weight as it lies in memory is the 3x3 convolution."""
    for data, B, H, W in R.ENCODER_CASES:
        sd, x = R.encoder_state(data), R.encoder_input(data, B, H, W, 3)
        full = {"cond_model." + k: v for k, v in sd.items()}
        with torch.no_grad():
            assert torch.equal(R.encoder(sd, x, data), unet_ref.cond_encoder(full, x, data))
            sd64, full64 = {k: v.double() for k, v in sd.items()}, {k: v.double() for k, v in full.items()}
            assert torch.equal(R.encoder(sd64, x.double(), data), unet_ref.cond_encoder(full64, x.double(), data))
    sd, x = R.make_block(32, 32, 64, key=1), R.uniform((2, 32, 6, 6), 5)
    with torch.no_grad():
        want = unet_ref.basic_block({"b." + k: v for k, v in sd.items()}, "b", x)
        assert torch.equal(R.basic_block(sd, x), want) and torch.equal(R.basic_block(sd, x, pool=True), F.max_pool2d(want, 2))
    img, w = R.uniform((2, 3, 5, 7), 4).double(), R.uniform((32, 3, 3, 3), 5).double()
    cols = R.im2col3(img, 64)
    assert bool((cols[..., 27:] == 0).all())
    out = (cols[..., :27] @ w.reshape(32, 27).t()).permute(0, 3, 1, 2)
    assert R.rel_err(out, F.conv2d(img, w, padding=1)) < 1e-14


def test_margin_report_sees_a_relu_at_zero_and_a_tied_window():
    a = torch.tensor([[[[1.0, -2.0], [0.5, 4.0]]]])
    m = {}
    R.relu(a, m)
    R.max_pool(a, m)
    assert m == {"relu": [0.125], "pool": [0.75]}
    m = {}
    R.max_pool(torch.tensor([[[[3.0, 3.0], [0.0, 1.0]]]]), m)
    R.max_pool(torch.zeros(1, 1, 2, 2), m)                                             # a window of zeros is not counted
    assert m["pool"] == [0.0, float("inf")]


# ------------------------------------------------------------------------------------------------ the margin condition
def check_margins(m, what, kinds):
    print(f"{what}: " + ", ".join(f"{k} margin {v:.2e}" for k, v in m.items()))
    assert set(m) == set(kinds), (what, m)
    assert all(v >= R.MARGIN for v in m.values()), (what, m)


@pytest.mark.parametrize("case", sorted({(C, B, H, W) for C, _, B, H, W in R.GN_CASES}))
def test_margin_condition_of_the_groupnorm_cases(case):
    for nop in (1, 2):
        t, dout = R.gn_inputs(*case, nop, R.GN_KEYS[case + (nop,)])
        check_margins(R.gn_yardstick(t, dout, True, F64)[2], f"gn {case} operands {nop}", ("relu",))


@pytest.mark.parametrize("case", R.BLOCK_CASES)
def test_margin_condition_of_the_block_cases(case):
    sd, x, dout = R.block_inputs(case, R.BLOCK_KEYS[case])
    m = R.yardstick(sd, x, dout, F64, pool=case[3], x_grad=case[0] > 4)[2]
    check_margins(m, f"block {case}", ("relu", "pool") if case[3] else ("relu",))


@pytest.mark.parametrize("case", R.ENCODER_CASES)
def test_margin_condition_of_the_encoder_cases(case):
    sd, x, dout = R.encoder_inputs(case, R.ENCODER_KEYS[case])
    check_margins(R.yardstick(sd, x, dout, F64, data=case[0], x_grad=False)[2], f"encoder {case}", ("relu", "pool"))


def test_margin_condition_of_the_chain_case():
    check_margins(R.chain_yardstick(*R.chain_inputs(R.CHAIN_KEYS["chain"]), F64)[2], "chain", ("relu", "pool"))
