"""CPU-side checks of the time MLP and the trainable Unet (no GPU needed): the yardstick is the oracle, the state_dict is the
reference's in names, shapes and order, the inference Unet's weights load in both directions, the refusals, and the C ABI's
declarations, bindings and argument checks."""
import ctypes as C
import os
import re

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import weights
from oracle import unet_ref

import unet_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ld_dn_time_mlp_forward", "ld_dn_time_mlp_work_bytes", "ld_dn_time_mlp_backward", "ld_dn_join"]
F32, F64 = torch.float32, torch.float64


def test_public_surface():
    assert "TimeMLP" in ldh.__all__ and "TrainableUnet" in ldh.__all__
    assert ldh.TimeMLP.__module__.endswith(".unet_grad") and ldh.TrainableUnet.__module__.endswith(".unet_grad")


@pytest.mark.parametrize("case", R.CASES)
def test_restatement_in_fp32_is_the_oracle_bit_for_bit(case):
    """unet_grad_ref.unet_forward in fp32 equals oracle.unet_ref.unet_forward at the three cases of the GPU tests, and its fp64
    run agrees with it to fp32 rounding (the output's own d is below 1e-6)."""
    sd, x, cond, time, _ = R.inputs(case)
    cfg = R.CONFIGS[case[0]]
    with torch.no_grad():
        want = unet_ref.unet_forward(sd, cfg, x, cond, time)
        got = R.unet_forward(sd, cfg, x, cond, time)
        sd64 = {k: v.double() for k, v in sd.items()}
        o64 = R.unet_forward(sd64, cfg, x.double(), cond.double(), time, F64)
    assert torch.equal(got, want)
    d = R.rel_err(got, o64)
    print(f"{case}: fp32 restatement to fp64 {d:.2e}")
    assert o64.dtype == F64 and d < 1e-5


def test_fp64_angle_is_double_t_times_the_fp32_table():
    f = R.freqs(32)
    assert f.dtype == F32
    sd = {k[len("time_mlp."):]: v.double() for k, v in R.state("mnist").items() if k.startswith("time_mlp.")}
    parts = {}
    R.time_mlp(sd, torch.tensor([999, 0]), 32, F64, p="", parts=parts)
    want = torch.tensor([999.0, 0.0], dtype=F64)[:, None] * f.double()[None, :]
    assert torch.equal(parts["emb"], torch.cat([want.sin(), want.cos()], dim=-1))


@pytest.mark.parametrize("data", list(R.KWARGS))
def test_state_dict_is_the_references_in_names_shapes_and_order(data):
    net = ldh.TrainableUnet(dim=32, init_dim=32, **R.KWARGS[data])
    want = weights.unet_param_shapes(net.cfg)
    got = net.state_dict()
    assert net.cfg == R.CONFIGS[data]
    assert list(got) == list(want)
    assert {k: tuple(v.shape) for k, v in got.items()} == dict(want)
    assert [k for k, _ in net.named_parameters()] == list(want)            # every entry trains; the frequency table is no entry
    assert all(p.requires_grad for p in net.parameters())
    # the inference Unet and a reference checkpoint load into it and back
    inf = ldh.Unet(dim=32, init_dim=32, **R.KWARGS[data])
    sd = R.state(data)
    net.load_state_dict(sd)
    inf.load_state_dict(net.state_dict())
    for k, v in inf.state_dict().items():
        assert torch.equal(v, sd[k]), k
    net.load_state_dict(inf.state_dict())
    assert net.downsample_factor == inf.downsample_factor and net.out_dim == inf.out_dim and net.channels == inf.channels


def test_time_mlp_keys_and_buffer():
    mlp = ldh.TimeMLP(32)
    assert list(mlp.state_dict()) == ["1.weight", "1.bias", "3.weight", "3.bias"]
    assert {k: tuple(v.shape) for k, v in mlp.state_dict().items()} == {"1.weight": (128, 32), "1.bias": (128,),
                                                                         "3.weight": (128, 128), "3.bias": (128,)}
    assert torch.equal(mlp.freqs, R.freqs(32)) and "freqs" not in mlp.state_dict()
    assert torch.equal(ldh.TimeMLP(64, theta=100).freqs, R.freqs(64, 100))
    for dim in (0, 2, 7, 3.0):
        with pytest.raises(ValueError, match="TimeMLP"):
            ldh.TimeMLP(dim)


def test_debug_fill_reaches_every_sub_module():
    net = ldh.TrainableUnet(dim=32, **R.KWARGS["mnist"])
    net.debug_fill = 1.5
    owners = [m for m in net.modules() if m is not net and hasattr(type(m), "debug_fill")]
    kinds = {type(m).__name__ for m in owners}
    assert kinds == {"Conv2d", "TimeMLP", "ResnetBlock", "LinearAttention", "Attention", "Downsample", "Upsample", "BasicBlock"}
    assert all(m.debug_fill == 1.5 for m in owners) and net.debug_fill == 1.5
    net.debug_fill = None
    assert all(m.debug_fill is None for m in owners)


@pytest.mark.parametrize("kw,match", [
    (dict(self_condition=True), "self_condition"), (dict(learned_variance=True), "learned_variance"),
    (dict(learned_sinusoidal_cond=True), "learned_sinusoidal_cond"), (dict(random_fourier_features=True), "random_fourier"),
    (dict(attn_dim_head=64), "attn_dim_head"), (dict(dim=48), "multiple of 32"), (dict(dim=32, init_dim=64), "init_dim"),
    (dict(dim=64), "condition encoder"), (dict(dim_mults=(1, 2, 4), full_attn=False), "condition encoder"),
    (dict(full_attn=(False, True)), "full_attn"), (dict(mode="ct"), "ResUnet"), (dict(resnet_block_groups=16), "groups")])
def test_constructor_refuses(kw, match):
    args = dict(dim=32)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        ldh.TrainableUnet(**args)


def test_forward_refuses_without_touching_a_gpu():
    net = ldh.TrainableUnet(dim=32, **R.KWARGS["mri"])
    x, cond, t = torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16), torch.zeros(1, dtype=torch.long)
    with pytest.raises(ValueError, match="CPU"):
        net(x, cond, t)
    for bad in (torch.zeros(1, 1, 12, 16), torch.zeros(1, 1, 16, 20)):
        with pytest.raises(ValueError, match="divisible by 8"):
            net(bad, bad.clone(), t)
    with pytest.raises(ValueError, match="float32"):
        net(x.half(), cond, t)
    with pytest.raises(ValueError, match="float32"):
        net(x, cond.double(), t)
    with pytest.raises(ValueError, match="x is data"):
        net(x.clone().requires_grad_(True), cond, t)
    with pytest.raises(ValueError, match="cond_img is data"):
        net(x, cond.clone().requires_grad_(True), t)
    with pytest.raises(ValueError, match="x must be"):
        net(torch.zeros(1, 3, 16, 16), cond, t)
    with pytest.raises(ValueError, match="cond_img must be"):
        net(x, torch.zeros(1, 3, 16, 16), t)
    with pytest.raises(ValueError, match="differ"):
        net(x, torch.zeros(2, 1, 16, 16), t)
    with pytest.raises(ValueError, match="time must be"):
        net(x, cond, torch.zeros(2, dtype=torch.long))
    mlp = ldh.TimeMLP(32)
    with pytest.raises(ValueError, match="CPU"):
        mlp(t)
    with pytest.raises(ValueError, match="int32, int64 and float32"):
        mlp(torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError, match="no gradient"):
        mlp(torch.zeros(1, requires_grad=True))
    with pytest.raises(ValueError, match=r"\[B\]"):
        mlp(torch.zeros(1, 1))


def test_header_declares_and_cabi_binds_the_new_symbols():
    src = open(os.path.join(ROOT, "include", "localdiff_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = cabi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in the header"
        assert name in cabi.EXPORTS and hasattr(lib, name)
    build = open(os.path.join(ROOT, "localdiffusion-hallucination_amd", "csrc", "build.sh")).read()
    assert "unet_grad" in build


def test_argument_validation_needs_no_gpu():
    """Null or misaligned pointers and sizes that are refused return -1 before any launch."""
    lib = cabi.lib()
    buf = (C.c_double * 64)()
    p, N = C.addressof(buf), None
    p = (p + 15) // 16 * 16
    ok = (2, 32, 128)
    assert lib.ld_dn_time_mlp_forward(p, p, p, p, p, p, p, p, N, *ok, N) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_time_mlp_forward(p, p + 2, p, p, p, p, p, p, p, *ok, N) == -1 and b"aligned" in lib.ld_last_error()
    for B, dim, T in ((0, 32, 128), (2, 2, 128), (2, 31, 128), (2, 32, 126), (2, 32, 0), (2, 8192, 8192), (2, 4, 65536)):
        assert lib.ld_dn_time_mlp_forward(p, p, p, p, p, p, p, p, p, B, dim, T, N) == -1, (B, dim, T)
        assert lib.ld_dn_time_mlp_backward(p, p, p, p, p, p, p, p, p, B, dim, T, N) == -1, (B, dim, T)
        assert int(lib.ld_dn_time_mlp_work_bytes(B, dim, T)) == 0
    assert int(lib.ld_dn_time_mlp_work_bytes(3, 32, 128)) == 2 * 3 * 128 * 4
    assert lib.ld_dn_time_mlp_backward(p, p, p, p, N, p, p, p, p, *ok, N) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_time_mlp_backward(p, p, p, p, p, p, p + 1, p, p, *ok, N) == -1 and b"aligned" in lib.ld_last_error()
    shape = (2, 5, 3)
    assert lib.ld_dn_join(N, N, p, p + 16, *shape, 32, 64, 32, 64, 64, N) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_join(p, N, N, p + 16, *shape, 32, 64, 0, 0, 64, N) == -1 and b"nothing" in lib.ld_last_error()
    assert lib.ld_dn_join(p, N, p, p + 16, *shape, 32, 64, 0, 64, 64, N) == -1 and b"together" in lib.ld_last_error()
    assert lib.ld_dn_join(p, N, N, p + 16, *shape, 32, 64, 32, 64, 64, N) == -1 and b"together" in lib.ld_last_error()
    assert lib.ld_dn_join(p, N, p, p + 8, *shape, 32, 64, 32, 64, 64, N) == -1 and b"aligned" in lib.ld_last_error()
    assert lib.ld_dn_join(p, p + 4, N, p + 16, *shape, 32, 64, 0, 0, 64, N) == -1 and b"aligned" in lib.ld_last_error()
    assert lib.ld_dn_join(p, N, p, p, *shape, 32, 64, 32, 64, 64, N) == -1 and b"inputs" in lib.ld_last_error()
    for ca, lda, cb, ldb, ldo in ((16, 64, 32, 64, 64), (32, 64, 48, 64, 128), (64, 32, 32, 64, 128), (32, 64, 32, 16, 64),
                                  (32, 64, 32, 64, 32), (32, 66, 32, 64, 64), (32, 64, 32, 64, 66), (0, 64, 32, 64, 64)):
        assert lib.ld_dn_join(p, N, p + 16, p + 32, *shape, ca, lda, cb, ldb, ldo, N) == -1, (ca, lda, cb, ldb, ldo)
    assert lib.ld_dn_join(p, N, p + 16, p + 32, 0, 5, 3, 32, 64, 32, 64, 64, N) == -1
    big = 1 << 20
    assert lib.ld_dn_join(p, N, p + 16, p + 32, 32767, big, big, 32, 64, 32, 64, 64, N) == -1 and b"pixels" in lib.ld_last_error()
