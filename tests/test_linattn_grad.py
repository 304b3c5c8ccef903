"""CPU-side checks of the trainable LinearAttention (no GPU needed): the public surface, the reference's state_dict names
and shapes, the limits, the C ABI's declarations and bindings, and the yardstick the GPU tests compare with."""
import ctypes as C
import os
import re

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from oracle import unet_ref

import linattn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ld_dn_rms_work_bytes", "ld_dn_rms_forward", "ld_dn_rms_backward", "ld_dn_la_splits", "ld_dn_la_work_bytes",
               "ld_dn_la_context", "ld_dn_la_out", "ld_dn_la_backward_reduce", "ld_dn_la_backward_apply"]


def test_public_surface():
    assert "LinearAttention" in ldh.__all__
    assert ldh.LinearAttention.__module__.endswith(".linattn_grad")


@pytest.mark.parametrize("dim,heads", [(32, 1), (64, 4), (96, 2)])
def test_state_dict_names_and_shapes(dim, heads):
    mod = ldh.LinearAttention(dim, heads=heads)
    want = R.key_shapes(dim, heads)
    got = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    assert list(got) == list(want) and got == dict(want)
    assert bool((mod.norm.g == 1).all()) and bool((mod.to_out[1].g == 1).all())      # the reference's initialisation
    mod.load_state_dict(R.make_attn(dim, heads))                                    # a slice of a checkpoint loads by name
    assert torch.equal(mod.state_dict()["to_out.0.bias"], R.make_attn(dim, heads)["to_out.0.bias"])


def test_constructor_refuses():
    with pytest.raises(ValueError, match="multiple of 32"):
        ldh.LinearAttention(48)
    with pytest.raises(ValueError, match="dim_head = 32"):
        ldh.LinearAttention(64, dim_head=64)
    with pytest.raises(ValueError, match="heads"):
        ldh.LinearAttention(64, heads=0)


def test_module_refuses_without_touching_a_gpu():
    mod = ldh.LinearAttention(32, heads=1)
    with pytest.raises(ValueError, match="CPU"):
        mod(torch.zeros(1, 32, 4, 4))
    with pytest.raises(ValueError, match="float32"):
        mod(torch.zeros(1, 32, 4, 4, dtype=torch.float16))
    with pytest.raises(ValueError, match="32"):
        mod(torch.zeros(1, 16, 4, 4))


def test_header_declares_and_cabi_binds_the_new_symbols():
    src = open(os.path.join(ROOT, "include", "localdiff_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = cabi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in the header"
        assert name in cabi.EXPORTS and hasattr(lib, name)
    build = open(os.path.join(ROOT, "localdiffusion-hallucination_amd", "csrc", "build.sh")).read()
    assert "linattn_grad" in build


def test_argument_validation_needs_no_gpu():
    lib = cabi.lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)

    def refused(rc, word):
        return rc == -1 and word in lib.ld_last_error()

    # RMSNorm: null pointer; ldc < C; C not a multiple of 4
    assert refused(lib.ld_dn_rms_forward(None, None, None, None, 1, 4, 4, 32, 32, None), b"null")
    assert refused(lib.ld_dn_rms_forward(p, p, None, p, 1, 4, 4, 32, 16, None), b"ldc")
    assert refused(lib.ld_dn_rms_forward(p, p, None, p, 1, 4, 4, 30, 32, None), b"ldc")
    assert refused(lib.ld_dn_rms_backward(p, p, p, p, None, p, p, 1, 4, 4, 32, 32, None), b"null")
    assert refused(lib.ld_dn_rms_backward(p, p, p, None, p, p, p, 1, 4, 4, 32, 32, None), b"null")      # the saved 1 / norm
    assert refused(lib.ld_dn_rms_backward(p, p, p, p, p, p, p, 1, 4, 4, 32, 16, None), b"ldc")
    assert refused(lib.ld_dn_rms_backward(p, p, p, p, p, p, p, 1, 4, 4, 30, 32, None), b"ldc")
    assert int(lib.ld_dn_rms_work_bytes(1, 4, 4, 30)) == 0 and int(lib.ld_dn_rms_work_bytes(0, 4, 4, 32)) == 0
    assert int(lib.ld_dn_rms_work_bytes(2, 16, 16, 64)) > 0
    # the attention core: null pointer; heads < 1; a pixel stride below the channels; a stride that is no multiple of 4
    assert refused(lib.ld_dn_la_context(None, None, None, None, 1, 4, 4, 1, 128, None), b"null")
    assert refused(lib.ld_dn_la_context(p, p, p, p, 1, 4, 4, 0, 128, None), b"heads")
    assert refused(lib.ld_dn_la_context(p, p, p, p, 1, 4, 4, 2, 128, None), b"ld3")
    assert refused(lib.ld_dn_la_out(None, None, None, 1, 4, 4, 1, 128, 64, None), b"null")
    assert refused(lib.ld_dn_la_out(p, p, p, 1, 4, 4, 0, 128, 64, None), b"heads")
    assert refused(lib.ld_dn_la_out(p, p, p, 1, 4, 4, 1, 128, 16, None), b"ldo")
    assert refused(lib.ld_dn_la_out(p, p, p, 1, 4, 4, 1, 98, 64, None), b"ld3")
    assert refused(lib.ld_dn_la_backward_reduce(p, p, p, None, p, p, 1, 4, 4, 1, 128, 64, None), b"null")
    assert refused(lib.ld_dn_la_backward_reduce(p, p, p, p, p, p, 1, 4, 4, -1, 128, 64, None), b"heads")
    assert refused(lib.ld_dn_la_backward_reduce(p, p, p, p, p, p, 1, 4, 4, 2, 128, 64, None), b"ld3")
    assert refused(lib.ld_dn_la_backward_apply(p, p, p, p, p, p, None, 1, 4, 4, 1, 128, 64, None), b"null")
    assert refused(lib.ld_dn_la_backward_apply(p, p, p, p, p, p, p, 1, 4, 4, 0, 128, 64, None), b"heads")
    assert refused(lib.ld_dn_la_backward_apply(p, p, p, p, p, p, p, 1, 0, 4, 1, 128, 64, None), b"H=0")
    assert int(lib.ld_dn_la_splits(1, 0, 4, 4)) == 0 and int(lib.ld_dn_la_work_bytes(1, 0, 4, 4)) == 0
    assert int(lib.ld_dn_la_work_bytes(1, 4, 0, 4)) == 0
    assert int(lib.ld_dn_la_splits(2, 4, 16, 16)) >= 1 and int(lib.ld_dn_la_work_bytes(2, 4, 16, 16)) > 0
    # the split depends on the shape alone
    assert int(lib.ld_dn_la_splits(1, 2, 33, 31)) == int(lib.ld_dn_la_splits(1, 2, 33, 31)) >= 2


@pytest.mark.parametrize("dim,heads", [(32, 1), (64, 4)])
def test_yardstick_forward_is_the_oracle(dim, heads):
    sd = R.make_attn(dim, heads, key=3)
    x = R.uniform((2, dim, 6, 5), 1)
    full = {"p." + k: v for k, v in sd.items()}
    with torch.no_grad():
        want = unet_ref.linear_attention(full, "p", x, heads, 32)
        assert torch.equal(R.forward(sd, x, heads), want)
    dout = R.uniform(want.shape, 3)
    out32, g32 = R.yardstick(sd, x, dout, heads, dtype=torch.float32)
    out64, g64 = R.yardstick(sd, x, dout, heads, dtype=torch.float64)
    assert torch.equal(out32, want)
    assert set(g64) == {"x"} | set(sd)
    for k in g64:
        assert g64[k].shape == (x.shape if k == "x" else sd[k].shape)
        assert R.rel_err(g32[k], g64[k]) < 1e-5, k


def test_core_formulas_are_the_oracle():
    """linattn_ref.core, which the per-kernel GPU tests compare with, is the oracle's attention between to_qkv and to_out."""
    dim, heads = 32, 2
    sd = R.make_attn(dim, heads, key=4)
    x = R.uniform((2, dim, 5, 4), 7).double()
    full = {"p." + k: v.double() for k, v in sd.items()}
    qkv = torch.nn.functional.conv2d(unet_ref.rms_norm(x, full["p.norm.g"]), full["p.to_qkv.weight"])
    att = R.core(qkv, heads, None, torch.float64)["out"]
    y = torch.nn.functional.conv2d(att, full["p.to_out.0.weight"], full["p.to_out.0.bias"])
    assert torch.equal(unet_ref.rms_norm(y, full["p.to_out.1.g"]), unet_ref.linear_attention(full, "p", x, heads, 32))
