"""CPU-side checks of the trainable full Attention (no GPU needed): the public surface, the reference's state_dict names and
shapes, the limits, the C ABI's declarations and bindings, and the yardstick the GPU tests compare with."""
import ctypes as C
import os
import re

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from oracle import unet_ref

import attention_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ld_dn_fa_forward", "ld_dn_fa_work_bytes", "ld_dn_fa_backward"]


def test_public_surface():
    assert "Attention" in ldh.__all__
    assert ldh.Attention.__module__.endswith(".attention_grad")


@pytest.mark.parametrize("dim,heads", [(32, 1), (64, 4), (96, 2)])
def test_state_dict_names_and_shapes(dim, heads):
    mod = ldh.Attention(dim, heads=heads)
    want = R.key_shapes(dim, heads)
    assert list(want) == ["norm.g", "to_qkv.weight", "to_out.weight", "to_out.bias"]     # no RMSNorm behind to_out
    got = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    assert list(got) == list(want) and got == dict(want)
    assert bool((mod.norm.g == 1).all())                                            # the reference's initialisation
    mod.load_state_dict(R.make_attn(dim, heads))                                    # a slice of a checkpoint loads by name
    assert torch.equal(mod.state_dict()["to_out.bias"], R.make_attn(dim, heads)["to_out.bias"])


def test_constructor_refuses():
    with pytest.raises(ValueError, match="multiple of 32"):
        ldh.Attention(48)
    with pytest.raises(ValueError, match="multiple of 32"):
        ldh.Attention(0)
    with pytest.raises(ValueError, match="dim_head = 32"):
        ldh.Attention(64, dim_head=64)
    with pytest.raises(ValueError, match="heads"):
        ldh.Attention(64, heads=0)


def test_module_refuses_without_touching_a_gpu():
    mod = ldh.Attention(32, heads=1)
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
    assert re.search(r"\battention_grad\b", build)


def test_argument_validation_needs_no_gpu():
    lib = cabi.lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    assert p % 16 == 0

    def refused(rc, word):
        return rc == -1 and word in lib.ld_last_error()

    fwd, bwd = lib.ld_dn_fa_forward, lib.ld_dn_fa_backward
    # forward: null pointers (lse alone may be null); a misaligned pointer; heads < 1; the strides; an empty map
    assert refused(fwd(None, None, None, 1, 4, 4, 1, 128, 64, None), b"null")
    assert refused(fwd(p, None, None, 1, 4, 4, 1, 128, 64, None), b"null")
    assert refused(fwd(p + 4, p, None, 1, 4, 4, 1, 128, 64, None), b"aligned")
    assert refused(fwd(p, p + 8, None, 1, 4, 4, 1, 128, 64, None), b"aligned")
    assert refused(fwd(p, p, None, 1, 4, 4, 0, 128, 64, None), b"heads")
    assert refused(fwd(p, p, None, 1, 4, 4, 2, 128, 64, None), b"ld3")            # ld3 < 192
    assert refused(fwd(p, p, None, 1, 4, 4, 1, 98, 64, None), b"ld3")             # no multiple of 4
    assert refused(fwd(p, p, None, 1, 4, 4, 1, 128, 16, None), b"ldo")            # ldo < 32
    assert refused(fwd(p, p, None, 1, 4, 4, 1, 128, 34, None), b"ldo")
    assert refused(fwd(p, p, None, 1, 0, 4, 1, 128, 64, None), b"H=0")
    assert refused(fwd(p, p, None, 1, 4, 0, 1, 128, 64, None), b"W=0")
    assert refused(fwd(p, p, None, 0, 4, 4, 1, 128, 64, None), b"B=0")
    # backward: every pointer is needed
    for i in range(6):
        ptrs = [p] * 6
        ptrs[i] = None
        assert refused(bwd(*ptrs, 1, 4, 4, 1, 128, 64, None), b"null"), i
    for i in (0, 1, 2, 5):
        ptrs = [p] * 6
        ptrs[i] = p + 4
        assert refused(bwd(*ptrs, 1, 4, 4, 1, 128, 64, None), b"aligned"), i
    assert refused(bwd(p, p, p, p, p, p, 1, 4, 4, -1, 128, 64, None), b"heads")
    assert refused(bwd(p, p, p, p, p, p, 1, 4, 4, 2, 128, 64, None), b"ld3")
    assert refused(bwd(p, p, p, p, p, p, 1, 4, 4, 1, 128, 30, None), b"ldo")
    assert refused(bwd(p, p, p, p, p, p, 1, 0, 4, 1, 128, 64, None), b"H=0")
    # the scratch: delta [B, heads, n] floats; 0 for a shape the backward refuses
    assert int(lib.ld_dn_fa_work_bytes(1, 0, 4, 4)) == 0 and int(lib.ld_dn_fa_work_bytes(1, 4, 0, 4)) == 0
    assert int(lib.ld_dn_fa_work_bytes(0, 4, 4, 4)) == 0 and int(lib.ld_dn_fa_work_bytes(1, 4, 4, -1)) == 0
    assert int(lib.ld_dn_fa_work_bytes(2, 4, 16, 16)) == 2 * 4 * 256 * 4
    assert int(lib.ld_dn_fa_work_bytes(1, 1, 5, 3)) == 64                          # 15 floats, rounded up to 8 bytes
    assert all(v == 0.0 for v in buf)


@pytest.mark.parametrize("dim,heads", [(32, 1), (64, 4)])
def test_yardstick_forward_is_the_oracle(dim, heads):
    sd = R.make_attn(dim, heads, key=3)
    x = R.uniform((2, dim, 6, 5), 1)
    full = {"p." + k: v for k, v in sd.items()}
    with torch.no_grad():
        want = unet_ref.full_attention(full, "p", x, heads, 32)
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
    """attention_ref.core, which the per-kernel GPU tests compare with, composed with the oracle's norm and convolutions is
    the oracle's full_attention bit for bit in fp64; its lse is the log of the softmax's normaliser."""
    dim, heads = 32, 2
    sd = R.make_attn(dim, heads, key=4)
    x = R.uniform((2, dim, 5, 4), 7).double()
    full = {"p." + k: v.double() for k, v in sd.items()}
    qkv = torch.nn.functional.conv2d(unet_ref.rms_norm(x, full["p.norm.g"]), full["p.to_qkv.weight"])
    res = R.core(qkv, heads, None, torch.float64)
    y = torch.nn.functional.conv2d(res["out"], full["p.to_out.weight"], full["p.to_out.bias"])
    assert torch.equal(y, unet_ref.full_attention(full, "p", x, heads, 32))
    q, k, _ = [t.reshape(2, heads, 32, 20) for t in qkv.chunk(3, dim=1)]
    sim = torch.einsum("bhdi,bhdj->bhij", q, k) * 32 ** -0.5
    assert res["lse"].shape == (2, heads, 20)
    assert torch.allclose(res["lse"], sim.exp().sum(dim=-1).log(), rtol=1e-12, atol=1e-12)
    dout = R.uniform((2, heads * 32, 5, 4), 9)
    assert R.core(qkv, heads, dout, torch.float64)["dqkv"].shape == qkv.shape
