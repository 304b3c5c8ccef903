"""CPU-side checks of the trainable ResnetBlock (no GPU needed): the public surface, the reference's state_dict names and
shapes, the constructor's limits, the C ABI's declarations and bindings, and the yardstick the GPU tests compare with."""
import ctypes as C
import os
import re

import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from oracle import unet_ref

import resblock_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ld_p_losses_grad", "ld_dn_gn_work_bytes", "ld_dn_gn_forward", "ld_dn_gn_backward", "ld_dn_colsum",
               "ld_dn_time_proj", "ld_dn_time_proj_backward", "ld_dn_pack_nhwc", "ld_dn_gather3"]


def test_public_surface():
    assert "ResnetBlock" in ldh.__all__
    assert ldh.ResnetBlock.__module__.endswith(".resblock")
    assert callable(ldh.GaussianDiffusion.p_losses_grad)


@pytest.mark.parametrize("dim,dim_out,tdim", [(32, 64, 128), (64, 64, 128), (128, 64, None)])
def test_state_dict_names_and_shapes(dim, dim_out, tdim):
    blk = ldh.ResnetBlock(dim, dim_out, time_emb_dim=tdim)
    want = resblock_ref.key_shapes(dim, dim_out, tdim)
    got = {k: tuple(v.shape) for k, v in blk.state_dict().items()}
    assert list(got) == list(want) and got == dict(want)
    assert any(k.startswith("res_conv.") for k in got) == (dim != dim_out)
    assert any(k.startswith("mlp.") for k in got) == (tdim is not None)
    blk.load_state_dict(resblock_ref.make_block(dim, dim_out, tdim))           # a slice of a checkpoint loads by name


@pytest.mark.parametrize("kw", [dict(dim=48, dim_out=64), dict(dim=64, dim_out=48), dict(dim=64, dim_out=64, groups=5),
                                dict(dim=32, dim_out=32, groups=16)])
def test_constructor_refuses(kw):
    args = dict(kw)
    with pytest.raises(ValueError, match="multiple|divide"):
        ldh.ResnetBlock(args.pop("dim"), args.pop("dim_out"), time_emb_dim=64, **args)


def test_module_refuses_without_touching_a_gpu():
    blk = ldh.ResnetBlock(32, 32)
    with pytest.raises(ValueError, match="CPU"):
        blk(torch.zeros(1, 32, 4, 4))
    with pytest.raises(ValueError, match="float32"):
        blk(torch.zeros(1, 32, 4, 4, dtype=torch.float16))
    with pytest.raises(ValueError, match="32"):
        blk(torch.zeros(1, 16, 4, 4))


def test_header_declares_and_cabi_binds_the_new_symbols():
    src = open(os.path.join(ROOT, "include", "localdiff_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = cabi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in the header"
        assert name in cabi.EXPORTS and hasattr(lib, name)
    build = open(os.path.join(ROOT, "localdiffusion-hallucination_amd", "csrc", "build.sh")).read()
    assert "denoiser_grad" in build


def test_argument_validation_needs_no_gpu():
    lib = cabi.lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    assert lib.ld_p_losses_grad(None, None, None, None, None, None, None, 1.0, None, 1, 4, 0, None) == -1
    assert b"null" in lib.ld_last_error()
    assert lib.ld_p_losses_grad(p, p, p, p, p, p, p, 1.0, p, 1, 4, 7, None) == -1 and b"objective" in lib.ld_last_error()
    assert lib.ld_dn_gn_forward(None, None, None, None, None, None, None, None, 1, 4, 4, 32, 32, 8, None) == -1
    assert b"null" in lib.ld_last_error()
    # C must be a multiple of 4 * groups
    assert lib.ld_dn_gn_forward(p, p, p, None, None, p, p, p, 1, 4, 4, 24, 24, 8, None) == -1
    assert b"groups" in lib.ld_last_error()
    assert lib.ld_dn_gn_backward(p, p, p, p, p, None, p, p, p, None, p, 1, 4, 4, 24, 24, 8, None) == -1
    assert lib.ld_dn_gn_backward(None, p, p, p, p, None, p, p, p, None, p, 1, 4, 4, 32, 32, 8, None) == -1
    assert lib.ld_dn_gn_backward(p, p, p, p, p, p, p, p, p, None, p, 1, 4, 4, 32, 32, 8, None) == -1     # film without dfilm
    assert lib.ld_dn_colsum(None, None, None, 1, 4, 4, 32, 32, None) == -1 and b"null" in lib.ld_last_error()
    assert lib.ld_dn_colsum(p, p, p, 1, 4, 4, 32, 16, None) == -1                                        # ldc < C
    assert lib.ld_dn_time_proj(None, None, None, None, 1, 8, 8, None) == -1
    assert lib.ld_dn_time_proj_backward(None, None, None, None, None, None, 1, 8, 8, None) == -1
    assert lib.ld_dn_pack_nhwc(None, None, 1, 32, 4, 4, 512, 16, 4, 1, 64, None) == -1
    assert lib.ld_dn_pack_nhwc(p, p, 1, 32, 4, 4, 512, 16, 4, 1, 16, None) == -1                         # ldc < C
    assert lib.ld_dn_gather3(None, None, 1, 1, 1, 0, 1, 1, 1, None) == -1
    assert int(lib.ld_dn_gn_work_bytes(1, 4, 4, 30)) == 0 and int(lib.ld_dn_gn_work_bytes(2, 16, 16, 64)) > 0


@pytest.mark.parametrize("dim,dim_out,tdim", [(32, 64, 128), (64, 64, None)])
def test_yardstick_forward_is_the_oracle(dim, dim_out, tdim):
    sd = resblock_ref.make_block(dim, dim_out, tdim, key=3)
    x = resblock_ref.uniform((2, dim, 6, 5), 1)
    temb = None if tdim is None else resblock_ref.uniform((2, tdim), 2)
    full = {"p." + k: v for k, v in sd.items()}
    with torch.no_grad():
        want = unet_ref.resnet_block(full, "p", x, temb)
        assert torch.equal(resblock_ref.forward(sd, x, temb), want)
    dout = resblock_ref.uniform(want.shape, 3)
    out32, g32 = resblock_ref.yardstick(sd, x, temb, dout, dtype=torch.float32)
    out64, g64 = resblock_ref.yardstick(sd, x, temb, dout, dtype=torch.float64)
    assert torch.equal(out32, want)
    assert set(g64) == {"x"} | ({"time_emb"} if tdim else set()) | set(sd)
    for k in g64:
        assert resblock_ref.rel_err(g32[k], g64[k]) < 1e-5, k
