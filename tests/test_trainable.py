"""The scaffold of the trainable modules (localdiffusion_hallucination_amd/trainable.py) where it can be checked without a
device: the packed-weight cache, the shared input check, and ``pack_conv``'s index arithmetic against plain torch."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import trainable


# ------------------------------------------------------------------------------------------------ 1. PackedWeights
class Toy(trainable.PackedWeights, nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(3, 2)
        self.packs = 0

    def _pack(self, dev):
        self.packs += 1
        return (self.packs, self.lin.weight.detach().clone())


def test_packed_weights_repack_exactly_when_a_parameter_may_have_changed():
    toy, dev = Toy(), torch.device("cpu")
    first = toy._packed_for(dev)
    assert toy.packs == 1 and toy._packed_for(dev) is first and toy.packs == 1            # nothing changed: no repack
    with torch.no_grad():
        toy.lin.bias.add_(1)                                                              # the version moves
    assert toy._packed_for(dev)[0] == 2 and toy._packed_for(dev)[0] == 2 and toy.packs == 2
    toy.load_state_dict({k: v + 1 for k, v in toy.state_dict().items()})
    packed = toy._packed_for(dev)
    assert toy.packs == 3 and torch.equal(packed[1], toy.lin.weight)                      # and holds the new weights
    toy.double().float()                                                                  # _apply
    assert toy._packed_for(dev)[0] == 4 and toy.packs == 4
    assert toy._packed_for(dev)[0] == 4 and toy.packs == 4
    toy.invalidate()
    assert toy._packed_for(dev)[0] == 5 and toy.packs == 5


# ------------------------------------------------------------------------------------------------ 1b. the switches
MODULES = {"ResnetBlock": lambda: ldh.ResnetBlock(32, 64), "LinearAttention": lambda: ldh.LinearAttention(32),
           "Attention": lambda: ldh.Attention(32), "Downsample": lambda: ldh.Downsample(32, 64),
           "Upsample": lambda: ldh.Upsample(64, 32), "Conv2d": lambda: ldh.Conv2d(32, 32, 3, padding=1),
           "BasicBlock": lambda: ldh.BasicBlock(32, 32, 64)}


@pytest.mark.parametrize("cls", MODULES)
@pytest.mark.parametrize("switch", trainable.SWITCHES)
def test_every_switch_refuses_what_its_class_does_not_list(switch, cls):
    """A module has a switch exactly when its class defines the default and the tuple; a value outside the tuple is a
    ``ValueError`` with one text, and the old value stays."""
    mod = MODULES[cls]()
    assert type(mod).__name__ == cls and isinstance(mod, trainable.TrainableModule)
    has = hasattr(type(mod), switch)
    assert has == hasattr(type(mod), trainable.SWITCHES[switch])
    assert has or switch in ("attn_precision", "full_attn_precision")          # (every module has the first two)
    if not has:
        return
    allowed = getattr(type(mod), trainable.SWITCHES[switch])
    assert getattr(mod, switch) == "fp32" and allowed[0] == "fp32" and set(allowed) <= {"fp32", "bf16"}
    for value in allowed[::-1]:
        setattr(mod, switch, value)                                             # (ends at "fp32")
        assert getattr(mod, switch) == value
    bad = [v for v in ("fp32", "bf16", "fp16", "BF16", "", None, 16, ("bf16",)) if v not in allowed]
    for value in bad:
        with pytest.raises(ValueError) as e:
            setattr(mod, switch, value)
        assert str(e.value) == f"{cls}: {switch} {value!r} is not one of " + ", ".join(repr(v) for v in allowed)
        assert getattr(mod, switch) == "fp32"
    assert switch not in "".join(mod.state_dict())


# ------------------------------------------------------------------------------------------------ 2. the input check
@pytest.mark.parametrize("make", [lambda: ldh.ResnetBlock(32, 64), lambda: ldh.LinearAttention(32, heads=1),
                                  lambda: ldh.Attention(32, heads=1)], ids=["ResnetBlock", "LinearAttention", "Attention"])
def test_every_module_refuses_a_bad_input_under_its_own_name(make):
    mod = make()
    name = type(mod).__name__
    assert isinstance(mod, trainable.TrainableModule) and mod.debug_fill is None
    with pytest.raises(ValueError, match=name + r": .*CPU"):
        mod(torch.zeros(1, 32, 4, 4))
    with pytest.raises(ValueError, match=name + r": .*float32"):
        mod(torch.zeros(1, 32, 4, 4, dtype=torch.float16))
    with pytest.raises(ValueError, match=name + r": .*non-empty \[B, 32, H, W\]"):
        mod(torch.zeros(1, 16, 4, 4))
    with pytest.raises(ValueError, match=name + r": .*non-empty \[B, 32, H, W\]"):
        mod(torch.zeros(32, 4, 4))
    mod.debug_fill = 1.0                                                                  # settable per instance
    assert type(mod).debug_fill is None


def test_resnet_block_without_time_emb_dim_refuses_a_time_emb():
    with pytest.raises(ValueError, match="ResnetBlock: .*time_emb_dim"):
        ldh.ResnetBlock(32, 32)(torch.zeros(2, 32, 4, 4), torch.zeros(2, 64))
    with pytest.raises(ValueError, match=r"ResnetBlock: time_emb must be float32 \[2, 64\]"):
        ldh.ResnetBlock(32, 32, time_emb_dim=64)(torch.zeros(2, 32, 4, 4), torch.zeros(1, 64))


# ------------------------------------------------------------------------------------------------ 3. pack_conv
class ScatterLib:
    """Stands in for the library: ``ld_seg_permute3`` as out[off + i0 s0 + i1 s1 + i2 s2] = in[i] in torch on CPU memory,
    every call recorded."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def floats(ptr, n):
        return torch.from_numpy(np.ctypeslib.as_array((C.c_float * n).from_address(ptr)))

    def ld_seg_permute3(self, src, dst, d0, d1, d2, off, s0, s1, s2, st):
        self.calls.append((d0, d1, d2, off, s0, s1, s2))
        i0, i1, i2 = torch.meshgrid(torch.arange(d0), torch.arange(d1), torch.arange(d2), indexing="ij")
        idx = (off + i0 * s0 + i1 * s1 + i2 * s2).reshape(-1)
        assert int(idx.min()) >= 0 and idx.unique().numel() == idx.numel()
        self.floats(dst, int(idx.max()) + 1)[idx] = self.floats(src, d0 * d1 * d2)
        return 0


@pytest.mark.parametrize("co,ci,k", [(32, 32, 3), (96, 32, 1)])
def test_pack_conv_makes_the_forward_and_the_data_gradient_layout(co, ci, k):
    cop, cip, kk = trainable.pad64(co), trainable.pad64(ci), k * k
    w = torch.randn(co, ci, k, k, generator=torch.Generator().manual_seed(co + k))
    lib = ScatterLib()
    fwd, dgr = trainable.pack_conv(lib, None, nn.Parameter(w.clone()), co, cop, ci, cip, k)
    assert lib.calls == [(co, ci, kk, 0, kk * cip, 1, cip), (co, ci, kk, (kk - 1) * cop, 1, kk * cop, -cop)]
    want_f = F.pad(w.permute(0, 2, 3, 1).reshape(co, kk, ci), (0, cip - ci, 0, 0, 0, cop - co))
    want_d = F.pad(w.flip(2, 3).permute(1, 2, 3, 0).reshape(ci, kk, co), (0, cop - co, 0, 0, 0, cip - ci))
    assert fwd.shape == (cop * kk * cip,) and torch.equal(fwd.reshape(cop, kk, cip), want_f)
    assert dgr.shape == (cip * kk * cop,) and torch.equal(dgr.reshape(cip, kk, cop), want_d)
    assert not fwd.requires_grad and not dgr.requires_grad


def test_pack_vec_pads_with_zeros():
    v = trainable.pack_vec(nn.Parameter(torch.arange(1.0, 4.0)), 8)
    assert v.tolist() == [1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0] and not v.requires_grad
    assert trainable.pad64(1) == 64 and trainable.pad64(64) == 64 and trainable.pad64(96) == 128
