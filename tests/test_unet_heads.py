"""Head counts of the denoiser's attention blocks, the part that needs no GPU: what the constructor accepts, and that the
oracle and the procedural weights follow cfg.attn_heads (tests/test_hip_attention_heads.py compares the kernels with
them at 2 and 8 heads)."""
import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import rng, weights
from oracle import unet_ref

KW = dict(dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist")


@pytest.mark.parametrize("heads", [3, 1, 5, 0, -2])
def test_odd_head_counts_are_refused_by_the_constructor(heads):
    """hidden = 32 * heads must be a multiple of 64 (the to_qkv epilogues of ld_conv1x1 work on 64-channel tiles): a
    ValueError at construction, like attn_dim_head != 32, not an ld_conv1x1 error at the first forward."""
    with pytest.raises(ValueError, match="attn_heads"):
        ldh.Unet(dim=32, attn_heads=heads)
    with pytest.raises(ValueError, match="attn_heads"):
        ldh.Unet(dim=32, init_dim=32, attn_heads=heads, **KW)


@pytest.mark.parametrize("heads", [2, 4, 8])
def test_even_head_counts_reach_the_configuration_the_weights_and_the_oracle(heads):
    net = ldh.Unet(dim=32, init_dim=32, attn_heads=heads, **KW)
    assert net.cfg.attn_heads == heads and net.cfg.hidden == 32 * heads
    sd = {k: torch.from_numpy(v) for k, v in weights.procedural_state_dict(net.cfg, 0).items()}
    assert list(net.state_dict().keys()) == list(sd.keys())
    qkv = [k for k in sd if k.endswith(".to_qkv.weight")]
    assert qkv and all(sd[k].shape[0] == 96 * heads for k in qkv)
    net.load_state_dict(sd)
    B, H = 1, 28
    x = torch.from_numpy(rng.randn((B, 1, H, H), 1, 100))
    cond = torch.from_numpy(rng.uniform((B, 1, H, H), 1, 101, 0.0, 2.0))
    with torch.no_grad():
        y = unet_ref.unet_forward(sd, net.cfg, x, cond, torch.full((B,), 5, dtype=torch.long))
    assert tuple(y.shape) == (B, 1, H, H) and bool(torch.isfinite(y).all())
