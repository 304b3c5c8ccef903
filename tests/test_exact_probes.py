"""The exact-arithmetic probes of tests/exact_probes.py, proved on the CPU: every builder at every shape that
tests/test_hip_exact.py uses asserts its own preconditions (fp32 torch == fp64 torch bit for bit, results inside the
range all three storage types hold exactly, integer statistics, logit gaps, ...) when it is called, so calling it IS
the test.  And the case that motivates them: a 3x3 convolution that mis-reads one channel at one tap passes the
norm-wise rule of tests/test_hip_ops.py in bf16 and fails torch.equal on the integer probe."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from localdiffusion_hallucination_amd import rng
from oracle import unet_ref
import exact_probes as P

RTOL_BF16 = 3e-2            # hip_helpers.RTOL["bf16"], the rule of tests/test_hip_ops.py (no device import here)


@pytest.mark.parametrize("shape", P.CONV3_SHAPES + P.CONV3_SK_SHAPES + [P.BIG64_SHAPE, P.C32_SHAPE])
@pytest.mark.parametrize("frac", [False, True])
def test_conv3x3_probes(shape, frac):
    p = P.conv3x3(*shape, frac=frac)
    assert float(p.ref.abs().max()) > 8            # a probe, not a field of zeros
    if frac:          # the fraction survives: every output is an integer + odd/1024
        assert bool((((p.ref.double() * 1024).round() % 2) == 1).all())


@pytest.mark.parametrize("H,W", P.S32_SIZES)
@pytest.mark.parametrize("case", sorted(P.S32_CASES))
def test_lean_kernel_probes(case, H, W):
    P.conv3x3(2, P.S32_CASES[case], 32, H, W)
    P.conv3x3(2, P.S32_CASES[case], 32, H, W, frac=True)


def test_two_source_and_side_output_probes():
    P.conv3x3_concat_upsample()
    p = P.conv3x3_side()
    assert p.ref.shape == p.ref_side.shape == (2, 64, 17, 23)


@pytest.mark.parametrize("shape", P.CONV1_SHAPES)
def test_conv1x1_probes(shape):
    P.conv1x1(*shape)
    P.conv1x1(*shape, frac=True)


def test_conv1x1_variant_probes():
    P.conv1x1_concat()
    P.conv1x1(2, 128, 64, 9, 11, residual=True)
    P.conv1x1(2, 128, 64, 9, 11, residual=True, per_batch=True)
    for nch in (2, 3, 5, 13):
        P.conv1x1(2, 32 * nch, 64, 16, 16, key=2300 + nch)
    p = P.conv1x1_unshuffle()
    sd = {"d.1.weight": p.w, "d.1.bias": p.b}
    assert torch.equal(unet_ref.pixel_unshuffle_conv(sd, "d", p.x), p.ref)      # the oracle's rearrangement


TILE3_ALL = sorted(set(P.TILE3_RAGGED32 + P.TILE3_RAGGED64 + list(P.TILE3_WHOLE.values()) + P.TILE3_SK_SHAPES))


@pytest.mark.parametrize("shape", TILE3_ALL)
@pytest.mark.parametrize("frac", [False, True])
def test_conv3x3_tile_probes(shape, frac):
    """The shapes of tests/test_hip_conv_tiles.py: ragged for 8- and 16-row tiles, whole tiles only, eight K-chunks."""
    p = P.conv3x3(*shape, frac=frac, groups=P.tile_groups(shape[2]))
    assert float(p.ref.abs().max()) > 8
    assert p.stats.shape[1] == (12 if shape[2] == 96 else 8) and 32 % (shape[2] // p.stats.shape[1]) == 0


def test_conv3x3_tile_variant_probes():
    B, c1, c2, H, W = P.TILE3_CAT
    for cout in P.TILE3_CAT_COUTS:
        p = P.conv3x3_concat_upsample(B, c1, c2, cout, H, W, groups=P.tile_groups(cout))
        assert p.ref.shape == (B, cout, H, W) and p.x1.shape == (B, c1, H // 2, W // 2)
    for shape in P.TILE3_ADDEND_SHAPES:
        p = P.conv3x3_addend(*shape)
        assert float(p.add.abs().max()) == 4.0 and P.is_integer(p.add)
        for dt in ("bf16", "fp16"):
            P.check_representable(p.add, dt)
        # the statistics are taken AFTER the addend
        assert torch.equal(p.stats, P.gn_stats_ref(F.conv2d(p.x.double(), p.w.double(), p.b.double(), padding=1) + p.add.double(), 8))


@pytest.mark.parametrize("shape", P.TILE1_SHAPES)
def test_conv1x1_tile_probes(shape):
    """391 pixels: a 256-pixel tile plus 135, a 16-pixel group of 7 at the end -- plain, rounding, residual, per-batch weights."""
    assert shape[3] * shape[4] == 391
    P.conv1x1(*shape)
    P.conv1x1(*shape, frac=True)
    P.conv1x1(*shape, residual=True)
    P.conv1x1(*shape, residual=True, per_batch=True)


def test_conv1x1_tile_variant_probes():
    for shape in P.TILE1_GROUP_SHAPES:
        P.conv1x1(*shape)
    B, c1, c2, H, W = P.TILE1_CAT
    Bu, cu, Hu, Wu = P.TILE1_UNSHUFFLE
    for cout in P.TILE1_VARIANT_COUTS:
        P.conv1x1_concat(B, c1, c2, cout, H, W)
        p = P.conv1x1_unshuffle(Bu, cu, cout, Hu, Wu)
        assert p.x.shape == (Bu, cu, 2 * Hu, 2 * Wu)


@pytest.mark.parametrize("cin,ks,H,W", P.IMAGE_CASES)
def test_conv_image_probes(cin, ks, H, W):
    P.conv_image(cin, ks, H, W)


@pytest.mark.parametrize("cin,H,W", P.STEM_SHAPES)
@pytest.mark.parametrize("variant", ["int", "frac", "split", "mirror"])
def test_stem_probes(cin, H, W, variant):
    p = P.stem(cin, H, W, variant)
    if variant != "int":
        assert not torch.equal(P.stored(p.ref, "bf16"), p.ref)


@pytest.mark.parametrize("cin,cout", P.FINAL_CASES)
def test_final_conv_probes(cin, cout):
    P.final_conv(cin, cout)
    P.final_conv(cin, cout, frac=True)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["3x3", "1x1"])
def test_two_term_weight_probes(kind, dtype):
    P.two_term(kind, dtype)


@pytest.mark.parametrize("n", P.ATTN_SIZES)
def test_attention_probes(n):
    p = P.attention_onehot(n)
    print(f"one-hot n={n}: smallest logit gap {p.gap:.0f}")
    u = P.attention_uniform(n)
    print(f"uniform n={n}: fp32 torch distance even {u.d_even:.2e} (of 8), odd {u.d_odd:.2e}")
    # what the probe is for: ONE key skipped or counted twice moves an even channel by at least 4 / (n + 1)
    assert 4.0 / (n + 1) / 8.0 > 10 * max(1e-5, 4 * u.d_even)


@pytest.mark.parametrize("C,H,W", P.LINATTN_SHAPES)
def test_linattn_probes(C, H, W):
    p = P.linattn_uniform(C, H, W)
    n = H * W
    print(f"linattn C={C} n={n}: fp32 torch distance {p.d:.2e}")
    assert 1.0 / (n + 1) > 10 * max(1e-5, 4 * p.d)         # a pixel lost or doubled: 1.6e-4 at n = 6144
    # the oracle's RMSNorm with g = scale / sqrt(C) is the normalisation the builder used
    g = (p.scale / C ** 0.5).reshape(1, C, 1, 1)
    kv = F.conv2d(unet_ref.rms_norm(p.x, g), p.w)
    assert float(kv[:, 128:256].abs().max()) == 0.0
    assert float((kv[:, 256:].abs() - 1).abs().max()) < 1e-6 or C == 32
    assert float((kv[:, 256:].abs().round() - kv[:, 256:].abs()).abs().max()) < 1e-6


@pytest.mark.parametrize("heads", P.OTHER_HEADS)
@pytest.mark.parametrize("n", P.ATTN_HEADS_SIZES)
def test_attention_probes_at_other_head_counts(n, heads):
    """The builders with a ``heads`` parameter (tests/test_hip_attention_heads.py): the same preconditions, a tensor of
    3 * heads * 32 channels, and the default head count still gives the tensors it gave."""
    p, u = P.attention_onehot(n, heads=heads), P.attention_uniform(n, heads=heads)
    assert p.qkv.shape == u.qkv.shape == (2, n, 96 * heads) and p.ref.shape == u.ref.shape == (2, n, 32 * heads)
    assert 4.0 / (n + 1) / 8.0 > 10 * max(1e-5, 4 * u.d_even)
    assert P.attention_onehot(n, heads=4) is P.attention_onehot(n, heads=P.HEADS) and P.attention_onehot(n, heads=4).qkv.shape[-1] == 384


@pytest.mark.parametrize("heads", P.OTHER_HEADS)
@pytest.mark.parametrize("C,H,W", P.KVCTX_HEADS_SHAPES)
def test_linattn_probes_at_other_head_counts(C, H, W, heads):
    """C = 128 (64 of its channels non-zero) and an odd pixel count (7 x 7: the balanced channels sum to +1, the
    expected context there is 1 / 49) are new with these shapes."""
    p = P.linattn_uniform(C, H, W, heads=heads)
    n = H * W
    print(f"linattn C={C} n={n} heads={heads}: fp32 torch distance {p.d:.2e}")
    assert p.ref.shape == (2, heads, 32, 32) and p.w.shape == (96 * heads, C, 1, 1)
    assert 1.0 / (n + 1) > 10 * max(1e-5, 4 * p.d)
    assert float(p.ref[..., 0::2].abs().max()) == (n % 2) / n and bool((p.ref[..., 1::2].abs() == 1).all())
    g = (p.scale / C ** 0.5).reshape(1, C, 1, 1)
    kv = F.conv2d(unet_ref.rms_norm(p.x, g), p.w)
    hid = 32 * heads
    assert float(kv[:, hid:2 * hid].abs().max()) == 0.0
    assert float((kv[:, 2 * hid:].abs() - 1).abs().max()) < 1e-6


@pytest.mark.parametrize("n", P.LINOUT_SIZES)
@pytest.mark.parametrize("C", P.LINOUT_CHANNELS)
def test_linout_probes(C, n):
    """Calling the builders proves them (_linout_check).  And what the one-hot probe is for: two k-slots of the chained
    operand exchanged change stored outputs on it, at every shape, while the uniform probe cannot see that."""
    p, u = P.linout_onehot(C, n), P.linout_uniform(C, n)
    assert p.x.shape == (4, C, n) and u.x.shape == (2, C, n)
    assert int((p.x != 0).sum()) == 4 * n                                   # one non-zero channel per pixel
    for dt in ("bf16", "fp16"):
        bad = P.linout_swapped_slots(p, dt)
        assert not torch.equal(bad, p.ref)
        assert torch.equal(P.linout_swapped_slots(u, dt), u.ref)
    print(f"linout one-hot C={C} n={n}: {int((bad != p.ref).sum())} of {bad.numel()} outputs differ with k-slots 4 and 20 exchanged")


def test_linout_contract_is_the_oracle_block():
    """linout_contract without rounding, fed the oracle's own context, IS LinearAttention.forward + x (fp64 vs the fp32
    oracle): the reference of the random-operand test restates the right operation."""
    B, C, H, W = 2, 64, 9, 11
    n = H * W
    r = lambda shape, key, lo=-1.0, hi=1.0: torch.from_numpy(rng.uniform(shape, 1234, key, lo, hi))
    x = r((B, C, H, W), 1, -2, 2)
    sd = {"a.norm.g": r((1, C, 1, 1), 2, 0.5, 1.5), "a.to_qkv.weight": r((384, C, 1, 1), 3, -0.3, 0.3),
          "a.to_out.0.weight": r((C, 128, 1, 1), 4, -0.3, 0.3), "a.to_out.0.bias": r((C,), 5), "a.to_out.1.g": r((1, C, 1, 1), 6, 2.0, 4.0)}
    ref = unet_ref.linear_attention(sd, "a", x) + x
    _, k, v = [t.reshape(B, 4, 32, n) for t in F.conv2d(unet_ref.rms_norm(x, sd["a.norm.g"]), sd["a.to_qkv.weight"]).chunk(3, dim=1)]
    ctxn = torch.einsum("bhdn,bhen->bhde", k.softmax(dim=-1), v)
    scale = sd["a.norm.g"].flatten() * C ** 0.5
    got = P.linout_contract(x.reshape(B, C, n), sd["a.to_qkv.weight"][:128, :, 0, 0] * scale[None, :], ctxn, sd["a.to_out.0.weight"][:, :, 0, 0],
                            sd["a.to_out.0.bias"], sd["a.to_out.1.g"].flatten() * C ** 0.5, 32 ** -0.5)
    err = float((got.reshape(B, C, H, W) - ref.double()).abs().max()) / float(ref.abs().max())
    print(f"linout_contract vs the oracle block: {err:.2e}")
    assert err < 1e-5


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("C", P.LINOUT_CHANNELS)
def test_linout_random_operands(C, dtype):
    """The restatement's own distance d from the unrounded fp64 value, per weight-term count (what the GPU test's
    max(floor, 2 d) is made of): a few storage half-ulps of the largest output, and two terms are not worse than one."""
    for n in (49, 1024):
        p = P.linout_random(C, n, dtype)
        print(f"linout random C={C} n={n} {dtype}: d one term {p.d[1]:.2e}, two terms {p.d[2]:.2e}, max |ref| {p.top:.2f}")
        ulp = 2.0 ** -8 if dtype == "bf16" else 2.0 ** -11
        assert 0.25 * ulp < p.d[1] < 8 * ulp and p.d[2] <= p.d[1] * 1.05
        assert float((p.qshift[:, None] - (p.wq * p.scale[None, :]).norm(dim=1).reshape(4, 32)).min()) > 0
        assert float(p.qshift.max()) <= 40.0                                 # a bound the product code would pass on (unet.py)
        s = P.linout_random(C, n, dtype, sharp=True)
        print(f"   sharp: d one term {s.d[1]:.2e}, two terms {s.d[2]:.2e}; rms {s.d_rms[1]:.3e}, {s.d_rms[2]:.3e} ({s.d_rms[2] / s.d_rms[1]:.3f})")
        assert s.d_rms[2] < 0.995 * s.d_rms[1]                               # here the second term shows


def _emulated_bf16(conv, x, w, b):
    """A clean bf16 kernel: fp32 arithmetic on bf16-rounded operands, the output rounded once."""
    q = lambda t: t.to(torch.bfloat16).float()
    return q(conv(q(x), q(w), b))


def test_a_misread_channel_passes_the_normwise_rule_and_fails_the_exact_probe():
    """256 -> 256 at 8 x 8 on the inputs of test_hip_ops.test_conv3x3_plain_and_stats: the last input channel of the
    centre tap reads its neighbour.  max-abs error / max-abs reference stays under the bf16 bound of 3e-2 (a clean
    kernel sits at 2-3e-3); on the integer probe of the same shape the same mutation changes output bits."""
    B, cin, cout, H, W = 1, 256, 256, 8, 8
    r = lambda shape, key, lo=-1.0, hi=1.0: torch.from_numpy(rng.uniform(shape, 1234, key, lo, hi))
    x, w, b = r((B, cin, H, W), 1), r((cout, cin, 3, 3), 2, -0.1, 0.1), r((cout,), 3)
    q = lambda t: t.to(torch.bfloat16).float()
    ref = F.conv2d(q(x), q(w), b, padding=1)
    rel = lambda got: float((got - ref).abs().max()) / float(ref.abs().max())
    clean = rel(_emulated_bf16(lambda x, w, b: F.conv2d(x, w, b, padding=1), x, w, b))
    broken = rel(_emulated_bf16(P.misread_last_channel, x, w, b))
    print(f"old rule: clean {clean:.2e}, one mis-read channel {broken:.2e}, bound {RTOL_BF16:.0e}")
    assert clean < RTOL_BF16 / 8
    assert broken < RTOL_BF16 and broken > 2 * clean       # wrong, visibly worse than clean, and let through
    p = P.conv3x3(B, cin, cout, H, W)
    good = _emulated_bf16(lambda x, w, b: F.conv2d(x, w, b, padding=1), p.x, p.w, p.b)
    bad = _emulated_bf16(P.misread_last_channel, p.x, p.w, p.b)
    assert torch.equal(good, p.ref)
    assert not torch.equal(bad, p.ref)
    print(f"integer probe: {int((bad != p.ref).sum())} of {bad.numel()} outputs differ")
