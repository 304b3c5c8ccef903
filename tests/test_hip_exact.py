"""Exact-arithmetic probes of the forward kernels (tests/exact_probes.py): inputs on which every product and partial sum
is exact, so the kernels' chunk width, MFMA shape and accumulation order cannot matter and the comparison with the
fp64 result is torch.equal -- a mis-read channel, a key or pixel lost or counted twice, an output element never
written all change bits here, while the norm-wise rule of test_hip_ops.py lets them through in 16-bit storage.
Every output buffer holds NaN before the launch; kernel variants are routed through ld_tuning_set, restored
afterwards, and confirmed with the launch counters where one exists."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from localdiffusion_hallucination_amd import _cabi as cabi       # noqa: E402
from localdiffusion_hallucination_amd.tuning import kernel_table  # noqa: E402
import exact_probes as P                                           # noqa: E402
import hip_helpers as hh                                           # noqa: E402

DTYPES = ["fp32", "bf16", "fp16"]
LOWP = ["bf16", "fp16"]
HERE = os.path.dirname(os.path.abspath(__file__))


@contextlib.contextmanager
def routed(**sets):
    """Entries of the library's routing table for the duration of the block."""
    lib = cabi.lib()
    keep = kernel_table(lib)
    try:
        for k, v in sets.items():
            cabi.check(lib.ld_tuning_set(k.encode(), v), "tuning_set")
        yield lib
    finally:
        for k, v in keep.items():
            cabi.check(lib.ld_tuning_set(k.encode(), v), "tuning_set")


class counted:
    """Launch counters across a block: ``c[which]`` = launches counted since it was entered."""
    def __enter__(self):
        self.lib = cabi.lib()
        self.at = {w: self.lib.ld_counter(w) for w in (cabi.COUNTER_CONV3X3_C32, cabi.COUNTER_CONV3X3_GENERIC, cabi.COUNTER_CONV3X3_S32)}
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        return False

    def __getitem__(self, which):
        return self.lib.ld_counter(which) - self.at[which]


def want(ref, dtype):
    """The exact fp32 value as ``dtype`` storage holds it (one round-to-nearest-even; the identity on integer probes)."""
    return P.stored(ref, dtype)


def conv3(srcs, p, B, H, W, cout, dtype, stats=True, **kw):
    st = hh.stats_buffer(B, 8) if stats else None
    out = hh.conv3x3(srcs, hh.pack(p.w, dtype, 3), p.b.to(hh.DEV), B, H, W, cout, dtype, stats=st, groups=8, **kw)
    return out, st


def assert_conv(out, st, p, dtype, what=""):
    got = hh.nchw(out)
    assert torch.equal(got, want(p.ref, dtype)), (what, int((got != want(p.ref, dtype)).sum()), float((got - p.ref).abs().max()))
    if st is not None:
        assert torch.equal(st.sum(1).cpu(), p.stats), (what, float((st.sum(1).cpu() - p.stats).abs().max()))


# ------------------------------------------------------------------------------------------------ 3a / 3b: ld_conv3x3
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frac", [False, True], ids=["int", "rne"])
@pytest.mark.parametrize("B,cin,cout,H,W", P.CONV3_SHAPES)
def test_conv3x3_generic(dtype, B, cin, cout, H, W, frac):
    """The generic kernel (lean and persistent variants routed off): output and fp64 statistics equal to the integer
    reference; with odd/1024 in the bias the stored output is the one round-to-nearest-even of the exact value."""
    p = P.conv3x3(B, cin, cout, H, W, frac=frac)
    with routed(conv_s32=0, conv_c32=0), counted() as c:
        out, st = conv3([hh.make_src(hh.nhwc(p.x, dtype), cin)], p, B, H, W, cout, dtype, stats=not frac)
        assert c[cabi.COUNTER_CONV3X3_GENERIC] == 1 and c[cabi.COUNTER_CONV3X3_S32] == 0 and c[cabi.COUNTER_CONV3X3_C32] == 0
    assert_conv(out, st, p, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv3x3_concat_upsample(dtype):
    p = P.conv3x3_concat_upsample()
    B, c1, c2, cout, H, W = 2, 64, 32, 32, 12, 12
    srcs = [hh.make_src(hh.nhwc(p.x1, dtype), c1, ups=1), hh.make_src(hh.nhwc(p.x2, dtype), c2)]
    out, st = conv3(srcs, p, B, H, W, cout, dtype)
    assert_conv(out, st, p, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv3x3_source_is_a_channel_slice_of_a_wider_tensor(dtype):
    """pix_stride: the first 32 channels come from a 64-channel tensor whose other channels hold NaN."""
    B, cin, cout, H, W = 2, 64, 32, 17, 23
    p = P.conv3x3(B, cin, cout, H, W)
    wide = hh.padded(p.x[:, :32], 64).to(hh.TDT[dtype])
    srcs = [hh.make_src(wide, 32, stride=64), hh.make_src(hh.nhwc(p.x[:, 32:].contiguous(), dtype), 32)]
    out, st = conv3(srcs, p, B, H, W, cout, dtype)
    assert_conv(out, st, p, dtype)


@pytest.mark.parametrize("dtype", LOWP)
def test_conv3x3_side_output(dtype):
    """The res_conv as a second output of the launch: both outputs and the statistics, ragged 17 x 23."""
    p = P.conv3x3_side()
    B, c1, c2, cout, H, W = 2, 64, 32, 64, 17, 23
    srcs = [hh.make_src(hh.nhwc(p.x1, dtype), c1), hh.make_src(hh.nhwc(p.x2, dtype), c2)]
    st = hh.stats_buffer(B, 8)
    with counted() as c:
        out, side = hh.conv3x3(srcs, hh.pack(p.w, dtype, 3), p.b.to(hh.DEV), B, H, W, cout, dtype, stats=st, groups=8,
                               side=(hh.pack(p.wr, dtype, 1), p.br.to(hh.DEV)))
        assert c[cabi.COUNTER_CONV3X3_GENERIC] == 1
    assert_conv(out, st, p, dtype)
    assert torch.equal(hh.nchw(side), p.ref_side)


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("frac", [False, True], ids=["int", "rne"])
@pytest.mark.parametrize("H,W", P.S32_SIZES)
@pytest.mark.parametrize("case", sorted(P.S32_CASES))
def test_conv3x3_s32_lean_kernel(dtype, case, H, W, frac):
    """conv_s32 = 7, conv_s32_min_tiles = 1: 48 x 32 runs on the lean kernel (counter asserted).  Its router takes whole
    16 x 16 tiles only (conv3x3_s32.hip: H and W multiples of 16), so the ragged 40 x 24 launch must be DECLINED and
    computed by the generic kernel -- asserted with the counters too, and the result is held to the same equality."""
    B, cout, cin = 2, 32, P.S32_CASES[case]
    p = P.conv3x3(B, cin, cout, H, W, frac=frac)
    if case == "two32":
        wide = hh.padded(p.x[:, :32], 64).to(hh.TDT[dtype])
        srcs = [hh.make_src(wide, 32, stride=64), hh.make_src(hh.nhwc(p.x[:, 32:].contiguous(), dtype), 32)]
    else:
        srcs = [hh.make_src(hh.nhwc(p.x, dtype), cin)]
    lean = H % 16 == 0 and W % 16 == 0
    with routed(conv_s32=7, conv_s32_min_tiles=1, conv_c32=0), counted() as c:
        out, st = conv3(srcs, p, B, H, W, cout, dtype, stats=not frac)
        assert c[cabi.COUNTER_CONV3X3_S32] == int(lean) and c[cabi.COUNTER_CONV3X3_GENERIC] == int(not lean)
    assert_conv(out, st, p, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv3x3_big64_tile(dtype):
    """The 64-channel x 16-row tile (conv_big4_min = 1, conv_mt4_min_wgs = 1) on a ragged 40 x 24 map."""
    B, cin, cout, H, W = P.BIG64_SHAPE
    p = P.conv3x3(B, cin, cout, H, W)
    with routed(conv_big4_min=1, conv_mt4_min_wgs=1), counted() as c:
        out, st = conv3([hh.make_src(hh.nhwc(p.x, dtype), cin)], p, B, H, W, cout, dtype)
        assert c[cabi.COUNTER_CONV3X3_GENERIC] == 1
    assert_conv(out, st, p, dtype)


@pytest.mark.parametrize("dtype", LOWP)
def test_conv3x3_c32_persistent_kernel(dtype):
    """conv_c32 on, conv_c32_min_tiles = 1, 32 -> 32 at 32 x 32: the smallest map the persistent kernel's router takes
    (conv3x3_c32.hip: Cout = 32, ONE K-chunk, H, W >= 32 and multiples of 16).  16-bit storage: a K-chunk of fp32
    storage is 16 channels and sources are multiples of 32, so no fp32 launch reaches that kernel."""
    B, cin, cout, H, W = P.C32_SHAPE
    p = P.conv3x3(B, cin, cout, H, W)
    with routed(conv_c32=1, conv_c32_min_tiles=1), counted() as c:
        out, st = conv3([hh.make_src(hh.nhwc(p.x, dtype), cin)], p, B, H, W, cout, dtype)
        assert c[cabi.COUNTER_CONV3X3_C32] == 1 and c[cabi.COUNTER_CONV3X3_S32] == 0 and c[cabi.COUNTER_CONV3X3_GENERIC] == 0
    assert_conv(out, st, p, dtype)


def _sk_probe():
    """Child process of test_conv3x3_split_k_halves (LD_CONV_SK is read once per process)."""
    lib = cabi.lib()
    assert kernel_table(lib)["conv_sk"] == 2
    for dtype in LOWP:
        for (B, cin, cout, H, W) in P.CONV3_SK_SHAPES:
            p = P.conv3x3(B, cin, cout, H, W)
            with routed(conv_s32=0, conv_c32=0), counted() as c:
                out, st = conv3([hh.make_src(hh.nhwc(p.x, dtype), cin)], p, B, H, W, cout, dtype)
                assert c[cabi.COUNTER_CONV3X3_GENERIC] == 1
            assert_conv(out, st, p, dtype, (dtype, cin, cout))
    print("SK-EXACT-OK")


def test_conv3x3_split_k_halves():
    """LD_CONV_SK=2 (two halves of a workgroup own alternate K-chunks, partial sums joined through LDS): an odd chunk
    count on a ragged map and eight chunks, output and statistics."""
    code = (f"import sys; sys.path.insert(0, {HERE!r}); sys.path.insert(0, {os.path.dirname(HERE)!r}); "
            "import test_hip_exact as t; t._sk_probe()")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LD_CONV_SK="2"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SK-EXACT-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ 3a / 3b: ld_conv1x1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frac", [False, True], ids=["int", "rne"])
@pytest.mark.parametrize("B,cin,cout,H,W", P.CONV1_SHAPES)
def test_conv1x1_plain(dtype, B, cin, cout, H, W, frac):
    p = P.conv1x1(B, cin, cout, H, W, frac=frac)
    out = hh.conv1x1([hh.make_src(hh.nhwc(p.x, dtype), cin)], hh.pack(p.w, dtype, 1), B, H, W, cout, dtype, bias=p.b.to(hh.DEV))
    assert torch.equal(hh.nchw(out), want(p.ref, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv1x1_concat_and_unshuffle(dtype):
    p = P.conv1x1_concat()
    B, c1, c2, cout, H, W = 1, 64, 32, 64, 12, 10
    out = hh.conv1x1([hh.make_src(hh.nhwc(p.x1, dtype), c1), hh.make_src(hh.nhwc(p.x2, dtype), c2)], hh.pack(p.w, dtype, 1),
                     B, H, W, cout, dtype, bias=p.b.to(hh.DEV))
    assert torch.equal(hh.nchw(out), p.ref)
    p = P.conv1x1_unshuffle()
    out = hh.conv1x1([hh.make_src(hh.nhwc(p.x, dtype), 32)], hh.pack(p.w, dtype, 1, unshuffle=1), B, H, W, cout, dtype,
                     bias=p.b.to(hh.DEV), unshuffle=1)
    assert torch.equal(hh.nchw(out), p.ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv1x1_residual_and_per_batch_weights(dtype):
    """EPI_RES with an integer residual; then a different weight per batch element (weight_bstride)."""
    B, cin, cout, H, W = 2, 128, 64, 9, 11
    p = P.conv1x1(B, cin, cout, H, W, residual=True)
    out = hh.conv1x1([hh.make_src(hh.nhwc(p.x, dtype), cin)], hh.pack(p.w, dtype, 1), B, H, W, cout, dtype, bias=p.b.to(hh.DEV),
                     epi=cabi.EPI_RES, residual=hh.nhwc(p.res, dtype))
    assert torch.equal(hh.nchw(out), p.ref)
    p = P.conv1x1(B, cin, cout, H, W, residual=True, per_batch=True)
    wp = torch.stack([hh.pack(p.w[i], dtype, 1) for i in range(B)]).contiguous()
    es = 4 if dtype == "fp32" else 2
    out = hh.conv1x1([hh.make_src(hh.nhwc(p.x, dtype), cin)], wp, B, H, W, cout, dtype, bias=p.b.to(hh.DEV),
                     epi=cabi.EPI_RES, residual=hh.nhwc(p.res, dtype), bstride=cout * cin * es)
    assert torch.equal(hh.nchw(out), p.ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nch", [2, 3, 5, 13])
def test_conv1x1_grouped_staging_and_plain_k_loop(dtype, nch):
    """c1_group = 1 (four chunks per barrier pair / pairs) and c1_group = 0 (the plain K loop) at K extents with full
    groups and a partial last group: both equal to the integer reference (test_hip_ops holds them equal to each other)."""
    B, cin, cout, H, W = 2, 32 * nch, 64, 16, 16
    p = P.conv1x1(B, cin, cout, H, W, key=2300 + nch)
    for group in (1, 0):
        with routed(c1_group=group):
            out = hh.conv1x1([hh.make_src(hh.nhwc(p.x, dtype), cin)], hh.pack(p.w, dtype, 1), B, H, W, cout, dtype, bias=p.b.to(hh.DEV))
            torch.cuda.synchronize()
        assert torch.equal(hh.nchw(out), p.ref), group


# ------------------------------------------------------------------------------------------------ image convolutions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,ks,H,W", P.IMAGE_CASES)
def test_conv_image(dtype, cin, ks, H, W):
    B = 2
    p = P.conv_image(cin, ks, H, W)
    out, stats = hh.nans(B, H, W, 32, dtype=hh.TDT[dtype]), hh.stats_buffer(B, 16)
    xd, wd, bd = p.x.to(hh.DEV), p.w.to(hh.DEV), p.b.to(hh.DEV)
    cabi.check(cabi.lib().ld_conv_image(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), stats.data_ptr(),
                                        16, B, cin, H, W, ks, cabi.dtype_code(dtype), hh.st()), "conv_image")
    assert torch.equal(hh.nchw(out), p.ref)
    assert torch.equal(stats.sum(1).cpu(), p.stats)


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("variant", ["int", "frac", "split", "mirror"])
@pytest.mark.parametrize("cin,H,W", P.STEM_SHAPES)
def test_conv_stem(dtype, cin, H, W, variant):
    """The MFMA stem: integer operands; the rounding variant; and operands that need the lo term of its bf16 hi/lo
    split, on the image side (``split``) and on the weight side (``mirror``) -- the stored output is the exact value
    rounded once."""
    B = 2
    p = P.stem(cin, H, W, variant)
    lib = cabi.lib()
    xd, wd, bd = p.x.to(hh.DEV), p.w.to(hh.DEV).contiguous(), p.b.to(hh.DEV)
    wp = torch.zeros(int(lib.ld_stem_packed_bytes()), dtype=torch.uint8, device=hh.DEV)
    cabi.check(lib.ld_pack_stem_weight(wd.data_ptr(), wp.data_ptr(), cin, hh.st()), "pack_stem")
    out = hh.nans(B, H, W, 32, dtype=hh.TDT[dtype])
    cabi.check(lib.ld_conv_stem(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), out.data_ptr(), B, cin, H, W,
                                cabi.dtype_code(dtype), hh.st()), "conv_stem")
    assert torch.equal(hh.nchw(out), want(p.ref, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frac", [False, True], ids=["int", "rne"])
@pytest.mark.parametrize("cin,cout", P.FINAL_CASES)
def test_final_conv(dtype, cin, cout, frac):
    """NHWC storage -> NCHW fp32: the output is fp32 whatever the storage, so it equals the exact value in both variants."""
    B, H, W = 2, 9, 11
    p = P.final_conv(cin, cout, frac=frac)
    out = hh.nans(B, cout, H, W)
    xd, wd, bd = hh.nhwc(p.x, dtype), p.w.reshape(cout, cin).contiguous().to(hh.DEV), p.b.to(hh.DEV)
    cabi.check(cabi.lib().ld_final_conv(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, W, cin, cout,
                                        cabi.dtype_code(dtype), hh.st()), "final_conv")
    assert torch.equal(out.cpu(), p.ref)


# ------------------------------------------------------------------------------------------------ two-term weights
@pytest.mark.parametrize("dtype", LOWP)
def test_two_term_weights_are_exact(dtype):
    """Weights k/256 (bf16; k/4096 for fp16, which holds k/256 in one term) need hi + lo: with weight_terms = 2 EVERY
    element of the 3x3 (concat + nearest x2) and of the 1x1 (concat) result is the exact value stored once; with one
    term the rounded weights give another result."""
    B, c1, c2, cout, H, W = 2, 64, 32, 64, 16, 16
    lib = cabi.lib()

    def packed(w, k, terms):
        w = w.to(hh.DEV, torch.float32).contiguous()
        out = hh.nans(terms * w.numel(), dtype=hh.TDT[dtype])
        cabi.check(lib.ld_pack_conv_weight_terms(w.data_ptr(), None, out.data_ptr(), w.shape[0], w.shape[1], k, 0,
                                                 cabi.dtype_code(dtype), terms, hh.st()), "pack")
        return out
    for kind in ("3x3", "1x1"):
        p = P.two_term(kind, dtype)
        for terms in (1, 2):
            a = cabi.Conv3x3Args() if kind == "3x3" else cabi.Conv1x1Args()
            s1 = hh.make_src(hh.nhwc(p.x1, dtype), c1, ups=1 if kind == "3x3" else 0)
            s2 = hh.make_src(hh.nhwc(p.x2, dtype), c2)
            a.src[0], a.src[1], a.nsrc = s1, s2, 2
            wp, bd = packed(p.w, 3 if kind == "3x3" else 1, terms), p.b.to(hh.DEV)
            out = hh.nans(B, H, W, cout, dtype=hh.TDT[dtype])
            a.weight, a.bias, a.out, a.weight_terms = wp.data_ptr(), bd.data_ptr(), out.data_ptr(), terms
            a.B, a.H, a.W, a.Cout, a.dtype = B, H, W, cout, cabi.dtype_code(dtype)
            if kind == "3x3":
                cabi.check(lib.ld_conv3x3(C.byref(a), hh.st()), "conv3x3")
            else:
                a.epilogue, a.hidden, a.q_scale = cabi.EPI_PLAIN, 128, 32 ** -0.5
                cabi.check(lib.ld_conv1x1(C.byref(a), hh.st()), "conv1x1")
            got = hh.nchw(out)
            assert bool(torch.isfinite(got).all())
            assert torch.equal(got, want(p.ref, dtype)) == (terms == 2), (kind, terms, float((got - p.ref).abs().max()))


# ------------------------------------------------------------------------------------------------ 3c: ld_attention
def _attention(qkv, dtype):
    B, n, _ = qkv.shape
    qd = qkv.to(hh.DEV, hh.TDT[dtype]).contiguous()
    out = hh.nans(B, n, P.HID, dtype=hh.TDT[dtype])
    cabi.check(cabi.lib().ld_attention(qd.data_ptr(), out.data_ptr(), B, n, P.HEADS, P.DH, cabi.dtype_code(dtype), hh.st()), "attention")
    torch.cuda.synchronize()
    return out.float().cpu()


ATTN_ROUTES = [("one", dt) for dt in DTYPES] + [("two", dt) for dt in LOWP]
ROUTE_SETS = {"one": dict(attn_split_max_wgs=0), "two": dict(attn_split_max_wgs=1 << 30, attn_split_min_n=256)}


@pytest.mark.parametrize("route,dtype", ATTN_ROUTES)
@pytest.mark.parametrize("n", P.ATTN_SIZES)
def test_attention_one_hot(route, dtype, n):
    """Every query selects exactly one key (logit 2048, every other at least 128 lower): the output is the gather
    v[pi(i)], bit for bit, for one key group and for two (ragged last tiles, n = 324's empty last tile of the second
    group; n = 49 fits one tile, where the router must keep one group).  A key tile that starts one key late, a key
    masked by mistake or a group boundary off by one loses some query's only key."""
    p = P.attention_onehot(n)
    with routed(**ROUTE_SETS[route]):
        got = _attention(p.qkv, dtype)
    assert torch.equal(got, p.ref), (int((got != p.ref).any(-1).sum()), "queries differ")


@pytest.mark.parametrize("route,dtype", ATTN_ROUTES)
@pytest.mark.parametrize("n", P.ATTN_SIZES)
def test_attention_uniform(route, dtype, n):
    """q = 0: the output is the mean of v over the keys -- 0 on even channels (+-m pairs, 4 <= m <= 8), 1 on odd ones.
    Even channels: max |got| / 8 <= max(1e-5, 4 d), d = fp32 torch's own distance from the fp64 value on this probe
    (test_hip_segtrain.reduction_bound's rule); a key dropped or doubled moves one by at least 4 / (n + 1), 1.2e-4 of 8
    at n = 4096.  Odd channels see the normaliser: exactly 1.0 in 16-bit storage (half a spacing at 1 is 2^-9 in bf16
    and 2^-12 in fp16, far above any fp32 error), the same rule in fp32.  One phantom key in the normaliser turns 1 into
    n / (n + 1), which leaves the 16-bit value 1.0 only while 1 / (n + 1) exceeds a quarter spacing below 1: in bf16
    for n <= 510, in fp16 for n <= 4094 -- n = 49, 324 and 400 are here for that; fp32 storage sees it at every n.
    Measured on the MI355X (printed per case): even and odd channels 0.00e+00 at all five sizes, every storage type and
    both routings (q = 0 makes every weight exactly 1 and the sums of v are exact integers in fp32; the kernels divide
    once at the end); fp32 torch on the same probe: even up to 3.4e-8 of 8, odd up to 7.2e-7 (4.2e-6 on a host whose
    torch sums in another order), 0 at n = 1024 and 4096, where 1 / n is a power of two."""
    p = P.attention_uniform(n)
    with routed(**ROUTE_SETS[route]):
        got = _attention(p.qkv, dtype).double()
    e_even = float(got[..., 0::2].abs().max()) / 8.0
    e_odd = float((got[..., 1::2] - 1.0).abs().max())
    print(f"uniform attention n={n} {dtype} {route}: even {e_even:.2e} (fp32 torch {p.d_even:.2e}, bound {max(1e-5, 4 * p.d_even):.2e}), "
          f"odd {e_odd:.2e} (fp32 torch {p.d_odd:.2e})")
    assert e_even <= max(1e-5, 4 * p.d_even)
    if dtype == "fp32":
        assert e_odd <= max(1e-5, 4 * p.d_odd)
    else:
        assert e_odd == 0.0


# ------------------------------------------------------------------------------------------------ 3d: fused linear attention
@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("C_,H,W", P.LINATTN_SHAPES)
def test_linattn_kvctx_uniform(dtype, C_, H, W):
    """ld_linattn_kvctx (+ _terms with two-term weights) -> ld_linattn_ctx_reduce on the uniform probe: zero k rows (P = 1
    for every pixel, in the two-sweep mode and with kshift = 0), v rows that select one +-1 channel.  The normalised
    context is mean_n v_e for every d: |ctxn - that| <= max(1e-5, 4 d) relative to |v| = 1, d = fp32 torch's distance on
    the same probe; a pixel lost or doubled at a chunk edge is 1 / (n + 1), 1.6e-4 at n = 6144 (24 chunks).  Then
    ld_linattn_ctxfold against reduce + fold on integer to_out weights: the same packed M_b.
    Measured on the MI355X (printed per mode): 0.00e+00 at all three shapes, both storage types, one and two weight terms,
    two-sweep and kshift (the rounding of v to storage absorbs the error of the reciprocal norm, so P and v enter the
    matrix pipe as exact powers of two and +-1); fp32 torch on the same probe 3.6e-7 .. 1.8e-6, bound 1e-5.  With the
    first pixel of every chunk but the first skipped, the same test reads 2.6e-3 at n = 784 (3 chunks) and 1.8e-3 at
    n = 6144 (24 chunks), where test_hip_ops.test_linear_attention_fused_16bit still passes at 64 x 96."""
    B, n = 2, H * W
    p = P.linattn_uniform(C_, H, W)
    lib, dt = cabi.lib(), cabi.dtype_code(dtype)
    xd = hh.nhwc(p.x, dtype)
    scale = p.scale.to(hh.DEV)
    w = p.w

    def pack_rows(rows, terms):
        rows = rows.to(hh.DEV, torch.float32).contiguous()
        out = hh.nans(terms * rows.numel(), dtype=hh.TDT[dtype])
        cabi.check(lib.ld_pack_conv_weight_terms(rows.data_ptr(), scale.data_ptr(), out.data_ptr(), rows.shape[0], C_, 1, 0, dt, terms,
                                                 hh.st()), "pack")
        return out
    wout = P.trits((C_, P.HID), 5100).to(hh.DEV)
    bound = max(1e-5, 4 * p.d)
    for terms in (1, 2):
        wkv = torch.cat([pack_rows(torch.cat([w[P.HID + 32 * h: P.HID + 32 * h + 32], w[2 * P.HID + 32 * h: 2 * P.HID + 32 * h + 32]], 0), terms)
                         for h in range(P.HEADS)]).contiguous()
        for single in (False, True):
            kshift = torch.zeros(P.HID, device=hh.DEV) if single else None
            nchunks = max(1, min(128, n // 512)) if single else max(1, min(32, n // 256))
            ctx = hh.nans(int(lib.ld_linattn_ctx_part_floats(B, P.HEADS, P.DH, nchunks)))
            ctxn = hh.nans(B, P.HEADS, P.DH, P.DH)
            cabi.check(lib.ld_linattn_kvctx_terms(xd.data_ptr(), wkv.data_ptr(), cabi.ptr(kshift), ctx.data_ptr(), B, n, C_, P.HEADS, P.DH,
                                                  nchunks, dt, terms, hh.st()), "kvctx")
            cabi.check(lib.ld_linattn_ctx_reduce(ctx.data_ptr(), nchunks, ctxn.data_ptr(), B, P.HEADS, P.DH, hh.st()), "reduce")
            e = float((ctxn.cpu().double() - p.ref).abs().max())
            print(f"linattn ctxn C={C_} n={n} {dtype} terms={terms} {'kshift' if single else 'two-sweep'} chunks={nchunks}: "
                  f"{e:.2e} (fp32 torch {p.d:.2e}, bound {bound:.2e})")
            assert e <= bound, (terms, single, e)
            wfold, wfold2 = hh.nans(B, C_ * P.HID, dtype=hh.TDT[dtype]), hh.nans(B, C_ * P.HID, dtype=hh.TDT[dtype])
            for perm in (0, 1):
                cabi.check(lib.ld_linattn_fold(ctxn.data_ptr(), wout.data_ptr(), wfold.data_ptr(), B, C_, P.HEADS, P.DH, perm, dt, hh.st()), "fold")
                cabi.check(lib.ld_linattn_ctxfold(ctx.data_ptr(), nchunks, wout.data_ptr(), wfold2.data_ptr(), B, C_, P.HEADS, P.DH, perm, dt,
                                                  hh.st()), "ctxfold")
                assert bool(torch.isfinite(wfold.float()).all())
                assert torch.equal(wfold2, wfold), (terms, single, perm)


LINOUT_CASES = [(C_, terms) for C_ in P.LINOUT_CHANNELS for terms in (1, 2) if (C_, terms) != (128, 2)]


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("n", P.LINOUT_SIZES)
@pytest.mark.parametrize("C_,terms", LINOUT_CASES)
def test_linattn_out_one_hot(dtype, C_, terms, n):
    """ld_linattn_out / _terms by itself (hip_helpers.linattn_out: chosen ctxn, M_b from ld_linattn_fold(perm = 1), W_q from
    ld_pack_conv_weight_terms) on the one-hot probe: softmax_d(q) switches on ONE k-slot per head, M_b is one head's block
    of W_out, the block's value y_c k_c + x is an integer -- torch.equal, with the per-pixel maximum and with qshift, one
    and two weight terms, a partial tile (n = 49), a tail whose last 16-pixel group holds 4 pixels (196), a 16-pixel tail
    (784) and full tiles (1024); the row behind the last pixel stays untouched and every pixel is written.
    Measured on the MI355X (printed per case): 0 outputs differ in all 40 cases, both shift modes -- the hardware rsq / rcp
    errors, if any, disappear in the roundings of q and of the output, as the builder's docstring argues.  With k-slots 4
    and 20 of every head exchanged in the perm = 1 mapping of ld_linattn_fold / _ctxfold (an in-bounds change, built on a
    scratch copy) this test fails in all 40 cases: 2.6 - 4.1 % of the outputs differ, by up to 8 -- exactly the outputs
    exact_probes.linout_swapped_slots predicts on the CPU (200 of 6272 at C = 32, n = 49; 641 of 25088 at n = 196) --,
    test_linattn_out_uniform passes all 40 (every k-slot carries 1 / 32), the random-operand test of test_hip_ops.py
    fails all 24 (e / d 4.7 - 75), and test_hip_ops.test_linear_attention_fused_16bit PASSES its four bf16 cases at
    C = 32 (it reads 1.6e-2 at 28 x 28 and 2.3e-2 at 64 x 96 against its 6e-2) and fails the other twelve (fp16 at C = 32
    by 1.6e-2 against 1.5e-2; C = 64 reads 8.1e-2, C = 128 2.0e-1)."""
    p = P.linout_onehot(C_, n)
    for qshift in (None, p.qshift):
        got = hh.linattn_out(p, dtype, terms, qshift)
        bad = got != p.ref
        print(f"linout one-hot C={C_} n={n} {dtype} terms={terms} {'qshift' if qshift is not None else 'max'}: {int(bad.sum())} of {bad.numel()} differ, "
              f"max |diff| {float((got - p.ref).abs().max()):.2e}")
        assert torch.equal(got, p.ref), (qshift is not None, int(bad.sum()), int(bad.any(1).sum()), "outputs / pixels differ")


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("n", P.LINOUT_SIZES)
@pytest.mark.parametrize("C_,terms", LINOUT_CASES)
def test_linattn_out_uniform(dtype, C_, terms, n):
    """W_q = 0: softmax_d(q) = 1 / 32 on all 128 k-slots (with the max reduction and with qshift = 0), M_b = W_out with
    permuted columns (+-1): the second product is a row sum of 128 terms / 32, exact in any order; torch.equal.
    Measured on the MI355X: 0 outputs differ in all 40 cases, with the max reduction and with qshift = 0."""
    p = P.linout_uniform(C_, n)
    for qshift in (None, p.qshift):
        got = hh.linattn_out(p, dtype, terms, qshift)
        bad = got != p.ref
        print(f"linout uniform C={C_} n={n} {dtype} terms={terms} {'qshift' if qshift is not None else 'max'}: {int(bad.sum())} of {bad.numel()} differ, "
              f"max |diff| {float((got - p.ref).abs().max()):.2e}")
        assert torch.equal(got, p.ref), (qshift is not None, int(bad.sum()))


@pytest.mark.parametrize("dtype", LOWP)
def test_linattn_out_refuses_two_terms_at_128_channels(dtype):
    """Two-term W_q is built for C = 32 / 64: C = 128 returns -1 and writes nothing (the NaN-filled output and the row
    behind it are as they were)."""
    hh.linattn_out(P.linout_uniform(128, 49), dtype, terms=2, expect_refusal=True)
