"""ld_conv3x3_route on the CPU: the routing decision ld_conv3x3 launches by, asked without launching.  Pointers are only
tested for null, so the argument blocks here carry made-up addresses; nothing touches a GPU.  The GPU side of the same
contract -- the word equals ld_last_route after the launch -- is asserted by tests/hip_helpers.conv3x3 on every 3x3 test."""
import ctypes as C

import pytest

from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd.unet import conv3x3_family
from test_hip_conv_tiles import NEVER, TILES, TILE_ID, routed, sets3

FAKE = 0x10000          # a non-null "device pointer"
DTYPES = ["fp32", "bf16", "fp16"]


def block(dtype, cins, cout, h, w, B, gn=False):
    a = cabi.Conv3x3Args()
    a.nsrc = len(cins)
    for i, c in enumerate(cins):
        a.src[i].data, a.src[i].C = FAKE, c
        if gn:
            a.src[i].gn_stats, a.src[i].gn_gamma, a.src[i].gn_beta, a.src[i].gn_groups = FAKE, FAKE, FAKE, 8
    a.weight, a.bias, a.out = FAKE, FAKE, FAKE
    a.B, a.H, a.W, a.Cout, a.dtype = B, h, w, cout, cabi.dtype_code(dtype)
    return a


def decode(word):
    assert word >= 0, (word, cabi.lib().ld_last_error())
    return dict(family={0: "generic", 1: "lean", 2: "persistent"}[word & 15], MT=(word >> 4) & 15, NW=(word >> 8) & 15,
                raw=bool((word >> 12) & 1), sk=bool((word >> 13) & 1), side=bool((word >> 14) & 1))


def route(a):
    return decode(int(cabi.lib().ld_conv3x3_route(C.byref(a))))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", TILES, ids=[TILE_ID[t] for t in TILES])
def test_forcing_entries_select_the_tile_on_a_small_map(tile, dtype):
    """The entries test_hip_conv_tiles forces a tile with work on a 16 x 16 map of one image: that is what forcing is for."""
    a = block(dtype, [32], 64, 16, 16, 1)
    with routed(**sets3(tile)):
        assert route(a) == dict(family="generic", MT=tile[0], NW=tile[1], raw=True, sk=False, side=False)
    with routed(**sets3(tile, conv_raw=0)):
        assert route(a)["raw"] is False


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_default_routing_of_the_bench_shape(dtype):
    """What test_hip_bench_shape.py pins with launch counters, from the query: 32 -> 32 at 256^2, B = 4 on the lean kernel (with
    and without the GroupNorm prologue), 64 -> 32 on the generic one, the persistent kernel retired -- and the labels follow
    the table where the plan builder's old Python rule could not (it never read conv_big_min / conv_mt4_min_wgs)."""
    lib = cabi.lib()
    one, one_gn, two = block(dtype, [32], 32, 256, 256, 4), block(dtype, [32], 32, 256, 256, 4, gn=True), block(dtype, [32, 32], 32, 256, 256, 4)
    defaults = dict(conv_s32=3, conv_s32_min_tiles=1024, conv_c32=0, conv_c32_min_tiles=2048, conv_raw=1, conv_sk=0, conv_mt4_min_wgs=256,
                    conv_big_min=512, conv_big4_min=256)                 # the header's defaults, whatever the environment says
    with routed(**defaults):
        assert route(one) == dict(family="lean", MT=2, NW=4, raw=True, sk=False, side=False)
        assert route(one_gn) == dict(family="lean", MT=2, NW=4, raw=False, sk=False, side=False)
        assert route(two) == dict(family="generic", MT=2, NW=4, raw=True, sk=False, side=False)
        assert conv3x3_family(int(lib.ld_conv3x3_route(C.byref(one))), one.dtype) == f"conv3x3_s32<{'bf16' if dtype == 'bf16' else 'f16'}>"
        assert conv3x3_family(int(lib.ld_conv3x3_route(C.byref(two))), two.dtype) == f"conv3x3<{'bf16' if dtype == 'bf16' else 'f16'},2,4>"
        cabi.check(lib.ld_tuning_set(b"conv_s32", 0), "tuning_set")
        assert route(one) == dict(family="generic", MT=2, NW=4, raw=True, sk=False, side=False)
        assert route(one_gn) == dict(family="generic", MT=2, NW=4, raw=False, sk=False, side=False)
        cabi.check(lib.ld_tuning_set(b"conv_big_min", NEVER), "tuning_set")
        assert route(one) == dict(family="generic", MT=2, NW=2, raw=True, sk=False, side=False)
        cabi.check(lib.ld_tuning_set(b"conv_c32", 1), "tuning_set")          # the persistent kernel: 1,024 tiles < 2,048 ...
        assert route(one)["family"] == "generic"
        cabi.check(lib.ld_tuning_set(b"conv_c32_min_tiles", 1024), "tuning_set")
        assert route(one) == dict(family="persistent", MT=2, NW=4, raw=True, sk=False, side=False)
        assert route(two)["family"] == "generic"                             # ... and never two K-chunks


def test_refusals_are_the_launch_functions_and_leave_the_last_route_alone():
    lib = cabi.lib()
    before = lib.ld_last_route(cabi.ROUTE_CONV3X3)
    cases = []
    a = block("bf16", [32], 64, 16, 16, 1)
    a.nsrc = 3
    cases.append((a, b"nsrc"))
    a = block("bf16", [32], 48, 16, 16, 1)
    cases.append((a, b"Cout"))
    a = block("bf16", [32], 64, 16, 16, 1)
    a.weight = None
    cases.append((a, b"null weight"))
    for a, msg in cases:
        rc = int(lib.ld_conv3x3_route(C.byref(a)))
        assert rc == -1 and msg in lib.ld_last_error(), (rc, lib.ld_last_error())
        said = lib.ld_last_error()
        assert lib.ld_conv3x3(C.byref(a), None) == rc and lib.ld_last_error() == said
    assert route(block("bf16", [32], 64, 16, 16, 1))["family"] == "generic"      # an accepted query does not move it either
    assert lib.ld_last_route(cabi.ROUTE_CONV3X3) == before
