"""A plan's 3x3 labels are the library's routing decision, not a copy of it: every launch of ``ops_main`` whose ``meta``
carries a ``route`` (asked of ld_conv3x3_route when the plan was built) must report that word through ld_last_route when it
runs, and its ``family`` -- what bench.py groups the roofline table, picks the ResBlock conv path and looks the committed
counter traffic up by -- must be that word's spelling.  Also under a Tuning that moves the thresholds, where the plan
builder's old hand-kept rule filed launches under kernels that did not run (docs/findings.md)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import localdiffusion_hallucination_amd as ldh                   # noqa: E402
from localdiffusion_hallucination_amd import _cabi as cabi       # noqa: E402
from localdiffusion_hallucination_amd import rng, weights        # noqa: E402
from localdiffusion_hallucination_amd.tuning import Tuning        # noqa: E402
import hip_helpers as hh                                           # noqa: E402
from test_hip_conv_tiles import routed                             # noqa: E402

MRI = dict(mode="mri")
MNIST = dict(dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist")
DNAME = {"fp32": "f32", "bf16": "bf16", "fp16": "f16"}


def spelled(r, dtype):
    d = DNAME[dtype]
    return {"generic": f"conv3x3<{d},{r['MT']},{r['NW']}>", "lean": f"conv3x3_s32<{d}>", "persistent": f"conv3x3_c32<{d}>"}[r["family"]]


def run_launch_by_launch(kw, dtype, H, tuning=None):
    """Build the sampler plan, run the encoder, the step-begin launch as bench.conv_path_chip_leg issues it, then ops_main one
    launch at a time -> the families of the routed launches, each confirmed against what ran."""
    net = ldh.Unet(dim=32, init_dim=32, compute_dtype=dtype, tuning=tuning, **kw)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.procedural_state_dict(net.cfg, 0).items()})
    net = net.to("cuda")
    plan = net.plan(1, H, H, table_T=4)
    lib, st = cabi.lib(), hh.st()
    plan.x_in.copy_(torch.from_numpy(rng.randn(tuple(plan.x_in.shape), 1, 7)))
    plan.cond_in.copy_(torch.from_numpy(rng.uniform(tuple(plan.cond_in.shape), 1, 8, 0.0, 2.0)))
    plan.run_cond(st)
    cabi.check(lib.ld_step_begin_film(*plan._begin_args, plan._t_dev_ptr, 0, None, None, *plan._film_args, st), "step_begin")
    fams = []
    assert sorted(plan.meta) == list(range(len(plan.ops_main)))
    for i, op in enumerate(plan.ops_main):
        op(st)
        m = plan.meta[i]
        assert ("route" in m) == m["what"].startswith("conv3x3 "), m
        if "route" in m:
            assert int(lib.ld_last_route(cabi.ROUTE_CONV3X3)) == m["route"], (i, m, hh.last_route(cabi.ROUTE_CONV3X3))
            assert m["family"] == spelled(hh.last_route(cabi.ROUTE_CONV3X3), dtype), (i, m)
            fams.append(m["family"])
    torch.cuda.synchronize()
    assert torch.isfinite(plan.model_out).all()
    return fams


@pytest.mark.parametrize("kw,dtype,H", [(MRI, "bf16", 64), (MRI, "fp32", 64), (MNIST, "fp16", 28)], ids=["mri-bf16", "mri-fp32", "mnist-fp16"])
def test_plan_labels_are_what_runs(kw, dtype, H):
    fams = run_launch_by_launch(kw, dtype, H)
    assert len(fams) >= 20 and all(f.startswith("conv3x3<") for f in fams), fams      # (maps this small stay on the generic kernel)


def test_plan_labels_follow_a_tuning_that_moves_the_thresholds():
    """conv_big_min = 1 puts every 32-channel-tile launch of a map of 16 rows or more on <2,4>; conv_s32 = 7 with
    conv_s32_min_tiles = 1 (so that the mask shows on a 64^2 map of one image) hands the Cout = 32 launches on whole 16 x 16
    tiles to the lean kernel, two-chunk ones included.  The old rule hard-coded 512 for the first and had its own conditions
    for the second."""
    with routed():                                                 # the net's Tuning.kernel lands in the process-wide table: put it back
        moved = run_launch_by_launch(MRI, "bf16", 64, Tuning.from_env(kernel=dict(conv_big_min=1, conv_s32=7, conv_s32_min_tiles=1)))
    default = run_launch_by_launch(MRI, "bf16", 64)
    assert len(moved) == len(default)
    assert "conv3x3_s32<bf16>" in moved and "conv3x3<bf16,2,4>" in moved, moved
    assert "conv3x3_s32<bf16>" not in default and "conv3x3<bf16,2,4>" not in default, default
