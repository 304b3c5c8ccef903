"""Training the segmentation U-Net, the parts that need no GPU: the plain-PyTorch restatement of the step
(tests/segtrain_ref.py) in fp64 against the reference's own fp64 run (golden G19), argument validation of every new
entry point, SegTrainer's refusals and its epoch bookkeeping with the GPU calls stubbed, and the weight-gradient
kernel's matrix-core instruction in the compiled code."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import checkpoint, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segtrain_ref                                                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "localdiffusion-hallucination_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def g19():
    g = np.load(os.path.join(GOLD, "g19_segtrain.npz"))
    small = np.load(os.path.join(GOLD, "g19_segtrain_grads.npz"))
    sd = weights.procedural_seg_state_dict(int(g["seed"]))
    batches = [(torch.from_numpy(g["x"][b]), torch.from_numpy(g["target"][b].astype(np.float32))) for b in range(g["x"].shape[0])]
    return g, small, sd, batches


def close(got, ref, rtol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max()) <= rtol * max(float(np.abs(ref).max()), 1e-300)


def test_g19_fixture_shape_and_the_references_own_tight_tier():
    g, small, sd, batches = g19()
    assert g["x"].shape == (6, 4, 1, 32, 32) and g["target"].shape == (6, 4, 1, 32, 32)
    assert 0.005 < float(g["target"].mean()) < 0.2
    assert g["grad_norm"].shape == (6, 64) and g["grad_dots"].shape == (6, 64, 4) and g["clean"].shape == (3, 6)
    # each of the reference's three fp32 orders: on at least two batches at least 32 parameters within 1e-4 of fp64
    for o in range(3):
        assert int((g["clean"][o] >= 32).sum()) >= 2, g["clean"]
    assert float(g["loss_steps"][-1]) < 0.8 * float(g["loss_steps"][0])
    for name in ("g19_segtrain.npz", "g19_segtrain_grads.npz"):
        assert os.path.getsize(os.path.join(GOLD, name)) < 1000000


def test_restatement_in_fp64_reproduces_the_reference_at_the_initial_weights():
    g, small, sd, batches = g19()
    cache = {}
    for b, (x, t) in enumerate(batches):
        params, buffers = segtrain_ref.params_of(sd, torch.float64)
        stats = {}
        loss, grads = segtrain_ref.loss_and_grads(params, buffers, x, t, update_running=False, stats=stats)
        assert abs(float(loss) - float(g["loss_init"][b])) <= 1e-10 * abs(float(g["loss_init"][b]))
        for k, v in buffers.items():                           # untouched
            assert torch.equal(v, torch.as_tensor(sd[k]).to(v.dtype)), k
        for k, v in stats.items():
            assert close(v.numpy(), g[f"bn{b}.{k}"], 1e-9), (b, k)
        assert len(grads) == 64
        for i, (name, gr) in enumerate(grads.items()):
            assert abs(float(gr.norm()) - g["grad_norm"][b, i]) <= 1e-9 * g["grad_norm"][b, i], (b, name)
            scale = g["grad_norm"][b, i] * np.sqrt(gr.numel() / 3.0)       # |dot| of a uniform(-1, 1) probe is about this
            assert np.abs(np.asarray(segtrain_ref.probe_dots(i, gr, cache)) - g["grad_dots"][b, i]).max() <= 1e-9 * scale, (b, name)
            if gr.numel() <= 4096:
                assert close(gr.numpy(), small[f"grad{b}.{name}"], 1e-9), (b, name)


def test_restatement_in_fp64_reproduces_the_six_adam_steps():
    g, small, sd, batches = g19()
    losses, first, params, buffers = segtrain_ref.train_steps(sd, batches, torch.float64)
    for got, ref in zip(losses, g["loss_steps"]):
        assert abs(got - float(ref)) <= 1e-10 * abs(float(ref)), (losses, g["loss_steps"])
    for k, v in first.items():
        ref = g["step1." + k]
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref) == 1
        else:
            assert close(v.numpy(), ref, 1e-9), k


def test_adam_restatement_matches_torch_optim():
    torch.manual_seed(0)
    p0 = {"a": torch.randn(7, 5, dtype=torch.float64), "b": torch.randn(11, dtype=torch.float64)}
    mine = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    theirs = [v.clone().requires_grad_(True) for v in p0.values()]
    opt, ref = segtrain_ref.Adam(mine), torch.optim.Adam(theirs, lr=1e-3)
    for s in range(3):
        grads = {k: torch.randn_like(v) for k, v in p0.items()}
        for t, gk in zip(theirs, grads.values()):
            t.grad = gk.clone()
        opt.step(grads)
        ref.step()
    for m, t in zip(mine.values(), theirs):
        assert torch.allclose(m, t, rtol=1e-14, atol=0)


def test_argument_validation_of_every_new_entry_point_needs_no_gpu():
    lib = cabi.lib()
    one = 4096        # a non-null "pointer": validation happens before any use

    def adam(count=None, beta1=0.9, bc2_sqrt=0.03, second=None, **fields):
        """ld_seg_adam on a table of valid [2][2][2] entries (one, or two with ``second``) with the given fields changed."""
        arr = (cabi.SegAdamTensor * 2)()
        for a, changed in zip(arr, (fields, second or {})):
            a.param = a.grad = a.m = a.v = one
            a.d0 = a.d1 = a.d2 = 2
            for k, v in changed.items():
                setattr(a, k, v)
        n = (2 if second else 1) if count is None else count
        return lib.ld_seg_adam(arr, n, beta1, 0.999, 1e-8, 1e-3, bc2_sqrt, None)
    bad = [
        ("ld_seg_wgrad", lambda: lib.ld_seg_wgrad(one, one, one, one, 1, 16, 16, 48, 64, 3, 1, None), b"Cin"),
        ("ld_seg_wgrad", lambda: lib.ld_seg_wgrad(one, one, one, one, 1, 16, 16, 64, 64, 2, 1, None), b"ksize"),
        ("ld_seg_wgrad", lambda: lib.ld_seg_wgrad(one, one, one, one, 1, 16, 16, 64, 64, 3, 9, None), b"splits"),
        ("ld_seg_wgrad", lambda: lib.ld_seg_wgrad(None, one, one, one, 1, 16, 16, 64, 64, 3, 1, None), b"null"),
        ("ld_seg_bn_train", lambda: lib.ld_seg_bn_train(one, one, one, one, one, None, None, 0.1, 1e-5, one, 256, 40, None), b"C 40"),
        ("ld_seg_bn_train", lambda: lib.ld_seg_bn_train(one, one, one, one, one, None, None, 0.1, 1e-5, one, 1, 64, None), b"two"),
        ("ld_seg_bn_train", lambda: lib.ld_seg_bn_train(one, one, one, one, one, one, None, 0.1, 1e-5, one, 256, 64, None), b"running"),
        ("ld_seg_bn_backward", lambda: lib.ld_seg_bn_backward(one, one, one, one, one, one, one, one, one, 0, 64, None), b"M 0"),
        ("ld_seg_bn_backward", lambda: lib.ld_seg_bn_backward(one, None, one, one, one, one, one, one, one, 4, 64, None), b"null"),
        ("ld_seg_colsum", lambda: lib.ld_seg_colsum(one, one, one, 16, 64, 3, None), b"fold"),
        ("ld_seg_pool", lambda: lib.ld_seg_pool(one, one, 1, 8, 8, 6, None), b"C=6"),
        ("ld_seg_pool_backward", lambda: lib.ld_seg_pool_backward(one, one, None, one, 1, 0, 8, 64, None), b"H=0"),
        ("ld_seg_cat_d2s", lambda: lib.ld_seg_cat_d2s(one, one, one, 1, 7, 8, 64, 64, None), b"even"),
        ("ld_seg_cat_d2s_backward", lambda: lib.ld_seg_cat_d2s_backward(one, one, one, 1, 8, 8, 64, 0, None), b"C1 0"),
        ("ld_seg_loss", lambda: lib.ld_seg_loss(one, one, one, one, None, 0, 10.0, 1e-5, None), b"0 logits"),
        ("ld_seg_loss", lambda: lib.ld_seg_loss(one, None, one, one, None, 16, 10.0, 1e-5, None), b"null"),
        ("ld_seg_head_backward", lambda: lib.ld_seg_head_backward(one, one, one, one, one, one, one, 16, 60, None), b"C 60"),
        ("ld_seg_adam", lambda: adam(count=0), b"tensors"),
        ("ld_seg_adam", lambda: adam(count=cabi.SEG_ADAM_MAX + 1), b"tensors"),
        ("ld_seg_adam", lambda: adam(d0=0), b"empty shape"),
        ("ld_seg_adam", lambda: adam(param=None), b"null"),
        ("ld_seg_adam", lambda: adam(gs1=-1), b"negative gradient stride"),
        ("ld_seg_adam", lambda: adam(mirror0=one, m0_s2=-1), b"mirror0"),
        ("ld_seg_adam", lambda: adam(mirror1=one, m1_off=3, m1_s0=-4), b"mirror1"),
        ("ld_seg_adam", lambda: adam(beta1=1.5), b"betas"),
        ("ld_seg_adam", lambda: adam(bc2_sqrt=0.0), b"betas"),
        ("ld_seg_adam", lambda: adam(second=dict(d2=0)), b"tensor 1 has an empty shape"),      # the whole table, not the first entry
        ("ld_seg_permute3", lambda: lib.ld_seg_permute3(one, one, 2, 2, 9, 0, 1, 18, -2, None), b"negative"),
        ("ld_seg_permute3", lambda: lib.ld_seg_permute3(one, one, 2, 0, 9, 0, 1, 18, 2, None), b"shape"),
    ]
    for name, call, word in bad:
        assert call() == -1, name
        assert word in lib.ld_last_error(), (name, lib.ld_last_error())
    assert {n for n, _, _ in bad} == {n for n in cabi.EXPORTS if n.startswith("ld_seg_") and n not in (
        "ld_seg_conv", "ld_seg_conv_image", "ld_seg_head", "ld_seg_pack_weight", "ld_seg_pack_convt", "ld_seg_wgrad_splits")}
    # the split count: 0 for a refused shape; fills the chip at the top level, one split where the tiles alone do
    assert lib.ld_seg_wgrad_splits(1, 16, 16, 48, 64, 3) == 0
    assert lib.ld_seg_wgrad_splits(32, 256, 256, 64, 64, 3) == 228
    assert lib.ld_seg_wgrad_splits(2, 16, 16, 1024, 1024, 3) == 1
    assert 1 <= lib.ld_seg_wgrad_splits(1, 16, 16, 64, 64, 3) <= 8        # never more splits than chunks of 32 pixels


def test_struct_layout_matches_the_header():
    src = open(os.path.join(ROOT, "include", "localdiff_hip.h")).read()
    body = re.search(r"typedef struct ld_seg_adam_tensor \{(.*?)\} ld_seg_adam_tensor;", src, flags=re.S).group(1)
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            names = decl.split(",")
            fields.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)$", names[0].strip())[0])
            fields += [n.strip() for n in names[1:]]
    assert [f[0] for f in cabi.SegAdamTensor._fields_] == fields
    assert C.sizeof(cabi.SegAdamTensor) == 152                 # the header's "152-byte entry"
    for name, value in (("GROUP", cabi.SEG_ADAM_GROUP), ("MAX", cabi.SEG_ADAM_MAX)):
        assert int(re.search(rf"#define LD_SEG_ADAM_{name} (\d+)", src).group(1)) == value


def test_reduction_scratch_size_matches_the_header():
    from localdiffusion_hallucination_amd import segtrain
    src = open(os.path.join(ROOT, "include", "localdiff_hip.h")).read()
    expr = re.search(r"#define LD_SEG_RED_WORK_BYTES \(([0-9 *]+)\)", src).group(1)
    assert segtrain.RED_WORK_BYTES == eval(expr)


def test_trainer_refusals():
    with pytest.raises(ValueError, match="fp32"):
        ldh.SegTrainer(ldh.SegUNet(compute_dtype="bf16"))
    with pytest.raises(TypeError):
        ldh.SegTrainer(torch.nn.Linear(2, 2))
    net = ldh.SegUNet().train()
    net.set_compute_dtype("fp16")
    with pytest.raises(ValueError, match="fp32"):
        net(torch.zeros(2, 1, 32, 32))
    net.set_compute_dtype("fp32")
    with pytest.raises(ValueError, match="multiples of 16"):
        net(torch.zeros(2, 1, 40, 32))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            net(torch.zeros(2, 1, 32, 32))
        with pytest.raises(RuntimeError, match="GPU"):
            ldh.SegTrainer(net).step(torch.zeros(2, 1, 32, 32), torch.zeros(2, 1, 32, 32))


def test_fit_keeps_the_best_dice_state_dict(tmp_path):
    net = ldh.SegUNet()
    tr = ldh.SegTrainer(net)
    dices = iter([0.2, 0.4, 0.5, 0.7, 0.3, 0.1])         # two validation batches per epoch: means 0.3, 0.6, 0.2
    calls = {"step": 0}

    def step(x, t):
        calls["step"] += 1
        with torch.no_grad():
            net.outc.conv.bias.fill_(float(calls["step"]))      # "training": the bias counts the steps
        return torch.tensor(1.0 / calls["step"])

    tr.step, tr.evaluate = step, lambda x, t: (next(dices), 0.5)
    z = torch.zeros(1, 1, 16, 16)
    out = str(tmp_path / "best_dice.pth")
    res = tr.fit([(z, z)] * 3, [(z, z)] * 2, epochs=3, out_path=out, log=str(tmp_path))
    assert res["best_epoch"] == 1 and abs(res["best_dice"] - 0.6) < 1e-12
    assert [r[0] for r in res["val"]] == [0, 1, 2] and abs(res["train"][0][1] - (1 + 1 / 2 + 1 / 3) / 3) < 1e-6
    fresh = ldh.SegUNet()
    assert checkpoint.load_seg_checkpoint(out, fresh) == {"n_tensors": 118}
    assert float(fresh.outc.conv.bias.detach()) == 6.0                  # the state after epoch 1 (six steps), not the last one
    rows = open(tmp_path / "val.csv").read().strip().splitlines()
    assert rows[0] == "epoch,dice,bce" and len(rows) == 4
    assert open(tmp_path / "train.csv").read().startswith("epoch,loss")


def test_fit_asks_a_callable_for_each_epochs_batches(tmp_path):
    tr = ldh.SegTrainer(ldh.SegUNet())
    seen = []
    tr.step = lambda x, t: seen.append(int(x)) or torch.tensor(1.0)
    tr.evaluate = lambda x, t: (0.5, 0.5)
    z = torch.zeros(1)
    tr.fit(lambda e: [(torch.tensor(10 * e + i), z) for i in range(2)], [(z, z)], epochs=3, out_path=str(tmp_path / "b.pth"))
    assert seen == [0, 1, 10, 11, 20, 21]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_weight_gradient_kernel_runs_on_the_matrix_cores(tmp_path):
    out = str(tmp_path / "segtrain.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mllvm", "-amdgpu-mfma-vgpr-form",
           "-S", "--cuda-device-only", os.path.join(CSRC, "segtrain.hip"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=CSRC)
    asm = open(out).read()
    m = re.search(r"^(_Z\w*seg_wgrad_kernel\w*):[^\n]*\n(.*?)\n\s*s_endpgm", asm, flags=re.S | re.M)
    assert m, "seg_wgrad_kernel not found in the assembly"
    body = m.group(2)
    assert body.count("v_mfma_f32_32x32x2_f32") >= 16, body.count("v_mfma")
    assert "global_atomic" not in body                         # slabs + an ordered reducer, no atomics
