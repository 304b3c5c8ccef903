"""The MNIST digit classifier and its training, the parts that need no GPU: the public names, the reference's parameter
inventory and the checkpoint round trip, the plain-PyTorch restatement (tests/mnistcls_ref.py) in fp64 against the
reference's own fp64 run (golden G20), the flatten order, the pooling tie rule, ``fit``'s bookkeeping with the GPU calls
stubbed, the documented refusals and the argument validation of every ``ld_mc_*`` entry point.

G20 holds every tensor of up to 32,768 elements whole; ``fc1.weight`` (401,408 elements, over the size limit of a
committed file in fp64) as its norm, four probe dot products and a sample of 4,096 elements at a stride of 97."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import checkpoint, rng, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mnistcls_ref                                                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RTOL = 1e-12


def g20():
    g = np.load(os.path.join(GOLD, "g20_mnistcls.npz"))
    grads = np.load(os.path.join(GOLD, "g20_mnistcls_grads.npz"))
    d = np.load(os.path.join(GOLD, "g20_mnist_digits.npz"))
    sd = weights.procedural_mnistcls_state_dict(int(g["seed"]))
    x, y = mnistcls_ref.images_of(d["images"]), torch.from_numpy(d["labels"].astype(np.int64))
    return g, grads, sd, x, y


def close(got, ref, rtol=RTOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return got.shape == ref.shape and float(np.abs(got - ref).max()) <= rtol * max(float(np.abs(ref).max()), 1e-300)


def matches_fixture(t, store, prefix):
    """A tensor against what G20 holds of it (whole, or norm + probe dots + sample)."""
    t = t.detach().double().contiguous()
    if prefix in store.files:
        return close(t.numpy(), store[prefix])
    flat = t.reshape(-1)
    norm = float(store[prefix + ".norm"])
    dots = [float(torch.dot(flat, torch.from_numpy(rng.uniform((flat.numel(),), 2020 + j, 20, -1.0, 1.0)).double()))
            for j in range(4)]
    scale = norm * np.sqrt(flat.numel() / 3.0)                 # |dot| of a uniform(-1, 1) probe is about this
    return (abs(float(flat.norm()) - norm) <= RTOL * norm and np.abs(np.asarray(dots) - store[prefix + ".dots"]).max() <= 1e-11 * scale
            and close(flat[::97][:4096].numpy(), store[prefix + ".sample"]))


# ------------------------------------------------------------------------------------------------ public surface
def test_public_names_exist_and_import_loads_no_library():
    assert ldh.MnistClassifier.__name__ == "MnistClassifier" and ldh.MnistClassifierTrainer.__name__ == "MnistClassifierTrainer"
    assert "MnistClassifier" in ldh.__all__ and "MnistClassifierTrainer" in ldh.__all__
    code = ("import sys; sys.path.insert(0, %r); import localdiffusion_hallucination_amd as l; "
            "from localdiffusion_hallucination_amd import _cabi; assert _cabi._lib is None; "
            "assert 'localdiffusion_hallucination_amd.mnistcls' not in sys.modules; l.MnistClassifier; l.MnistClassifierTrainer; "
            "assert _cabi._lib is None; print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_parameter_inventory_is_the_references():
    net = ldh.MnistClassifier()
    want = [("conv1.weight", (32, 1, 3, 3)), ("conv1.bias", (32,)), ("conv2.weight", (64, 32, 3, 3)), ("conv2.bias", (64,)),
            ("fc1.weight", (128, 3136)), ("fc1.bias", (128,)), ("fc2.weight", (10, 128)), ("fc2.bias", (10,))]
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == want
    assert [(k, tuple(v.shape)) for k, v in net.named_parameters()] == want
    assert list(weights.mnistcls_param_shapes().items()) == want
    assert (net.conv1.padding, net.conv2.padding, net.conv1.stride) == ((1, 1), (1, 1), (1, 1))
    sd = weights.procedural_mnistcls_state_dict(3)
    for k, shape in want:                                      # PyTorch's default bounds: 1 / sqrt(fan_in)
        fan_in = int(np.prod(dict(want)[k.rsplit(".", 1)[0] + ".weight"][1:]))
        assert sd[k].dtype == np.float32 and sd[k].shape == shape
        assert 0.9 / np.sqrt(fan_in) < np.abs(sd[k]).max() <= 1.0 / np.sqrt(fan_in), k
    assert not np.array_equal(sd["fc2.bias"], weights.procedural_mnistcls_state_dict(4)["fc2.bias"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert torch.equal(net.fc1.weight, torch.from_numpy(sd["fc1.weight"]))


def test_checkpoint_round_trip_unsafe_pickle_and_shape_mismatch(tmp_path):
    src = ldh.MnistClassifier()
    src.load_state_dict({k: torch.from_numpy(v) for k, v in weights.procedural_mnistcls_state_dict(5).items()})
    path = str(tmp_path / "cls.pth")
    torch.save(src.state_dict(), path)                        # as train_mnist_cls.py:116 does
    dst = ldh.MnistClassifier()
    assert checkpoint.load_mnist_classifier(path, dst) == {"n_tensors": 8}
    for k, v in src.state_dict().items():
        assert torch.equal(v, dst.state_dict()[k]), k
    wrapped = {"module." + k: v for k, v in src.state_dict().items()}
    assert checkpoint.load_mnist_classifier(wrapped, ldh.MnistClassifier())["n_tensors"] == 8

    class Evil:
        def __reduce__(self):
            return (print, ("arbitrary code ran",))
    evil = str(tmp_path / "evil.pth")
    torch.save({"conv1.weight": Evil()}, evil)
    with pytest.raises(RuntimeError, match="restricted unpickler"):
        checkpoint.load_mnist_classifier(evil, dst)
    bad = dict(src.state_dict())
    bad["fc1.weight"] = torch.zeros(128, 3137)
    with pytest.raises(RuntimeError, match="fc1.weight"):
        checkpoint.load_mnist_classifier(bad, dst)
    short = {k: v for k, v in src.state_dict().items() if k != "fc2.bias"}
    with pytest.raises(RuntimeError, match="fc2.bias"):
        checkpoint.load_mnist_classifier(short, dst)
    not_a_dict = str(tmp_path / "list.pth")
    torch.save([torch.zeros(1)], not_a_dict)
    with pytest.raises(RuntimeError, match="state_dict"):
        checkpoint.load_mnist_classifier(not_a_dict, dst)


def test_cache_control_follows_patchcore():
    net = ldh.MnistClassifier()
    net._packed = "stale"
    net.invalidate()
    assert net._packed is None
    net._packed = "stale"
    net.to(torch.float32)
    assert net._packed is None
    net._packed = "stale"
    net.load_state_dict(net.state_dict())
    assert net._packed is None


# ------------------------------------------------------------------------------------------------ the restatement against G20
def test_g20_fixture_shape_and_generation_time_conditions():
    g, grads, sd, x, y = g20()
    assert x.shape == (1536, 1, 28, 28) and y.shape == (1536,) and int(y.min()) == 0 and int(y.max()) == 9
    assert float(x.min()) == 0.0 and float(x.max()) == 2.0
    assert g["loss_steps"].shape == (48,) and g["test_logits"].shape == (512, 10) and g["logits_init"].shape == (64, 10)
    assert float(g["accuracy"]) > 0.80 and float(g["loss_steps"][-1]) < 0.5 * float(g["loss_steps"][0])
    assert int(g["left_out"]) <= 0.02 * 512
    # the reference's own fp32 run from weights one ulp away stays within the bound the GPU test uses: the block is one on
    # which a 48-step comparison can tell a correct fp32 implementation from a wrong one
    assert g["moved_loss_err"].shape == (6,) and float(g["moved_loss_err"].max()) <= 4.0 * float(g["loss_spread"])
    for k in ("grad_spread", "loss_spread", "logit_spread"):
        assert 0.0 < float(g[k]) < 1e-2, k
    for name in ("g20_mnistcls.npz", "g20_mnistcls_grads.npz", "g20_mnist_digits.npz"):
        assert os.path.getsize(os.path.join(GOLD, name)) < 1000000


def test_restatement_in_fp64_reproduces_the_references_logits_and_gradients():
    g, grads, sd, x, y = g20()
    params = mnistcls_ref.params_of(sd, torch.float64)
    assert close(mnistcls_ref.forward(params, x[:64].double()).detach().numpy(), g["logits_init"])
    for b in range(3):
        loss, gr = mnistcls_ref.loss_and_grads(mnistcls_ref.params_of(sd, torch.float64), x[64 * b:64 * b + 64], y[64 * b:64 * b + 64])
        assert abs(float(loss) - float(g["loss_init"][b])) <= RTOL * abs(float(g["loss_init"][b]))
        assert list(gr.keys()) == list(sd.keys())
        for k, v in gr.items():
            assert matches_fixture(v, grads, f"grad{b}.{k}"), (b, k)


def test_restatement_in_fp64_reproduces_the_48_adam_steps():
    g, grads, sd, x, y = g20()
    batches = mnistcls_ref.epoch_batches(x[:1024], y[:1024], 3)
    losses, kept, params = mnistcls_ref.train_steps(sd, batches, torch.float64, keep=(1, 48))
    assert len(losses) == 48
    for got, ref in zip(losses, g["loss_steps"]):
        assert abs(got - float(ref)) <= RTOL * abs(float(ref))
    for step in (1, 48):
        for k, v in kept[step].items():
            assert matches_fixture(v, g, f"step{step}.{k}"), (step, k)
    logits = mnistcls_ref.forward(params, x[1024:].double()).detach()
    assert close(logits.numpy(), g["test_logits"])
    assert abs(float((logits.argmax(1) == y[1024:]).double().mean()) - float(g["accuracy"])) < 1e-12


def test_explicit_adam_is_torch_optim_adam():
    p0 = torch.from_numpy(rng.uniform((50,), 1, 2, -1.0, 1.0)).double()
    mine = {"p": p0.clone().requires_grad_(True)}
    theirs = p0.clone().requires_grad_(True)
    opt, ref = torch.optim.Adam([theirs], lr=1e-3), mnistcls_ref.Adam(mine)
    for t in range(4):
        gr = torch.from_numpy(rng.uniform((50,), 3 + t, 4, -1.0, 1.0)).double() * 10.0 ** (-t)
        theirs.grad = gr.clone()
        opt.step()
        ref.step({"p": gr})
    assert close(mine["p"].detach().numpy(), theirs.detach().numpy())


# ------------------------------------------------------------------------------------------------ the places that are easy to get wrong
@pytest.mark.parametrize("c,yy,xx", [(0, 0, 0), (5, 3, 6), (63, 6, 6), (17, 0, 4)])
def test_flatten_order_is_channel_row_column(c, yy, xx):
    """A net whose fc1 reads one feature index picks out channel c, row y, column x of the pooled map: c * 49 + y * 7 + x."""
    sd = {k: torch.from_numpy(v).double() for k, v in weights.procedural_mnistcls_state_dict(7).items()}
    sd["fc1.weight"] = torch.zeros(128, 3136, dtype=torch.float64)
    sd["fc1.weight"][0, c * 49 + yy * 7 + xx] = 1.0
    sd["fc1.bias"] = torch.zeros(128, dtype=torch.float64)
    sd["fc2.weight"] = torch.zeros(10, 128, dtype=torch.float64)
    sd["fc2.weight"][0, 0] = 1.0
    sd["fc2.bias"] = torch.zeros(10, dtype=torch.float64)
    x = torch.from_numpy(rng.uniform((2, 1, 28, 28), 8, 9, 0.0, 2.0)).double()
    params = mnistcls_ref.params_of(sd, torch.float64)
    F = torch.nn.functional
    h = F.max_pool2d(F.relu(F.conv2d(x, sd["conv1.weight"], sd["conv1.bias"], padding=1)), 2)
    h = F.max_pool2d(F.relu(F.conv2d(h, sd["conv2.weight"], sd["conv2.bias"], padding=1)), 2)
    assert h.shape == (2, 64, 7, 7)
    got = mnistcls_ref.forward(params, x).detach()
    assert torch.equal(got[:, 0], h[:, c, yy, xx]) and float(got[:, 1:].abs().max()) == 0.0


def test_pooling_ties_send_the_gradient_to_the_first_maximum():
    """Equal positive values in a 2x2 window: the gradient goes to the first of them in row-major order; ReLU's gradient
    at exactly 0 is 0."""
    a = torch.tensor([[[[3.0, 3.0, 1.0, 5.0],
                        [3.0, 2.0, 5.0, 5.0],
                        [0.0, 0.0, 4.0, 1.0],
                        [0.0, 0.0, 1.0, 4.0]]]], dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.max_pool2d(torch.relu(a), 2)
    (g,) = torch.autograd.grad(out, a, torch.tensor([[[[1.0, 2.0], [3.0, 4.0]]]], dtype=torch.float64))
    want = torch.tensor([[[[1.0, 0.0, 0.0, 2.0],
                           [0.0, 0.0, 0.0, 0.0],
                           [0.0, 0.0, 4.0, 0.0],
                           [0.0, 0.0, 0.0, 0.0]]]], dtype=torch.float64)
    assert torch.equal(g, want)
    # the same through the restatement: a background image makes conv1's output its bias everywhere inside, all equal
    sd = {k: torch.from_numpy(v).double() for k, v in weights.procedural_mnistcls_state_dict(7).items()}
    sd["conv1.bias"] = sd["conv1.bias"].abs() + 0.1
    params = mnistcls_ref.params_of(sd, torch.float64)
    x = torch.zeros(1, 1, 28, 28, dtype=torch.float64)
    pre = torch.nn.functional.conv2d(x, params["conv1.weight"], params["conv1.bias"], padding=1)
    pre.retain_grad()
    pooled = torch.nn.functional.max_pool2d(torch.relu(pre), 2)
    pooled.sum().backward()
    grid = pre.grad[0, 0]
    assert torch.equal(grid[0::2, 0::2], torch.ones(14, 14, dtype=torch.float64)) and float(grid.sum()) == 196.0


# ------------------------------------------------------------------------------------------------ fit's bookkeeping
def test_fit_keeps_the_references_running_mean_and_saves_only_on_strict_improvement(tmp_path, monkeypatch):
    class StubTrainer(ldh.MnistClassifierTrainer):
        """step / evaluate replaced by scripted values: what is left is fit's own bookkeeping."""

        def __init__(self, losses, correct):
            super().__init__(ldh.MnistClassifier())
            self._losses, self._correct, self.steps = iter(losses), iter(correct), 0

        def step(self, x, label):
            self.steps += 1
            return torch.tensor(next(self._losses), dtype=torch.float32)

        def evaluate(self, x, label):
            return torch.tensor(next(self._correct)), 10

    losses = [4.0, 2.0, 1.0, 3.0, 0.5, 1.5]                    # two steps per epoch
    correct = [3, 4, 3, 4, 5, 4]                              # two test batches of 10 per epoch: 35 %, 35 %, 45 %
    tr = StubTrainer(losses, correct)
    saves = []
    real_save = torch.save
    monkeypatch.setattr(torch, "save", lambda obj, path, *a, **k: (saves.append(path), real_save(obj, path, *a, **k))[1])
    out_path, csv_path = str(tmp_path / "best.pth"), str(tmp_path / "loss.csv")
    batches = [(torch.zeros(1), torch.zeros(1, dtype=torch.int64))] * 2
    res = tr.fit(batches, batches, 3, out_path, csv_path)
    assert tr.steps == 6
    rows = list(csv.reader(open(csv_path)))
    assert rows[0] == ["epoch", "train_loss", "accuracy"] and len(rows) == 4
    want_loss = [np.mean(losses[:2]), np.mean(losses[:4]), np.mean(losses[:6])]      # all steps so far, not the epoch's
    for e, row in enumerate(rows[1:]):
        assert int(row[0]) == e and abs(float(row[1]) - want_loss[e]) < 1e-6
    assert [float(r[2]) for r in rows[1:]] == [35.0, 35.0, 45.0]
    assert saves == [out_path, out_path]                       # epoch 0 and epoch 2; the tie of epoch 1 is not a save
    assert res["best_acc"] == 45.0 and res["best_epoch"] == 2
    dst = ldh.MnistClassifier()
    assert checkpoint.load_mnist_classifier(out_path, dst)["n_tensors"] == 8


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_forward_predict_and_step_refuse_to_run_without_a_gpu():
    net = ldh.MnistClassifier()
    with pytest.raises(RuntimeError, match="GPU"):
        net(torch.zeros(2, 1, 28, 28))
    with pytest.raises(RuntimeError, match="GPU"):
        net.predict(torch.zeros(2, 1, 28, 28))
    tr = ldh.MnistClassifierTrainer(net)
    with pytest.raises(RuntimeError, match="GPU"):
        tr.step(torch.zeros(2, 1, 28, 28), torch.zeros(2, dtype=torch.int64))


def test_documented_argument_errors():
    net = ldh.MnistClassifier()
    with pytest.raises(ValueError, match=r"\[B, 1, 28, 28\]"):
        net(torch.zeros(2, 3, 28, 28))
    with pytest.raises(ValueError, match=r"\[B, 1, 28, 28\]"):
        net(torch.zeros(2, 1, 32, 32))
    with pytest.raises(TypeError):
        ldh.MnistClassifierTrainer(torch.nn.Linear(1, 1))
    tr = ldh.MnistClassifierTrainer(net)
    x = torch.zeros(2, 1, 28, 28)
    with pytest.raises(ValueError, match="int64"):
        tr._label(x, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[B\]"):
        tr._label(x, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="outside 0..9"):
        tr._label(x, torch.tensor([0, 10]))
    with pytest.raises(ValueError, match="outside 0..9"):
        tr._label(x, torch.tensor([-1, 3]))


def test_ld_mc_argument_validation_needs_no_gpu():
    lib = cabi.lib()
    one = 8                                                    # any non-null address: validation fails before it is used

    def refused(rc, word):
        return rc == -1 and word in lib.ld_last_error()
    assert refused(lib.ld_mc_conv1(one, one, one, one, None, 0, None), b"batch")
    assert refused(lib.ld_mc_conv1(None, one, one, one, None, 4, None), b"null")
    assert refused(lib.ld_mc_pool(one, one, None, 1, 0, 7, 64, None), b"shape")
    assert refused(lib.ld_mc_pool(None, one, None, 1, 7, 7, 64, None), b"null")
    assert refused(lib.ld_mc_pool_backward(one, one, None, one, 1, 7, 7, 64, None), b"null")
    assert refused(lib.ld_mc_gemm(one, one, one, 0, 128, 3136, 3136, 1, 3136, 1, 128, 1, None), b"shape")
    assert refused(lib.ld_mc_gemm(one, one, one, 64, 128, 3136, 3136, 1, 3136, 1, 64, 1, None), b"cm")
    assert refused(lib.ld_mc_gemm(one, one, one, 64, 128, 3136, 3136, 1, 3136, 1, 128, 99, None), b"splits")
    assert refused(lib.ld_mc_gemm(one, one, one, 64, 128, 130, 130, 1, 130, 1, 128, 4, None), b"empty slab")
    assert refused(lib.ld_mc_gemm(None, one, one, 64, 128, 3136, 3136, 1, 3136, 1, 128, 49, None), b"null")
    assert refused(lib.ld_mc_fc1_finish(one, one, one, 4, 128, 0, None), b"splits")
    assert refused(lib.ld_mc_head(one, one, one, one, one, None, None, None, None, None, 4, None), b"labels without")
    assert refused(lib.ld_mc_head(one, one, one, None, None, None, None, None, None, None, 4, None), b"null")
    assert refused(lib.ld_mc_head(one, one, one, None, one, None, None, None, None, None, 0, None), b"batch")
    assert refused(lib.ld_mc_small_grads(one, one, one, one, one, one, one, None, 4, None), b"null")
    assert refused(lib.ld_mc_conv1_wgrad(one, one, one, one, one, one, one, -1, None), b"batch")
    assert int(lib.ld_mc_conv1_wgrad_work_floats(64)) == 196 * 320 and int(lib.ld_mc_conv1_wgrad_work_floats(0)) == 0
    assert int(lib.ld_mc_conv1_wgrad_work_floats(1)) == 4 * 320


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_gemm_runs_on_the_matrix_cores_and_nothing_uses_atomics(tmp_path):
    import re
    csrc = os.path.join(ROOT, "localdiffusion-hallucination_amd", "csrc")
    out = str(tmp_path / "mnistcls.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mllvm", "-amdgpu-mfma-vgpr-form",
           "-S", "--cuda-device-only", os.path.join(csrc, "mnistcls.hip"), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=csrc)
    asm = open(out).read()
    m = re.search(r"^(_Z\w*mc_gemm_kernel\w*):[^\n]*\n(.*?)\n\s*s_endpgm", asm, flags=re.S | re.M)
    assert m, "mc_gemm_kernel not found in the assembly"
    assert m.group(2).count("v_mfma_f32_32x32x2_f32") >= 16, m.group(2).count("v_mfma")
    assert "atomic" not in re.sub(r"^\s*[;.].*$", "", asm, flags=re.M)      # no reduction of this file uses an atomic
    assert "v_fma_f32" not in m.group(2)                       # -ffp-contract=off: products and sums stay apart
