"""Memory-bank construction, host side (no GPU): the Johnson-Lindenstrauss size, the sparse random projection, the
plain-torch restatement of KCenterGreedy (tests/coreset_ref.py) on hand cases, the coreset size, the bank-time input
preparation against a transcription of anomaly_model_train.py:354-361, the bank file round trip, and the argument
validation of ld_pc_project / ld_pc_coreset."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import localdiffusion_hallucination_amd as ldh
from localdiffusion_hallucination_amd import _cabi as cabi
from localdiffusion_hallucination_amd import checkpoint, coreset, evalio
from localdiffusion_hallucination_amd.patchcore import EMBED_DIM, PatchCore

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coreset_ref as ref  # noqa: E402


# ------------------------------------------------------------------------------------------------ projection
def test_jl_min_dim():
    for n, k in ((1000, 170), (36300, 259), (156800, 295), (784000, 335)):
        assert coreset.jl_min_dim(n) == k == ref.jl_min_dim(n)
    try:
        from sklearn.random_projection import johnson_lindenstrauss_min_dim
    except ImportError:
        johnson_lindenstrauss_min_dim = None
    if johnson_lindenstrauss_min_dim is not None:
        for n in (2, 10, 999, 1000, 1568, 36300, 156800, 784000, 7_500_000):
            for eps in (0.9, 0.5, 0.1):
                assert coreset.jl_min_dim(n, eps) == int(johnson_lindenstrauss_min_dim(n, eps=eps)), (n, eps)


def test_sparse_random_projection_distribution_and_seed():
    N, D = 36300, 1536
    R = coreset.sparse_random_projection(N, D, seed=3)
    k = coreset.jl_min_dim(N)
    assert R.shape == (k, D) and R.dtype == torch.float32
    v = np.float32(math.sqrt(math.sqrt(D)) / math.sqrt(k))          # sqrt(1 / density) / sqrt(k), density 1 / sqrt(D)
    vals = set(np.unique(R.numpy()).tolist())
    assert vals == {float(-v), 0.0, float(v)}
    nnz = int((R != 0).sum())
    d = 1.0 / math.sqrt(D)
    mean, sd = k * D * d, math.sqrt(k * D * d * (1 - d))
    assert abs(nnz - mean) < 5 * sd, (nnz, mean, sd)                  # Binomial(D, d) non-zeros per row
    rows = (R != 0).sum(1).double()
    assert rows.min() > 0 and abs(float(rows.var()) - D * d * (1 - d)) < 0.5 * D * d
    pos = int((R > 0).sum())
    assert abs(pos - nnz / 2) < 5 * math.sqrt(nnz / 4)                 # signs with probability 1/2
    assert torch.equal(R, coreset.sparse_random_projection(N, D, seed=3))
    assert not torch.equal(R, coreset.sparse_random_projection(N, D, seed=4))
    with pytest.raises(ValueError):
        coreset.sparse_random_projection(1, D)


# ------------------------------------------------------------------------------------------------ the restatement
def test_start_is_not_in_the_coreset_and_keeps_the_self_distance():
    F0 = torch.tensor([[0.0, 0.0], [10.0, 0.0], [0.0, 5.0], [1.0, 1.0]], dtype=torch.float64)
    picks = ref.greedy(F0, 4, start=0, dtype=torch.float64)
    assert picks[:3] == [1, 2, 3] and picks[3] == 0              # the start comes back last, at its self-distance
    states = list(ref.states(F0, 0, picks))
    k = F0.shape[1]
    assert abs(float(states[3][1][0]) - math.sqrt(k) * 1e-6) < 1e-18
    assert float(ref.dist(F0, F0[2])[2]) == pytest.approx(math.sqrt(k) * 1e-6, rel=1e-12)


def test_self_distance_is_sqrt_k_times_eps():
    x = torch.randn(7, 33, dtype=torch.float64)
    assert torch.allclose(ref.dist(x, x[3])[3], torch.tensor(math.sqrt(33) * 1e-6, dtype=torch.float64), rtol=1e-9)
    assert torch.allclose(ref.dist(x, x[3]), F.pairwise_distance(x, x[3][None].expand_as(x), p=2), rtol=1e-12)


def test_duplicate_rows_break_ties_to_the_lowest_index():
    a, b = [0.0, 0.0, 0.0], [3.0, 4.0, 0.0]
    F0 = torch.tensor([a, b, a, b, a, [0.0, 0.0, 1.0]], dtype=torch.float64)
    picks = ref.greedy(F0, 6, start=4, dtype=torch.float64)
    # from row 4 (= a): the first b is row 1; then the far-most is row 5; then every a / b duplicate ties at the
    # self-distance and the lowest index goes first, the start row 4 included
    assert picks == [1, 5, 0, 2, 3, 4]
    assert ref.greedy(F0, 6, start=4, dtype=torch.float32) == picks


def test_restatement_order_matches_the_update_first_loop():
    g = torch.Generator().manual_seed(0)
    X = torch.randn(50, 8, generator=g, dtype=torch.float64)
    # anomalib's order: update(idx) -> argmax -> zero -> append, starting with update(start)
    min_d, idx, out = None, 7, []
    for _ in range(20):
        d = F.pairwise_distance(X, X[idx][None].expand_as(X), p=2)
        min_d = d if min_d is None else torch.minimum(min_d, d)
        idx = int(torch.argmax(min_d))
        min_d[idx] = 0
        out.append(idx)
    assert ref.greedy(X, 20, 7, torch.float64) == out


@pytest.mark.parametrize("N,r,n", [(1568, 0.1, 156), (10, 0.1, 1), (9, 0.1, 0), (784000, 0.1, 78400), (3, 1.0, 3),
                                   (100, 0.0, 0), (36300, 0.1, 3630)])
def test_coreset_size(N, r, n):
    assert coreset.coreset_size(N, r) == n == int(N * r)


def test_subsample_embedding_rejects_an_empty_coreset():
    m = PatchCore((84, 84))
    with pytest.raises(ValueError):
        m.subsample_embedding(torch.zeros(9, EMBED_DIM), 0.1)
    with pytest.raises(ValueError):
        m.subsample_embedding(torch.zeros(9, 12), 0.5)


def test_kcenter_greedy_refuses_cpu_tensors():
    with pytest.raises(ValueError):
        coreset.kcenter_greedy(torch.zeros(20, EMBED_DIM), sampling_ratio=0.5)
    with pytest.raises(ValueError):
        coreset.kcenter_greedy(features=torch.zeros(20, 8), sampling_ratio=0.5)
    assert ldh.coreset is coreset


# ------------------------------------------------------------------------------------------------ inputs and files
def _transcribed_bank_input(input, mode):
    """anomaly_model_train.py:354-361."""
    if input.shape[1] != 3:
        input = input.repeat(1, 3, 1, 1)
    if mode != 'mri':
        if input.max() > 1.0:
            input = input / 2.0
    input = F.interpolate(input, size=(224, 224), mode='bilinear', align_corners=False)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(-1, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(-1, 1, 1)
    return (input - mean) / std


@pytest.mark.parametrize("data,shape,hi", [("mnist", (3, 1, 28, 28), 2.0), ("mnist", (1, 1, 28, 28), 1.0),
                                           ("mvtec", (2, 3, 64, 64), 2.0), ("mri", (2, 1, 32, 32), 4.0)])
def test_patchcore_bank_preprocess(data, shape, hi):
    x = torch.from_numpy(np.random.default_rng(5).uniform(0, hi, shape).astype(np.float32))
    got = evalio.patchcore_bank_preprocess(x, data)
    assert got.shape == (shape[0], 3, 224, 224)                       # 224^2 in every mode, mnist included
    assert torch.equal(got, _transcribed_bank_input(x, data))


def test_patchcore_bank_preprocess_uses_the_batch_max():
    x = torch.full((2, 1, 28, 28), 0.5)
    x[1, 0, 0, 0] = 1.5                                              # one pixel of one image lifts the whole batch
    got = evalio.patchcore_bank_preprocess(x, "mnist")
    alone = evalio.patchcore_bank_preprocess(x[:1], "mnist")
    assert not torch.equal(got[:1], alone)
    assert torch.equal(got, _transcribed_bank_input(x, "mnist"))
    assert torch.equal(got[:1], _transcribed_bank_input(x[:1] / 2.0, "mnist"))


def test_save_patchcore_bank_round_trips_through_load_patchcore(tmp_path):
    from localdiffusion_hallucination_amd import weights
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_patchcore_state_dict(0).items()}
    m = PatchCore((84, 84))
    bank = np.random.default_rng(1).standard_normal((23, EMBED_DIM)).astype(np.float32)
    m.set_memory_bank(bank)
    path = tmp_path / "memory_bank_mnist_train.npy"
    checkpoint.save_patchcore_bank(m, str(path))
    saved = np.load(path)
    assert saved.dtype == np.float32 and saved.shape == (23, EMBED_DIM) and np.array_equal(saved, bank)
    m2 = PatchCore((84, 84))
    info = checkpoint.load_patchcore(sd, str(path), m2)
    assert info["bank_rows"] == 23 and torch.equal(m2.memory_bank, torch.from_numpy(bank))
    with pytest.raises(ValueError):
        checkpoint.save_patchcore_bank(PatchCore((84, 84)), str(tmp_path / "empty.npy"))


# ------------------------------------------------------------------------------------------------ C ABI
def test_project_argument_validation_needs_no_gpu():
    lib = cabi.lib()
    P = 4096                                                         # a 16-byte aligned dummy address, never touched
    ok = dict(e=P, N=100, D=1536, rowptr=P, cols=P, vals=P, k=30, out=P, ld=100)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ld_pc_project(a["e"], a["N"], a["D"], a["rowptr"], a["cols"], a["vals"], a["k"], a["out"], a["ld"],
                                 None)
    for bad, word in ((dict(e=None), b"null"), (dict(vals=None), b"null"), (dict(N=0), b"N 0"), (dict(D=1538), b"D 1538"),
                      (dict(D=4096), b"D 4096"), (dict(k=0), b"k 0"), (dict(ld=99), b"ld 99"), (dict(ld=102), b"ld 102"),
                      (dict(out=P + 4), b"aligned")):
        assert call(**bad) == -1, bad
        assert word in lib.ld_last_error(), (bad, lib.ld_last_error())


def test_coreset_argument_validation_needs_no_gpu():
    lib = cabi.lib()
    P = 4096
    ok = dict(ft=P, ld=100, N=100, k=30, n=10, start=0, min_d=P, keys=P, idx=P)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ld_pc_coreset(a["ft"], a["ld"], a["N"], a["k"], a["n"], a["start"], a["min_d"], a["keys"], a["idx"],
                                 None)
    for bad, word in ((dict(ft=None), b"null"), (dict(idx=None), b"null"), (dict(N=0), b"N 0"), (dict(k=0), b"k 0"),
                      (dict(k=9000), b"k 9000"), (dict(ld=96), b"ld 96"), (dict(ld=101), b"ld 101"), (dict(n=0), b"n 0"),
                      (dict(n=101), b"n 101"), (dict(start=100), b"start 100"), (dict(start=-1), b"start -1"),
                      (dict(min_d=P + 8), b"aligned")):
        assert call(**bad) == -1, bad
        assert word in lib.ld_last_error(), (bad, lib.ld_last_error())
    assert C.sizeof(C.c_int64) == 8
