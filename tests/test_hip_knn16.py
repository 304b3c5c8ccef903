"""PatchCore's nearest-neighbour search at knn_precision = "fp16" on the GPU (csrc/knn16.hip): the bank's fp16 split, the
screened distances against fp64 within the bound that the window rests on (the hardware check of the accumulation
model), ``nearest`` on the cases of test_hip_patchcore.py's kNN tests, the fallback, the whole model and the gate in
both modes, and the switch itself."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import localdiffusion_hallucination_amd as ldh                              # noqa: E402
from localdiffusion_hallucination_amd import _cabi as cabi                  # noqa: E402
from localdiffusion_hallucination_amd import rng, weights                   # noqa: E402
from localdiffusion_hallucination_amd.patchcore import EMBED_DIM            # noqa: E402

import knn16_ref as k16                                                     # noqa: E402
from hip_helpers import DEV, st                                             # noqa: E402


def _gauss(shape, key, scale=1.0):
    return torch.from_numpy(rng.randn(shape, 3535, key)) * scale


def rel_err(a, b):
    return float((a.detach().cpu().double() - b.cpu().double()).abs().max() / b.cpu().double().abs().max())


def _pc_bank(bank, precision):
    m = ldh.PatchCore((84, 84), knn_precision=precision).to(DEV).eval()
    m.set_memory_bank(bank)
    return m


def row_norms(x):
    n = torch.empty(x.shape[0], dtype=torch.float32, device=DEV)
    cabi.check(cabi.lib().ld_pc_row_norms(x.data_ptr(), n.data_ptr(), x.shape[0], x.shape[1], st()), "pc_row_norms")
    return n


def pack_bank(bank):
    """bank [M, D] on the device -> (hi, lo, info, bn)."""
    bn = row_norms(bank)
    hi = torch.full(bank.shape, float("nan"), dtype=torch.float16, device=DEV)
    lo = torch.full(bank.shape, float("nan"), dtype=torch.float16, device=DEV)
    info = torch.full((2,), float("nan"), device=DEV)
    cabi.check(cabi.lib().ld_pc_pack_bank16(bank.data_ptr(), bn.data_ptr(), bank.shape[0], bank.shape[1], hi.data_ptr(),
                                            lo.data_ptr(), info.data_ptr(), st()), "pc_pack_bank16")
    return hi, lo, info, bn


# ------------------------------------------------------------------------------------------------ the bank's split
def test_pack_bank16_matches_the_cpu_split():
    M = 301
    mag = torch.from_numpy(10.0 ** rng.uniform((M, EMBED_DIM), 3535, 400, -6.0, 4.5).astype(np.float64)).float()
    bank = (_gauss((M, EMBED_DIM), 401) * mag).clamp(-6.0e4, 6.0e4)
    bank[0, :8] = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, 2.0 ** -25, 1.0e-6, 0.125])
    hi, lo, info, bn = pack_bank(bank.to(DEV))
    want_hi, want_lo = k16.split(bank)
    assert torch.equal(hi.cpu(), want_hi) and torch.equal(lo.cpu(), want_lo)
    assert float(info[0]) == float(bn.max()) and float(info[1]) == 1.0
    bad = _gauss((70, EMBED_DIM), 402)
    bad[69, 1535] = 7.0e4
    assert float(pack_bank(bad.to(DEV))[2][1]) == 0.0
    m = ldh.PatchCore((84, 84), knn_precision="fp16").to(DEV).eval()
    with pytest.raises(ValueError, match="fp16"):
        m.set_memory_bank(bad)
    m32 = _pc_bank(bad, "fp32")                                   # fp32 takes the bank ...
    m32.nearest(bad[:3].to(DEV))
    with pytest.raises(ValueError, match="fp16"):                 # ... and refuses to become "fp16" with it
        m32.knn_precision = "fp16"
    assert m32.knn_precision == "fp32"


# ------------------------------------------------------------------------------------------------ the screen's bound
def clustered(n, d, key):
    """Non-negative clustered rows (what post-ReLU features look like)."""
    centres = _gauss((7, d), 500).abs() * 2.0
    return (centres[torch.arange(n) % 7] + 0.28 * _gauss((n, d), key)).abs().contiguous()


@pytest.mark.parametrize("N,M,D", [(5, 3, 1536), (130, 1000, 1536), (300, 449, 1536), (130, 1000, 32), (130, 1000, 96)])
def test_screen_stays_inside_eps_s(N, M, D):
    """|s - t| <= eps_s for every pair: the hardware check of "each MFMA addition errs by at most 2^-23 of the partial
    sum".  D = 32 is one (half) K-chunk, D = 96 fewer K-steps than partial accumulators in the last chunk."""
    lib = cabi.lib()
    for kind in ("gauss", "clustered"):
        q = (_gauss((N, D), 510) if kind == "gauss" else clustered(N, D, 511)).to(DEV)
        bank = (_gauss((M, D), 512) if kind == "gauss" else clustered(M, D, 513)).to(DEV)
        hi, lo, info, bn = pack_bank(bank)
        qn = row_norms(q)
        work = torch.empty(int(lib.ld_pc_knn16_work_bytes(N, D)), dtype=torch.uint8, device=DEV)
        s = torch.full((N, M), float("nan"), device=DEV)
        cabi.check(lib.ld_pc_knn16_screen(q.data_ptr(), qn.data_ptr(), N, hi.data_ptr(), lo.data_ptr(), bn.data_ptr(), M, D,
                                          work.data_ptr(), s.data_ptr(), st()), "pc_knn16_screen")
        t = k16.exact_d2(q, qn, bank, bn)                         # fp64, on the device
        eps = k16.eps_s(qn, float(info[0]), D)
        ratio = float(((s.double() - t).abs() / eps[:, None]).max())
        s_ref = k16.screen(*k16.split(q.cpu()), qn.cpu(), hi.cpu(), lo.cpu(), bn.cpu())
        print(f"screen N={N} M={M} D={D} {kind}: max |s - t| / eps_s = {ratio:.4f}, "
              f"max |s - s_cpu| / eps_s = {float(((s.cpu().double() - s_ref.double()).abs() / eps.cpu()[:, None]).max()):.4f}")
        assert torch.isfinite(s).all() and ratio <= 1.0


# ------------------------------------------------------------------------------------------------ nearest
def both_modes(q, bank):
    """nearest(q) at "fp16" and at "fp32" on one bank -> ((d16, i16, stats), (d32, i32))."""
    m = _pc_bank(bank, "fp16")
    d16, i16 = m.nearest(q.to(DEV))
    stats = m.knn_stats()
    assert sum(stats) == q.shape[0]
    m.knn_precision = "fp32"
    d32, i32 = m.nearest(q.to(DEV))
    d16, i16, d32, i32 = d16.cpu(), i16.cpu().long(), d32.cpu(), i32.cpu().long()
    # the re-rank sums in the exact kernel's order, so the two modes agree to the bit, ties included
    print(f"fp16 vs fp32 mode: {int((i16 == i32).sum())} of {len(i16)} indices, {int((d16 == d32).sum())} distances equal")
    assert torch.equal(i16, i32) and torch.equal(d16, d32)
    return (d16, i16, stats), (d32, i32)


@pytest.mark.parametrize("N,M", [(5, 3), (130, 1000), (300, 64 * 7 + 1), (9, 1), (1, 777)])
def test_knn16_small_and_ragged(N, M):
    q, bank = _gauss((N, EMBED_DIM), 70), _gauss((M, EMBED_DIM), 71)
    # half the queries have a clear nearest row.  Not the lone query of N = 1: the distance tolerance is relative to the
    # largest distance, and fp32's d2 = (qn - 2 q.m) + bn at d = 2, |x|^2 = 1536 carries 2.6e-4 of d in EITHER mode (same
    # bits); the other cases measure it against the unplanted queries' d = 55, and so does this one
    plant = torch.arange(0, N, 2) if N > 1 else torch.arange(0)
    bank[plant % M] = q[plant] + 0.05 * _gauss((len(plant), EMBED_DIM), 72)
    d64 = torch.cdist(q.double(), bank.double())
    top2 = d64.topk(2, largest=False).values if M > 1 else None
    clear = (top2[:, 1] - top2[:, 0] > 1e-2) if M > 1 else torch.ones(N, dtype=torch.bool)
    assert clear.float().mean() >= 0.5
    (d16, i16, stats), (d32, i32) = both_modes(q, bank)
    assert torch.equal(i16[clear], d64.argmin(1)[clear]) and torch.equal(i16[clear], i32[clear])
    assert rel_err(d16, d64.min(1).values) < 1e-4
    assert stats == (N, 0)                                        # Gaussian rows: one or two rows inside every window


def test_knn16_large_bank():
    N, M = 121, 200_003
    q, bank = _gauss((N, EMBED_DIM), 80), _gauss((M, EMBED_DIM), 81)
    pos = torch.arange(N) * 1651 + 7                  # spread over the bank: many tiles, many splits
    bank[pos] = q + 0.5 * _gauss((N, EMBED_DIM), 83)
    (d16, i16, stats), (d32, i32) = both_modes(q, bank)
    d_ref = torch.cdist(q.to(DEV).double(), bank.to(DEV).double()).min(1)
    assert torch.equal(d_ref.indices.cpu(), pos)
    assert torch.equal(i16, pos) and torch.equal(i32, pos)
    assert rel_err(d16, d_ref.values.float().cpu()) < 1e-4
    assert stats == (N, 0)


def test_knn16_duplicate_rows_take_the_first_index():
    N, M = 40, 5000
    q, bank = _gauss((N, EMBED_DIM), 90), _gauss((M, EMBED_DIM), 91)
    near = q + 0.05 * _gauss((N, EMBED_DIM), 92)
    first = torch.arange(N) * 97 + 11                 # duplicates of the nearest row, spread over tiles and splits
    bank[first] = near
    bank[first + 1] = near
    bank[M - 1 - torch.arange(N)] = near
    (d16, i16, stats), (d32, i32) = both_modes(q, bank)
    assert torch.equal(i16, first) and torch.equal(i32, first)
    assert rel_err(d16, (q - near).norm(dim=1)) < 1e-3
    assert stats == (N, 0)


def test_knn16_near_tie_accepts_any_index_within_tolerance():
    N, M = 16, 3000
    q, bank = _gauss((N, EMBED_DIM), 100), _gauss((M, EMBED_DIM), 101)
    e = _gauss((N, EMBED_DIM), 102)
    e = 5.0 * e / e.norm(dim=1, keepdim=True)
    bank[:N] = q + e
    bank[N:2 * N] = q - e * (1.0 + 1e-7)              # a second row at (nearly) the same distance
    (d16, i16, stats), (d32, i32) = both_modes(q, bank)
    d64 = torch.cdist(q.double(), bank.double())
    best = d64.min(1).values
    picked = d64[torch.arange(N), i16]
    assert ((picked - best).abs() <= 1e-3 * best.max()).all()
    assert rel_err(d16, best.float()) < 1e-3
    # the contract, on the device's own norms: the answer is the first argmin of the CPU restatement's r over all rows
    # (the emulated multiply-add could differ from the fused one by a double rounding; on this data it does not)
    qn, bn = row_norms(q.to(DEV)).cpu(), row_norms(bank.to(DEV)).cpu()
    r = k16.rerank_d2(q, qn, bank, bn)
    r2 = r.topk(2, largest=False).values
    want = k16.argmin_first(r)[1]
    print(f"near tie: {int((i16 == want).sum())} of {N} indices are the first argmin of the restated r; "
          f"smallest gap to the runner-up {float((r2[:, 1] - r2[:, 0]).min()):.3e}")
    assert stats == (N, 0) and torch.equal(i16, want)


# ------------------------------------------------------------------------------------------------ fallback
def test_knn16_uncertified_queries_fall_back_to_the_exact_search():
    N, M = 12, 3000
    q, bank = _gauss((N, EMBED_DIM), 110), _gauss((M, EMBED_DIM), 111)
    near = q + 0.05 * _gauss((N, EMBED_DIM), 112)
    home = torch.arange(N) * 5 + 2000
    bank[home] = near
    bank[300:500] = near[3]                           # 200 exact duplicates: more than a candidate segment holds
    q[7, 1000] = 7.0e4                                # not finite in fp16 ...
    bank[2500, 1000] = 6.0                            # ... and this row is clearly the nearest to it
    (d16, i16, stats), (d32, i32) = both_modes(q, bank)
    assert stats == (N - 2, 2)
    want = home.clone()
    want[3] = 300                                     # the first of the duplicates
    d64 = torch.cdist(q.double(), bank.double())
    want[7] = 2500
    top2 = d64[7].topk(2, largest=False)
    assert int(top2.indices[0]) == 2500 and float(top2.values[1] - top2.values[0]) > 1.0
    assert torch.equal(i16, want)
    assert torch.equal(i16[[3, 7]], i32[[3, 7]]) and torch.equal(d16[[3, 7]], d32[[3, 7]])    # exactly ld_pc_knn's
    keep = torch.arange(N) != 7
    assert rel_err(d16[keep], d64.min(1).values[keep]) < 1e-3 and rel_err(d16[7:8], d64.min(1).values[7:8]) < 1e-3


# ------------------------------------------------------------------------------------------------ the whole model
_SD = {}


def _state_dict():
    if "sd" not in _SD:
        _SD["sd"] = {k: torch.from_numpy(np.asarray(v)) for k, v in weights.procedural_patchcore_state_dict(0).items()}
    return _SD["sd"]


def planted_bank(emb, B, seed=0):
    """test_hip_patchcore.py's recipe: a clear nearest row for every embedding row (e_i + noise of norm 2.0 .. 2.9, the
    image's patch p* at 3.0), a cluster of 8 rows around p*'s row and 997 far rows, shuffled."""
    N, D = emb.shape
    P = N // B
    g = torch.Generator().manual_seed(seed)
    dist = 2.0 + 0.9 * torch.rand(N, generator=g)
    pstar = torch.randint(0, P, (B,), generator=g)
    dist[torch.arange(B) * P + pstar] = 3.0
    n = torch.randn(N, D, generator=g)
    rows = [emb + n / n.norm(dim=1, keepdim=True) * dist[:, None]]
    for b in range(B):
        c = torch.randn(8, D, generator=g)
        r = 1.5 + 0.15 * torch.arange(1, 9, dtype=torch.float32)
        rows.append(rows[0][b * P + pstar[b]] + c / c.norm(dim=1, keepdim=True) * r[:, None])
    rows.append(emb.mean(0) + 3.0 * torch.randn(997, D, generator=g))
    bank = torch.cat(rows)
    return bank[torch.randperm(bank.shape[0], generator=g)].contiguous(), pstar


@pytest.mark.parametrize("H,B", [(84, 1), (224, 2)])
def test_patchcore_forward_fp16_equals_fp32(H, B):
    x = torch.from_numpy(rng.uniform((B, 3, H, H), 3535, 200 + H + B, -2.0, 2.0)).to(DEV)
    m = ldh.PatchCore((H, H))
    m.feature_extractor.load_state_dict(_state_dict())
    m = m.to(DEV).eval()
    emb = m.embed(x)
    m.set_memory_bank(planted_bank(emb.cpu(), B)[0])
    want = m(x)
    loc32 = m.nearest(emb)[1].clone()
    m.knn_precision = "fp16"
    got = m(x)
    loc16 = m.nearest(emb)[1]
    stats = m.knn_stats()
    print(f"PatchCore {H}^2 B={B} fp16 kNN: certified {stats[0]}, fell back {stats[1]}")
    assert sum(stats) == emb.shape[0] and torch.equal(loc16, loc32)
    assert rel_err(got["pred_score"], want["pred_score"]) < 1e-4
    assert rel_err(got["anomaly_map"], want["anomaly_map"]) < 1e-4


def test_gate_fp16_decides_as_fp32():
    config = dict(data="mnist")
    x0 = torch.from_numpy(rng.uniform((1, 1, 28, 28), 3535, 950, 0.0, 1.0)).to(DEV)
    m = ldh.PatchCore((84, 84))
    m.feature_extractor.load_state_dict(_state_dict())
    m = m.to(DEV).eval()
    clf = ldh.PatchCoreClassifier(config, 3, m, threshold=1.0)
    assert clf.knn_precision == "fp32"
    m.set_memory_bank(planted_bank(m.embed(clf.preprocess(x0)).cpu(), 1)[0])
    _, map32, s32 = clf(x0)
    map32, s32 = map32.clone(), s32.clone()
    clf16 = ldh.PatchCoreClassifier(config, 3, m, threshold=1.0, knn_precision="fp16")
    assert m.knn_precision == "fp16" and clf16.knn_precision == "fp16"
    for factor, want_dec in ((0.9, 1), (1.1, 0)):
        clf16.threshold = factor * float(s32)
        dec, map16, s16 = clf16(x0)
        assert dec == want_dec
        assert rel_err(s16, s32) < 1e-4 and rel_err(map16, map32) < 1e-4
    assert sum(m.knn_stats()) == 11 * 11


# ------------------------------------------------------------------------------------------------ the switch
def test_switch_default_validation_and_state_dict():
    m = ldh.PatchCore((84, 84))
    assert m.knn_precision == "fp32" and m.knn_stats() is None
    for bad in ("bf16", "FP16", None, 16):
        with pytest.raises(ValueError):
            m.knn_precision = bad
        with pytest.raises(ValueError):
            ldh.PatchCore((84, 84), knn_precision=bad)
    assert m.knn_precision == "fp32"
    m.knn_precision = "fp16"
    assert not any("knn" in k or "precision" in k for k in m.state_dict())
    assert set(m.state_dict()) == set(ldh.PatchCore((84, 84)).state_dict())
