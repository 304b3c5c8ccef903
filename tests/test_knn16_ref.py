"""The fp16-screen / fp32-re-rank nearest-neighbour search, on the CPU: the arithmetic of tests/knn16_ref.py against
fp64.  The split's residual, the bounds eps_s and eps_r on three kinds of bank, the contract (the answer is the argmin of
the re-rank distance over ALL rows, first index on ties), the mutation that must break it, and the overflow fallback."""
import functools

import numpy as np
import torch

from localdiffusion_hallucination_amd import rng

import knn16_ref as k16

D = 1536


def gauss(shape, key, scale=1.0):
    return torch.from_numpy(rng.randn(shape, 1616, key)) * scale


def norms(x):
    return (x * x).sum(1)


@functools.lru_cache(maxsize=None)
def bank_case(kind):
    """(q [64, D], bank [5000, D]) of the three bound banks; computed once, never modified."""
    N, M = 64, 5000
    if kind == "gauss":
        q, bank = gauss((N, D), 1), gauss((M, D), 2)
    elif kind == "clustered":
        # non-negative clustered rows, what post-ReLU features look like: |q|^2 ~ 6300, nearest d^2 ~ 235
        centres = gauss((20, D), 3).abs() * 2.0
        q = (centres[torch.arange(N) % 20] + 0.28 * gauss((N, D), 4)).abs()
        bank = (centres[torch.arange(M) % 20] + 0.28 * gauss((M, D), 5)).abs()
    else:
        # tiny and large magnitudes in one row: lo parts in fp16's subnormal range beside elements near 1e3
        mag_q = torch.from_numpy(10.0 ** rng.uniform((N, D), 1616, 6, -6.0, 3.0).astype(np.float64)).float()
        mag_b = torch.from_numpy(10.0 ** rng.uniform((M, D), 1616, 7, -6.0, 3.0).astype(np.float64)).float()
        q, bank = gauss((N, D), 8) * mag_q, gauss((M, D), 9) * mag_b
    return q.contiguous(), bank.contiguous()


def test_split_is_exact_to_the_stated_residual():
    mags = torch.from_numpy(10.0 ** rng.uniform((200_000,), 1616, 20, -6.0, np.log10(6.0e4)).astype(np.float64)).float()
    sign = torch.where(gauss((200_000,), 21) < 0, -1.0, 1.0)
    x = torch.cat([mags * sign, torch.zeros(8), torch.tensor([65504.0, -65504.0, 6.0e4, 1.0e-6, 2.0 ** -3, 2.0 ** -24])])
    hi, lo = k16.split(x)
    assert hi.dtype == torch.float16 and lo.dtype == torch.float16
    assert torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all()
    res = (x.double() - hi.double() - lo.double()).abs()
    bound = 2.0 ** -22 * x.double().abs() + 2.0 ** -25
    print(f"split: largest residual / bound {float((res / bound).max()):.3f}")
    assert (res <= bound).all()
    assert (lo.double().abs() <= 2.0 ** -11 * x.double().abs() + 2.0 ** -25).all()
    z = k16.split(torch.zeros(4))
    assert (z[0] == 0).all() and (z[1] == 0).all()
    assert not k16.fp16_finite(torch.tensor([1.0, 7.0e4])) and not k16.fp16_finite(torch.tensor([float("nan")]))


def test_screen_and_rerank_stay_inside_their_bounds():
    for kind in ("gauss", "clustered", "mixed"):
        q, bank = bank_case(kind)
        qn, bn = norms(q), norms(bank)
        t = k16.exact_d2(q, qn, bank, bn)
        s = k16.screen(*k16.split(q), qn, *k16.split(bank), bn)
        r = k16.rerank_d2(q, qn, bank, bn)
        es, er = k16.eps_s(qn, bn.max(), D), k16.eps_r(qn, bn.max(), D)
        ratio_s = float(((s.double() - t).abs() / es[:, None]).max())
        ratio_r = float(((r.double() - t).abs() / er[:, None]).max())
        inside = (s.double() <= (s.double().min(1).values + k16.window(qn, bn.max(), D))[:, None]).sum(1)
        print(f"{kind}: |s - t| / eps_s <= {ratio_s:.4f}, |r - t| / eps_r <= {ratio_r:.4f}, "
              f"rows inside the window mean {float(inside.float().mean()):.2f} max {int(inside.max())}")
        assert ratio_s <= 1.0 and ratio_r <= 1.0
        assert inside.min() >= 1


@functools.lru_cache(maxsize=None)
def near_tie_case():
    """16 queries, each with 40 rows at distances 5 (1 + delta), 0 <= delta <= 1e-4, two of them exact duplicates of the
    nearest one (at a lower and at a higher index than it would otherwise win at), in a bank of 3000 Gaussian rows."""
    N, M, R = 16, 3000, 40
    q, bank = gauss((N, D), 30), gauss((M, D), 31)
    delta = torch.from_numpy(rng.uniform((N, R), 1616, 32, 0.0, 1.0e-4)).float()
    delta[:, 7] = 0.0                                             # the nearest of the 40
    pos = torch.from_numpy(np.random.RandomState(33).permutation(M)[:N * R].reshape(N, R))     # disjoint positions
    for i in range(N):
        e = gauss((R, D), 40 + i)
        e = 5.0 * (1.0 + delta[i])[:, None] * e / e.norm(dim=1, keepdim=True)
        rows = q[i] + e
        rows[21] = rows[7]                                        # an exact duplicate of the nearest row
        bank[pos[i]] = rows
    return q.contiguous(), bank.contiguous(), pos


def test_contract_argmin_of_the_rerank_distance_over_all_rows():
    q, bank, pos = near_tie_case()
    qn, bn = norms(q), norms(bank)
    out = k16.knn16(q, qn, bank, bn)
    r_all = k16.rerank_d2(q, qn, bank, bn)
    want_d2, want_idx = k16.argmin_first(r_all)
    assert out["certified"].all() and int(out["count"].min()) >= 40       # every query is checked, none is excused
    assert torch.equal(out["idx"], want_idx)
    assert torch.equal(out["dist"], want_d2.sqrt())
    first_dup = torch.minimum(pos[:, 7], pos[:, 21])
    t = k16.exact_d2(q, qn, bank, bn)
    tied = (r_all[torch.arange(16), pos[:, 7]] == want_d2)                # where the duplicate pair is the minimum of r
    later_dup = torch.maximum(pos[:, 7], pos[:, 21])
    in_pair = tied & ((out["idx"] == first_dup) | (out["idx"] == later_dup))
    print(f"near ties: the duplicate pair holds the minimum of r for {int(tied.sum())} of 16 queries, wins {int(in_pair.sum())}")
    assert in_pair.any()                                                  # (fp32's rounding decides among the 40)
    assert (out["idx"] != later_dup).all()                                # the second of two equal rows never wins
    assert (out["idx"][tied] <= first_dup[tied]).all() and torch.equal(out["idx"][in_pair], first_dup[in_pair])
    # and the answer is within the two bounds of the true minimum
    assert ((t[torch.arange(16), out["idx"]] - t.min(1).values) <= 2.0 * k16.eps_r(qn, bn.max(), D)).all()


def test_mutation_a_plain_fp16_search_breaks_the_near_tie_bank():
    q, bank, _ = near_tie_case()
    qn, bn = norms(q), norms(bank)
    want = k16.argmin_first(k16.rerank_d2(q, qn, bank, bn))[1]
    plain = k16.knn16(q, qn, bank, bn, drop_lo=True, zero_window=True)
    wrong = int((plain["idx"] != want).sum())
    print(f"mutation (lo terms dropped, W = 0): {wrong} of {len(want)} indices wrong")
    assert wrong >= 1


def test_overflow_is_reported_and_still_answered_exactly():
    N, M = 8, 2000
    q, bank = gauss((N, D), 50), gauss((M, D), 51)
    near = q + 0.05 * gauss((N, D), 52)
    bank[torch.arange(N) * 3] = near
    bank[100:100 + k16.CAND + 6] = near[2]                        # more rows inside query 2's window than a segment holds
    big = q.clone()
    big[5, 17] = 7.0e4                                            # not finite in fp16
    qn, bn = norms(big), norms(bank)
    out = k16.knn16(big, qn, bank, bn)
    assert out["certified"].tolist() == [True, True, False, True, True, False, True, True]
    assert int(out["count"][2]) > k16.CAND
    want = k16.exact_knn(big, qn, bank, bn)
    assert torch.equal(out["idx"], want[1]) and int(out["idx"][2]) == 6       # the first of the duplicates
    fb = ~out["certified"]
    assert torch.equal(out["dist"][fb], want[0].sqrt()[fb])               # the fallback's own distances
    r_min = k16.argmin_first(k16.rerank_d2(big, qn, bank, bn))[0]
    assert torch.equal(out["dist"][~fb], r_min.sqrt()[~fb])               # the certified ones: the re-rank's
    assert int(out["certified"].sum()) + int((~out["certified"]).sum()) == N


def test_switch_is_validated_and_no_part_of_the_state_dict():
    import pytest
    import localdiffusion_hallucination_amd as ldh
    m = ldh.PatchCore((84, 84))
    assert m.knn_precision == "fp32" and m.knn_stats() is None
    with pytest.raises(ValueError):
        m.knn_precision = "bf16"
    with pytest.raises(ValueError):
        ldh.PatchCore((84, 84), knn_precision="half")
    m.knn_precision = "fp16"
    m.set_memory_bank(gauss((3, D), 60))                          # on the CPU: nothing to pack yet
    assert m.knn_precision == "fp16" and set(m.state_dict()) == set(ldh.PatchCore((84, 84)).state_dict())
    clf = ldh.PatchCoreClassifier(dict(data="mnist"), 3, m, threshold=1.0, knn_precision="fp32")
    assert m.knn_precision == "fp32" and clf.knn_precision == "fp32"
    with pytest.raises(ValueError):
        clf.knn_precision = "fp8"
