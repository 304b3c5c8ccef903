"""The arithmetic of csrc/knn16.hip (PatchCore.knn_precision = "fp16") restated in torch, fp64 as the yardstick: the
fp16 (hi, lo) split, the three-product screen, the error bounds eps_s / eps_r and the window W they give, the candidate
collection, the fp32 re-rank in the kernel's summation order (the exact search's own: one k-ordered fused chain), and the
fallback to an exact fp32 search.

Throughout, qn / bn are the fp32 squared norms the search is handed (``ld_pc_row_norms`` / ``ld_pc_embed`` make them) and
``t = max((qn - 2 q.m) + bn, 0)`` is evaluated in fp64 ON THOSE SAME fp32 NORMS: they enter the screen s, the re-rank r
and t alike, so their own rounding is no part of |s - t| or |r - t| and none of the window.

What the CPU cannot restate is the order in which one v_mfma_f32_32x32x16_f16 adds its 16 products; ``screen`` adds them
in torch's matmul order inside each of the P partial accumulators.  The bound assumes only that every addition errs by at
most 2^-23 of the partial sum; the GPU test of ``ld_pc_knn16_screen`` checks that on the hardware.
"""
import math

import torch

CAND = 64            # LD_PC_KNN16_CAND
P = 4                # partial hi.hi accumulators: K-step (16 elements) number mod 4
F16_MAX = 65504.0


# ---------------------------------------------------------------------------------------------- 1. split
def split(x):
    """x fp32 -> (hi, lo) fp16: hi = rne(x), lo = rne(x - float(hi)); the subtraction is exact in fp32.
    |x - hi - lo| <= 2^-22 |x| + 2^-25 for |x| <= 65504."""
    x = x.to(torch.float32)
    hi = x.to(torch.float16)
    lo = (x - hi.to(torch.float32)).to(torch.float16)
    return hi, lo


def fp16_finite(x):
    return bool((x.abs() <= F16_MAX).all())          # False for a NaN as well


# ---------------------------------------------------------------------------------------------- the bounds
def chain_hh(D):
    """L: the additions one hi.hi accumulator element sees: D / P products, then the merges and the + lo."""
    return D // P + P


def gamma(D):
    return 2.0 ** -20 + chain_hh(D) * 2.0 ** -23 + (2 * D + 2) * 2.0 ** -33


def eps_s(qn, bn_max, D):
    """|s - t| <= eps_s for every bank row with |m|^2 <= bn_max; qn fp32 [N] -> fp64 [N]."""
    q2 = qn.double()
    a, b = q2.sqrt(), math.sqrt(float(bn_max))
    return 2.0 * gamma(D) * a * b + 2.0 ** -22 * (q2 + float(bn_max)) + 2.0 ** -24 * math.sqrt(D) * (a + b)


def eps_r(qn, bn_max, D):
    """|r - t| <= eps_r: one fmaf chain of D products, 2^-24 each."""
    q2 = qn.double()
    a, b = q2.sqrt(), math.sqrt(float(bn_max))
    return 2.0 * D * 2.0 ** -24 * a * b + 2.0 ** -22 * (q2 + float(bn_max))


def window(qn, bn_max, D):
    """W = 2 (eps_s + eps_r) (1 + 2^-10).  A row with s > s_min + W has r > r(argmin s): it cannot be the answer."""
    return 2.0 * (eps_s(qn, bn_max, D) + eps_r(qn, bn_max, D)) * (1.0 + 2.0 ** -10)


def threshold(smin, qn, bn_max, D):
    """s_min + W rounded up to fp32, as k16_window_kernel does."""
    t = smin.double() + window(qn, bn_max, D)
    thr = t.float()
    low = thr.double() < t
    return torch.where(low, torch.nextafter(thr, torch.full_like(thr, float("inf"))), thr)


# ---------------------------------------------------------------------------------------------- 2. screen
def exact_d2(q, qn, bank, bn):
    """t [N, M] fp64."""
    return ((qn.double()[:, None] - 2.0 * (q.double() @ bank.double().T)) + bn.double()[None, :]).clamp_min(0.0)


def screen(q_hi, q_lo, qn, b_hi, b_lo, bn, drop_lo=False):
    """s [N, M] fp32 = max((qn - 2 dot16) + bn, 0), dot16 = ((hh0 + hh1) + (hh2 + hh3)) + lo, every sum in fp32."""
    D = q_hi.shape[1]
    qh, ql, bh, bl = (v.to(torch.float32) for v in (q_hi, q_lo, b_hi, b_lo))
    part = (torch.arange(D) // 16) % P
    hh = [qh[:, part == p] @ bh[:, part == p].T for p in range(P)]
    dot = (hh[0] + hh[1]) + (hh[2] + hh[3])
    if not drop_lo:
        # the one lo accumulator takes q_hi.m_lo and q_lo.m_hi of every K-step: a matmul over the interleaved K
        a = torch.stack([qh, ql], 2).reshape(qh.shape[0], 2 * D)
        b = torch.stack([bl, bh], 2).reshape(bh.shape[0], 2 * D)
        dot = dot + a @ b.T
    return ((qn[:, None] - 2.0 * dot) + bn[None, :]).clamp_min(0.0)


# ---------------------------------------------------------------------------------------------- 4. re-rank
def dot32(x, y):
    """The re-rank's fp32 dot product of every row of x [n, D] with every row of y [m, D] -> [n, m]: ONE chain
    acc = fma(x_k, y_k, acc) over k = 0, 1, ... from 0, the order of the exact kernel's v_mfma_f32_32x32x2_f32
    accumulator, so r is ld_pc_knn's own d2.  The fused multiply-add is emulated as fp32(fp64(x y) + acc): the product
    is exact in fp64, and the result can differ from the fused one only by a double rounding, which eps_r's 2^-24 per
    step covers."""
    xt, yt = x.double().T.contiguous(), y.double().T.contiguous()
    acc = torch.zeros((x.shape[0], y.shape[0]), dtype=torch.float32)
    for k in range(x.shape[1]):
        acc = (xt[k][:, None] * yt[k][None, :] + acc.double()).float()
    return acc


def rerank_d2(q, qn, bank, bn):
    """r [N, M] fp32 over ALL rows (what the contract is stated on)."""
    return ((qn[:, None] - 2.0 * dot32(q, bank)) + bn[None, :]).clamp_min(0.0)


def argmin_first(d2):
    """(min, first argmin) per row, as the (d2 bits << 32 | index) keys order."""
    v = d2.min(1).values
    idx = (d2 == v[:, None]).float().argmax(1)
    return v, idx


# ---------------------------------------------------------------------------------------------- 5. the whole search
def exact_knn(q, qn, bank, bn):
    """ld_pc_knn (the fallback): (d2 min, first argmin) of the same r over all rows."""
    return argmin_first(rerank_d2(q, qn, bank, bn))


def knn16(q, qn, bank, bn, cand=CAND, drop_lo=False, zero_window=False):
    """-> dict(dist [N], idx [N] int64, certified [N] bool, count [N] rows inside the window).  ``drop_lo`` /
    ``zero_window`` are the mutation (a plain 16-bit search): they must break the near-tie bank."""
    N, D = q.shape
    if not fp16_finite(bank):
        raise ValueError("knn16: the bank has an element that is not finite in fp16")
    q_hi, q_lo = split(q)
    b_hi, b_lo = split(bank)
    s = screen(q_hi, q_lo, qn, b_hi, b_lo, bn, drop_lo=drop_lo)
    s_cmp = torch.where(torch.isnan(s), torch.full_like(s, float("inf")), s)        # a NaN is never the minimum
    smin = s_cmp.min(1).values
    bn_max = float(bn.max())
    thr = smin.clone() if zero_window else threshold(smin, qn, bn_max, D)
    ok = torch.isfinite(thr) & torch.isfinite(qn) & (qn >= 0) & (q.abs() <= F16_MAX).all(1)
    inside = (s <= thr[:, None]) & ok[:, None]
    count = inside.sum(1)
    certified = ok & (count >= 1) & (count <= cand)
    d2 = torch.full((N,), float("nan"))
    idx = torch.zeros(N, dtype=torch.int64)
    for i in torch.nonzero(certified).flatten().tolist():
        rows = torch.nonzero(inside[i]).flatten()
        r = ((qn[i] - 2.0 * dot32(q[i][None, :], bank[rows])[0]) + bn[rows]).clamp_min(0.0)
        best = r.min()
        d2[i], idx[i] = best, rows[r == best][0]                                  # rows ascend: the first index
    fb = torch.nonzero(~certified).flatten()
    if len(fb):
        v, j = exact_knn(q[fb], qn[fb], bank, bn)
        d2[fb], idx[fb] = v, j
    return {"dist": d2.sqrt(), "idx": idx, "certified": certified, "count": count}
