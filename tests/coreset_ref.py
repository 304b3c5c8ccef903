"""Plain-torch restatement of the memory-bank coreset of the reference (anomalib's KCenterGreedy, as models.py:165-172
calls it), for the tests: the projection F = E @ R^T, the start row, the greedy loop and E[indices], with R and the start
given explicitly (the reference draws both unseeded).  ``dtype=torch.float64`` gives the exact-arithmetic yardstick.

The loop, in the reference's order: min_d = dist(F, F[start]); n times: idx = argmax(min_d) (the first index on ties),
min_d[idx] = 0, append idx, min_d = minimum(min_d, dist(F, F[idx])); dist is F.pairwise_distance(x, c, p=2), i.e.
|x - c + 1e-6|_2 with the eps added to every component.
"""
import numpy as np
import torch

PAIRWISE_EPS = 1e-6


def jl_min_dim(n_samples, eps=0.9):
    return int(np.int64(4 * np.log(n_samples) / (eps ** 2 / 2 - eps ** 3 / 3)))


def dist(F, c):
    """F.pairwise_distance(F, c[None], p=2) row by row: |(x - c) + eps|_2."""
    return torch.sqrt(((F - c[None, :]) + PAIRWISE_EPS).pow(2).sum(1))


def project(E, R, dtype=torch.float32):
    return E.to(dtype) @ R.to(dtype).T


def greedy(F, n, start, dtype=torch.float32):
    """The n picks (a list of ints) of the greedy loop over features F [N, k] from the start row."""
    F = F.to(dtype)
    min_d = dist(F, F[start])
    picks = []
    for _ in range(n):
        idx = int(torch.argmax(min_d))
        min_d[idx] = 0.0
        picks.append(idx)
        min_d = torch.minimum(min_d, dist(F, F[idx]))
    return picks


def states(F, start, picks, dtype=torch.float64):
    """min_d before each pick when the loop is made to take ``picks``: yields (i, min_d) for i = 0 .. len(picks) - 1,
    where min_d is what the argmax of step i sees."""
    F = F.to(dtype)
    min_d = dist(F, F[start])
    for i, p in enumerate(picks):
        yield i, min_d.clone()
        min_d[p] = 0.0
        min_d = torch.minimum(min_d, dist(F, F[p]))


def runner_up_gaps(F, start, picks, dtype=torch.float64):
    """Per step, (max - second largest value) / max of min_d along the given picks: how far each pick is from a tie."""
    gaps = []
    for _, m in states(F, start, picks, dtype):
        top = torch.topk(m, 2).values if m.numel() > 1 else torch.cat([m, m.new_zeros(1)])
        gaps.append(float((top[0] - top[1]) / top[0]))
    return gaps


def coreset(E, R, sampling_ratio, start, dtype=torch.float32):
    """(indices, memory bank E[indices]) as KCenterGreedy.sample_coreset would give them for this R and start."""
    n = int(E.shape[0] * sampling_ratio)
    F = project(E, R, dtype)
    idx = greedy(F, n, start, dtype)
    return idx, E[torch.tensor(idx, dtype=torch.long)]
