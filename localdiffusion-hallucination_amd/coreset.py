"""Memory-bank construction for ``PatchCore``: anomalib's ``KCenterGreedy`` coreset (models.py:165-172, what
anomaly_model_train.py:339-385 runs on the stacked training embeddings) on the kernels of ``csrc/coreset.hip``.

* ``sparse_random_projection``: the Johnson-Lindenstrauss matrix R [k, D] of anomalib's ``SparseRandomProjection(eps=0.9)``
  (k = ``johnson_lindenstrauss_min_dim(N, eps)``, density 1 / sqrt(D), values +-sqrt(1 / density) / sqrt(k) built in
  fp64), drawn from a seeded numpy ``Generator`` instead of the global RNGs;
* ``project``: F = E @ R^T on the GPU (``ld_pc_project``), stored feature-major for the greedy loop;
* ``kcenter_greedy``: the greedy selection (``ld_pc_coreset``): min_d = dist(F, F[start]), then n = int(N * ratio) times
  idx = first argmax(min_d), min_d[idx] = 0, min_d = minimum(min_d, dist(F, F[idx])), with dist the
  ``F.pairwise_distance`` |x - c + 1e-6|_2.  The start row itself is not in the coreset and keeps sqrt(k) * 1e-6.

A reference run draws R and the start index unseeded, so its picks cannot be reproduced; these functions give the same
picks as the reference for a given R and start.  No CPU fallback: the projection and the loop are HIP kernels only.
"""
import numpy as np
import torch

from . import _cabi as cabi

JL_EPS = 0.9


def jl_min_dim(n_samples, eps=JL_EPS):
    """sklearn's / anomalib's ``johnson_lindenstrauss_min_dim``: int64(4 ln N / (eps^2 / 2 - eps^3 / 3))."""
    den = (eps ** 2) / 2.0 - (eps ** 3) / 3.0
    return int(np.int64(4.0 * np.log(np.float64(n_samples)) / den))


def coreset_size(n_rows, sampling_ratio):
    """KCenterGreedy's ``coreset_size``: int(N * sampling_ratio)."""
    return int(n_rows * sampling_ratio)


def sparse_random_projection(n_samples, n_features=1536, eps=JL_EPS, seed=0):
    """R [k, n_features] fp32 (a dense tensor on the CPU), k = ``jl_min_dim(n_samples, eps)``: each row has
    Binomial(n_features, d) non-zeros, d = 1 / sqrt(n_features), at distinct random columns, each +-sqrt(1 / d) / sqrt(k)
    with equal probability (computed in fp64, then rounded to fp32 as the reference's ``.T.float()`` does)."""
    if n_samples < 2 or n_features < 1:
        raise ValueError(f"sparse_random_projection: n_samples {n_samples}, n_features {n_features}")
    k = jl_min_dim(n_samples, eps)
    if k < 1:
        raise ValueError(f"sparse_random_projection: eps {eps} gives k = {k}")
    g = np.random.default_rng(seed)
    density = 1.0 / np.sqrt(n_features)
    comp = np.zeros((k, n_features), np.float64)
    for i in range(k):
        nnz = int(g.binomial(n_features, density))
        cols = g.choice(n_features, size=nnz, replace=False)
        comp[i, cols] = g.integers(0, 2, size=nnz) * 2.0 - 1.0
    comp *= np.sqrt(1.0 / density) / np.sqrt(k)
    return torch.from_numpy(comp.astype(np.float32))


def _csr(R, dev):
    """Dense R [k, D] -> (rowptr [k + 1], cols, vals) int32 / int32 / fp32 on dev (columns ascending in each row)."""
    r = R.detach().to("cpu", torch.float32).numpy()
    rows, cols = np.nonzero(r)
    rowptr = np.zeros(r.shape[0] + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=r.shape[0]), out=rowptr[1:])
    vals = r[rows, cols]
    if cols.size == 0:                                   # an all-zero R: keep the pointers valid
        cols, vals = np.zeros(1, np.int64), np.zeros(1, np.float32)
    return (torch.from_numpy(rowptr).to(dev), torch.from_numpy(cols.astype(np.int32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(vals, np.float32)).to(dev))


def _ld(n):
    return (n + 3) // 4 * 4


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _check_gpu(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{what} must be a CUDA tensor (HIP kernels only; there is no CPU fallback)")


def project(E, R):
    """F = E @ R^T for the embedding E [N, D] (fp32, on the GPU) and a projection R [k, D] (sparse or dense, any
    device).  Returns F as an [N, k] view of feature-major storage [k, ld] (ld = N rounded up to 4), the layout that
    ``kcenter_greedy(features=F)`` streams without a copy."""
    _check_gpu(E, "project: E")
    if E.dim() != 2 or R.dim() != 2 or R.shape[1] != E.shape[1]:
        raise ValueError(f"project: E {tuple(E.shape)} and R {tuple(R.shape)} (expected [N, D] and [k, D])")
    N, D = E.shape
    k = R.shape[0]
    dev = E.device
    E = E.detach().to(torch.float32).contiguous()
    rowptr, cols, vals = _csr(R, dev)
    ld = _ld(N)
    ft = torch.zeros((k, ld), dtype=torch.float32, device=dev) if ld != N else \
        torch.empty((k, ld), dtype=torch.float32, device=dev)
    cabi.check(cabi.lib().ld_pc_project(E.data_ptr(), N, D, rowptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), k,
                                        ft.data_ptr(), ld, _stream(dev)), "pc_project")
    return ft[:, :N].t()


def _feature_major(F):
    """(ft [k, ld] storage, ld) for features F [N, k]: F itself when it is already such a view (what ``project``
    returns), else a padded feature-major copy."""
    N, k = F.shape
    ld = F.stride(1)
    if F.dtype == torch.float32 and F.stride(0) == 1 and ld >= N and ld % 4 == 0 and F.data_ptr() % 16 == 0 \
            and F.untyped_storage().nbytes() >= 4 * (F.storage_offset() + k * ld):
        return F.t().as_strided((k, ld), (ld, 1)), ld     # [k, ld] over F's own storage, row stride ld
    ld = _ld(N)
    ft = torch.zeros((k, ld), dtype=torch.float32, device=F.device)
    ft[:, :N] = F.detach().t()
    return ft, ld


def greedy_indices(features, n, start):
    """The n greedy picks (int64 [n] on the device) from features F [N, k] and the start row; n >= 1."""
    _check_gpu(features, "kcenter_greedy: features")
    N, k = features.shape
    if not 1 <= n <= N:
        raise ValueError(f"kcenter_greedy: coreset size {n} (1..{N})")
    if not 0 <= start < N:
        raise ValueError(f"kcenter_greedy: start {start} (0..{N - 1})")
    dev = features.device
    ft, ld = _feature_major(features)
    min_d = torch.empty(ld, dtype=torch.float32, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    cabi.check(cabi.lib().ld_pc_coreset(ft.data_ptr(), ld, N, k, n, start, min_d.data_ptr(), keys.data_ptr(),
                                        idx.data_ptr(), _stream(dev)), "pc_coreset")
    return idx


def start_index(n_rows, seed=0):
    """The start row that ``kcenter_greedy(start=None, seed=seed)`` uses (the reference's unseeded torch.randint)."""
    return int(np.random.default_rng([seed, 1]).integers(n_rows))


def kcenter_greedy(E=None, *, features=None, sampling_ratio, projection=None, start=None, seed=0):
    """anomalib's ``KCenterGreedy(E, sampling_ratio).sample_coreset()`` as row indices: int64 [int(N * ratio)] on the
    GPU, in pick order (``E[indices]`` is the memory bank).

    Either pass the embedding E [N, D] (fp32 on the GPU), projected with ``projection`` (R [k, D]) or, when that is
    None, with ``sparse_random_projection(N, D, seed=seed)``; or pass ``features`` F [N, k] that were projected
    elsewhere.  ``start`` is the first centre (not itself picked); None draws it with ``start_index(N, seed)``."""
    if features is None:
        if E is None:
            raise ValueError("kcenter_greedy: pass the embedding E or features")
        _check_gpu(E, "kcenter_greedy: E")
        if E.dim() != 2 or E.shape[0] < 1:
            raise ValueError(f"kcenter_greedy: E {tuple(E.shape)}, expected [N >= 1, D]")
        N = E.shape[0]
    else:
        if projection is not None:
            raise ValueError("kcenter_greedy: pass projection or features, not both")
        _check_gpu(features, "kcenter_greedy: features")
        if features.dim() != 2 or features.shape[0] < 1:
            raise ValueError(f"kcenter_greedy: features {tuple(features.shape)}, expected [N >= 1, k]")
        N = features.shape[0]
    n = coreset_size(N, sampling_ratio)
    dev = (E if features is None else features).device
    if n <= 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    if features is None:
        R = projection if projection is not None else sparse_random_projection(N, E.shape[1], seed=seed)
        features = project(E, torch.as_tensor(R))
    if start is None:
        start = start_index(N, seed)
    return greedy_indices(features, n, int(start))


def feature_stream_bytes(n_rows, k):
    """Bytes one greedy step reads from the features (the floor of its memory traffic, min_d aside)."""
    return 4 * n_rows * k


__all__ = ["jl_min_dim", "coreset_size", "sparse_random_projection", "project", "kcenter_greedy", "start_index",
           "greedy_indices", "feature_stream_bytes", "JL_EPS"]
