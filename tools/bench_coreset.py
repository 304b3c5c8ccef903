#!/usr/bin/env python3
"""Times the memory-bank coreset (anomalib's KCenterGreedy, models.py:165-172), the HIP kernels against an eager-torch
restatement of anomalib's loop on the same GPU:

* projection: F = E @ R^T for E [N, 1536] (ld_pc_project, one read of E), ms and E-stream GB/s;
* greedy step: ms per step of the selection loop over F [N, k] (ld_pc_coreset, one launch per step, no host sync) and
  the feature-stream rate (4 N k bytes per step / time), against eager torch: F.pairwise_distance, torch.minimum,
  torch.argmax and the .item() host sync of every step.

  python tools/bench_coreset.py [--rows 36300,156800,784000] [--steps 200] [--eager-steps 50]
Each case times --steps greedy steps (not the whole coreset), so the ms per step holds for any sampling ratio.  E is
random (timing does not depend on values).  Prints one line per case and a JSON list at the end.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import localdiffusion_hallucination_amd as ldh                    # noqa: E402
from localdiffusion_hallucination_amd import _cabi as cabi, coreset  # noqa: E402
from localdiffusion_hallucination_amd.patchcore import EMBED_DIM  # noqa: E402

HBM_TBS = 8.0


def timed(fn, iters=3, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def eager_greedy(Fr, n, start):
    """anomalib's loop: update -> argmax (.item()) -> zero -> append."""
    min_d, idx, out = None, start, []
    for _ in range(n):
        d = F.pairwise_distance(Fr, Fr[idx:idx + 1], p=2)
        min_d = d if min_d is None else torch.minimum(min_d, d)
        idx = int(torch.argmax(min_d).item())
        min_d[idx] = 0
        out.append(idx)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="36300,156800,784000")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--eager-steps", type=int, default=50)
    args = ap.parse_args()
    ldh.configure_runtime()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    results = []
    for N in (int(v) for v in args.rows.split(",")):
        E = torch.randn(N, EMBED_DIM, device=dev, generator=g).abs_()
        R = coreset.sparse_random_projection(N, EMBED_DIM, seed=0)
        k = R.shape[0]
        Fp = coreset.project(E, R)
        rowptr, cols, vals = coreset._csr(R, dev)
        ld = Fp.stride(1)
        ft = torch.empty((k, ld), device=dev)
        lib, st = cabi.lib(), torch.cuda.current_stream().cuda_stream
        t_proj = timed(lambda: cabi.check(lib.ld_pc_project(E.data_ptr(), N, EMBED_DIM, rowptr.data_ptr(), cols.data_ptr(),
                                                            vals.data_ptr(), k, ft.data_ptr(), ld, st), "pc_project"))
        R_dev = R.to(dev)
        t_proj_eager = timed(lambda: E @ R_dev.T)
        step_bytes = coreset.feature_stream_bytes(N, k)
        t_hip = timed(lambda: coreset.greedy_indices(Fp, args.steps, 0)) / args.steps
        Fr = Fp.contiguous()                                    # row-major [N, k] for the eager loop
        t_eager = timed(lambda: eager_greedy(Fr, args.eager_steps, 0), iters=1, warmup=1) / args.eager_steps
        gbs = step_bytes / (t_hip * 1e-3) / 1e9
        r = dict(N=N, k=k, bytes_per_step=step_bytes, floor_us_at_hbm=round(step_bytes / (HBM_TBS * 1e12) * 1e6, 1),
                 hip_ms_per_step=round(t_hip, 4), eager_ms_per_step=round(t_eager, 4), speedup=round(t_eager / t_hip, 2),
                 feature_stream_GBs=round(gbs, 1), frac_hbm=round(gbs / (HBM_TBS * 1e3), 3),
                 project_ms=round(t_proj, 3), project_E_GBs=round(N * EMBED_DIM * 4 / (t_proj * 1e-3) / 1e9, 1),
                 eager_matmul_project_ms=round(t_proj_eager, 3))
        print(json.dumps(r), flush=True)
        results.append(r)
        del E, Fp, Fr, R_dev, ft
        torch.cuda.empty_cache()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
