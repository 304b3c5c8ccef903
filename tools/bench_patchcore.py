#!/usr/bin/env python3
"""Times PatchCore (models.py:42-254, eval) in two parts, the HIP kernels against eager PyTorch on the same GPU:

* backbone: image -> embedding rows (wide_resnet50_2 to layer3, pools, resample, concat), ms per image;
* kNN: embedding rows -> nearest bank row of each (the fused distance GEMM + min / argmin), ms per image, with the
  bank-stream bandwidth (bank bytes x the number of 128-row query tiles / time) and the FLOP rate (2 N M D / time)
  against the MI355X fp32 roofline (8.0 TB/s HBM, 157.3 TFLOPS f32 matrix).

  python tools/bench_patchcore.py [--sizes 84,224] [--batches 1,8] [--banks 16384,100000,700000] [--iters 5] [--warmup 2]
                                 [--knn-precision fp32|fp16] [--clustered-bank M] [--skip-backbone] [--skip-eager]
``--knn-precision fp16`` adds the fp16-screen search (csrc/knn16.hip) to every kNN row: ``ld_pc_knn`` and ``ld_pc_knn16``
timed alternately, twice each, on the same queries and bank (the yardstick is the fp32 kernel of the same run), with the
certified / fallen-back split and the bank rows inside the windows per query.  ``--clustered-bank M`` adds one bank of M
non-negative clustered rows with queries drawn the same way (what post-ReLU features look like: the window is exercised).
The eager legs are F.conv2d / F.batch_norm / F.avg_pool2d / F.interpolate, and euclidean_dist on torch.matmul with
torch's min(1) (the bank in chunks of 65536 rows, so the N x M distance matrix fits in memory).  Weights are
procedural, the bank random (timing does not depend on values).  Prints one line per case and a JSON list at the end.
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
from localdiffusion_hallucination_amd import weights             # noqa: E402
from localdiffusion_hallucination_amd.patchcore import EMBED_DIM  # noqa: E402

HBM_TBS, F32_TFLOPS = 8.0, 157.3
STAGES = (("layer1", 3, 1), ("layer2", 4, 2), ("layer3", 6, 2))


def eager_embed(sd, x):
    def bn(p, h):
        return F.batch_norm(h, sd[p + "running_mean"], sd[p + "running_var"], sd[p + "weight"], sd[p + "bias"], False, 0.0,
                            1e-5)
    h = F.max_pool2d(F.relu(bn("bn1.", F.conv2d(x, sd["conv1.weight"], stride=2, padding=3))), 3, 2, 1)
    feats = {}
    for name, blocks, stride in STAGES:
        for i in range(blocks):
            p, s = f"{name}.{i}.", (stride if i == 0 else 1)
            o = F.relu(bn(p + "bn1.", F.conv2d(h, sd[p + "conv1.weight"])))
            o = F.relu(bn(p + "bn2.", F.conv2d(o, sd[p + "conv2.weight"], stride=s, padding=1)))
            o = bn(p + "bn3.", F.conv2d(o, sd[p + "conv3.weight"]))
            idn = bn(p + "downsample.1.", F.conv2d(h, sd[p + "downsample.0.weight"], stride=s)) if i == 0 else h
            h = F.relu(o + idn)
        feats[name] = h
    l2, l3 = F.avg_pool2d(feats["layer2"], 3, 1, 1), F.avg_pool2d(feats["layer3"], 3, 1, 1)
    e = torch.cat((l2, F.interpolate(l3, size=l2.shape[-2:], mode="bilinear")), 1)
    return e.permute(0, 2, 3, 1).reshape(-1, e.shape[1])


def eager_knn(q, bank, bank_norm, chunk=65536):
    qn = q.pow(2).sum(-1, keepdim=True)
    best_d, best_i = None, None
    for m0 in range(0, bank.shape[0], chunk):
        d = (qn - 2 * torch.matmul(q, bank[m0:m0 + chunk].T) + bank_norm[m0:m0 + chunk][None]).clamp_min_(0).sqrt_()
        v, i = d.min(1)
        if best_d is None:
            best_d, best_i = v, i
        else:
            better = v < best_d
            best_d, best_i = torch.where(better, v, best_d), torch.where(better, i + m0, best_i)
    return best_d, best_i


def timed(fn, iters, warmup):
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="84,224")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--banks", default="16384,100000,700000")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--knn-precision", choices=("fp32", "fp16"), default="fp32")
    ap.add_argument("--clustered-bank", type=int, default=0)
    ap.add_argument("--skip-backbone", action="store_true")
    ap.add_argument("--skip-eager", action="store_true")
    args = ap.parse_args()
    ldh.configure_runtime()
    dev = "cuda"
    sd = {k: torch.from_numpy(v).to(dev) for k, v in weights.procedural_patchcore_state_dict(0).items()}
    g = torch.Generator(device=dev).manual_seed(0)
    results = []
    for H in (int(s) for s in args.sizes.split(",")):
        m = ldh.PatchCore((H, H))
        m.feature_extractor.load_state_dict({k: v.cpu() for k, v in sd.items()})
        m = m.to(dev).eval()
        for B in (int(b) for b in args.batches.split(",")):
            x = torch.randn(B, 3, H, H, device=dev, generator=g)
            if not args.skip_backbone:
                with torch.no_grad():
                    t_hip = timed(lambda: m.embed(x), args.iters, args.warmup)
                    t_eager = timed(lambda: eager_embed(sd, x), args.iters, args.warmup)
                r = dict(part="backbone", size=H, B=B, hip_ms_per_image=t_hip / B, eager_ms_per_image=t_eager / B,
                         speedup=t_eager / t_hip)
                print(json.dumps(r), flush=True)
                results.append(r)
            q_emb = m.embed(x)
            N = q_emb.shape[0]
            cases = [("gauss", int(v)) for v in args.banks.split(",") if v]
            if args.clustered_bank:
                cases.append(("clustered", args.clustered_bank))
            for kind, M in cases:
                q = q_emb
                if kind == "gauss":
                    bank = torch.randn(M, EMBED_DIM, device=dev, generator=g)
                else:
                    centres = torch.randn(64, EMBED_DIM, device=dev, generator=g).abs() * 2.0
                    bank = torch.randn(M, EMBED_DIM, device=dev, generator=g).mul_(0.28)
                    bank.add_(centres[torch.arange(M, device=dev) % 64]).abs_()
                    q = (centres[torch.arange(N, device=dev) % 64]
                         + 0.28 * torch.randn(N, EMBED_DIM, device=dev, generator=g)).abs()
                m.knn_precision = "fp32"
                m.set_memory_bank(bank)
                bank_norm = bank.pow(2).sum(-1)
                with torch.no_grad():
                    t_hip = timed(lambda: m.nearest(q), args.iters, args.warmup)
                    t_eager = float("nan") if args.skip_eager else timed(lambda: eager_knn(q, bank, bank_norm), args.iters,
                                                                         args.warmup)
                passes = (N + 127) // 128
                gbs = M * EMBED_DIM * 4 * passes / (t_hip * 1e-3) / 1e9
                tflops = 2.0 * N * M * EMBED_DIM / (t_hip * 1e-3) / 1e12
                r = dict(part="knn", bank=kind, size=H, B=B, N=N, M=M, hip_ms_per_image=t_hip / B, eager_ms_per_image=t_eager / B,
                         speedup=t_eager / t_hip, bank_stream_GBs=round(gbs, 1),
                         bank_stream_frac_hbm=round(gbs / (HBM_TBS * 1e3), 3), tflops=round(tflops, 2),
                         frac_f32_peak=round(tflops / F32_TFLOPS, 3))
                if args.knn_precision == "fp16":
                    runs = {"fp32": [], "fp16": []}
                    with torch.no_grad():
                        d32, i32 = m.nearest(q)
                        for _ in range(2):                         # alternating, each twice: the spread shows
                            for mode in ("fp32", "fp16"):
                                m.knn_precision = mode
                                runs[mode].append(timed(lambda: m.nearest(q), args.iters, args.warmup))
                        d16, i16 = m.nearest(q)
                    (cert, fell), (rows_in, rows_max) = m.knn_stats(), m.knn_candidates()
                    r.update(fp32_ms=[round(t, 4) for t in runs["fp32"]], fp16_ms=[round(t, 4) for t in runs["fp16"]],
                             fp16_speedup=round(min(runs["fp32"]) / min(runs["fp16"]), 3), certified=cert, fell_back=fell,
                             candidates_per_query=round(rows_in / N, 2), candidates_max=rows_max,
                             same_bits=bool(torch.equal(d16, d32) and torch.equal(i16, i32)))
                    m.knn_precision = "fp32"
                print(json.dumps(r), flush=True)
                results.append(r)
                del bank, bank_norm
                m.set_memory_bank(torch.zeros(1, EMBED_DIM))
                torch.cuda.empty_cache()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
