#!/usr/bin/env python3
"""Times one call of the hallucination gate (classifier.PatchCoreClassifier, the reference's Classifier_PatchCore,
models.py:404-430) at B = 1, the way the sampler calls it inside the reverse loop: x0 on the device in, the decision as a
Python int out.  Three cases (mnist 28^2 -> 84^2, mvtec 256^2 x 3 -> 224^2, mri 256^2 -> 224^2), with and without the
anomaly map, against the same call composed in eager PyTorch around the SAME HIP PatchCore:

    repeat -> `.max() > 1.0` (host round trip) -> / 2   |  the MRI affine
    -> F.interpolate -> Normalize -> PatchCore (HIP) -> F.interpolate of the map -> `pred_score > threshold` (host round trip)

so the difference is what csrc/classifier.hip replaces.  Also one denoiser evaluation (`Unet` forward) of the matching
size timed the same way, and the gate's share of a gated joint step, gate / (gate + step).

  python tools/bench_classifier.py [--iters 20] [--warmup 5] [--bank-rows 16384] [--knn-precision fp32|fp16] [--cases 0,1,2]
``--bank-rows`` (``--bank``) takes the table at a reference-size bank (the reference's MVTec bank has 784k rows),
``--knn-precision fp16`` with PatchCore's search on the fp16 screen of csrc/knn16.hip.
Wall-clock ms per call between device synchronisations (a gate call ends with a host read, so the host side belongs to
it), median of --iters after --warmup.  Weights are procedural, the bank random (timing does not depend on values).
Prints one JSON line per case, then the README table.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import localdiffusion_hallucination_amd as ldh                    # noqa: E402
from localdiffusion_hallucination_amd import weights             # noqa: E402
from localdiffusion_hallucination_amd.classifier import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402
from localdiffusion_hallucination_amd.patchcore import EMBED_DIM  # noqa: E402

MRI = dict(data="mri", mean_flair=310.0, std_flair=420.0, mean_t1=505.0, std_t1=380.0)
CASES = [("mnist 28^2 -> 84^2", dict(data="mnist"), 3, 1, 28, dict(dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist")),
         ("mvtec 3 x 256^2 -> 224^2", dict(data="mvtec_pill"), "pill", 3, 256, dict(channels=3, out_dim=3, mode="mvtec")),
         ("mri 256^2 -> 224^2", MRI, "flair", 1, 256, dict(mode="mri"))]


def eager_gate(clf, x0, want_map):
    """Classifier_PatchCore.forward as the reference writes it, in eager PyTorch on the device around the HIP PatchCore."""
    hr = x0
    if hr.shape[1] != 3:
        hr = hr.repeat(1, 3, 1, 1)
    if clf.halve:
        if hr.max() > 1.0:
            hr = hr / 2.0
    else:
        mini, std, mean, div = clf.affine
        hr = ((hr - mini) * std + mean) / div
    S = clf.size
    hr = F.interpolate(hr, size=(S, S), mode="bilinear", align_corners=False)
    m = torch.tensor(IMAGENET_MEAN, device=hr.device).view(1, 3, 1, 1)
    s = torch.tensor(IMAGENET_STD, device=hr.device).view(1, 3, 1, 1)
    hr = (hr - m) / s
    pc = clf.patchcore
    amap = None
    if want_map:
        out = pc(hr)
        pred = out["pred_score"]
        amap = F.interpolate(out["anomaly_map"], size=tuple(x0.shape[-2:]), mode="bilinear", align_corners=False)
    else:
        pred = pc.score(hr)[0]
    if pred > clf.threshold:
        return 1, amap, pred
    return 0, amap, pred


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bank-rows", "--bank", dest="bank", type=int, default=16384)
    ap.add_argument("--knn-precision", choices=("fp32", "fp16"), default="fp32")
    ap.add_argument("--cases", default="0,1,2", help="indices into the three cases")
    args = ap.parse_args()
    ldh.configure_runtime()
    dev = "cuda"
    sd = {k: torch.from_numpy(v) for k, v in weights.procedural_patchcore_state_dict(0).items()}
    g = torch.Generator(device=dev).manual_seed(0)
    bank = torch.randn(args.bank, EMBED_DIM, device=dev, generator=g)
    pcs, rows = {}, []
    for name, config, obj, C, H, unet_kw in [CASES[int(c)] for c in args.cases.split(",")]:
        S = 84 if "mnist" in config["data"] else 224
        if S not in pcs:
            pc = ldh.PatchCore((S, S), knn_precision=args.knn_precision)
            pc.feature_extractor.load_state_dict(sd)
            pc.set_memory_bank(bank)
            pcs[S] = pc.to(dev).eval()
        x0 = torch.rand(1, C, H, H, device=dev, generator=g) * 2.0
        net = ldh.Unet(dim=32, init_dim=32, **unet_kw)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.procedural_state_dict(net.cfg, 0).items()})
        net = net.to(dev)
        xt, t = torch.randn(1, C, H, H, device=dev, generator=g), torch.full((1,), 5, dtype=torch.long, device=dev)
        with torch.no_grad():
            t_step = timed(lambda: net(xt, x0, t), args.iters, args.warmup)
            for want_map in (True, False):
                clf = ldh.PatchCoreClassifier(config, obj, pcs[S], threshold=1.0, return_map=want_map)
                a, b = clf(x0), eager_gate(clf, x0, want_map)
                assert a[0] == b[0] and abs(float(a[2]) - float(b[2])) <= 1e-3 * abs(float(b[2])), (a[2], b[2])
                t_hip = timed(lambda: clf(x0), args.iters, args.warmup)
                t_eager = timed(lambda: eager_gate(clf, x0, want_map), args.iters, args.warmup)
                t_pc = timed(lambda: pcs[S].score(clf._plan(1, H, H, x0.device)["x"]), args.iters, args.warmup)
                r = dict(case=name, return_map=want_map, bank_rows=args.bank, knn_precision=args.knn_precision,
                         knn_stats=pcs[S].knn_stats(), gate_hip_ms=round(t_hip, 4),
                         gate_eager_ms=round(t_eager, 4), speedup=round(t_eager / t_hip, 3), patchcore_score_ms=round(t_pc, 4),
                         unet_step_ms=round(t_step, 4), gate_share_of_gated_step=round(t_hip / (t_hip + t_step), 3))
                print(json.dumps(r), flush=True)
                rows.append(r)
        del net
    print("| case | map | gate, HIP | gate, eager around HIP PatchCore | eager / HIP | PatchCore score alone | `Unet` step | gate share of a gated joint step |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['case']} | {'yes' if r['return_map'] else 'no'} | {r['gate_hip_ms']:.3f} | {r['gate_eager_ms']:.3f} | "
              f"{r['speedup']:.2f} x | {r['patchcore_score_ms']:.3f} | {r['unet_step_ms']:.3f} | {100 * r['gate_share_of_gated_step']:.0f} % |")


if __name__ == "__main__":
    main()
