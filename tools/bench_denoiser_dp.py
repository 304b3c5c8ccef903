#!/usr/bin/env python3
"""Times the data-parallel training step of the denoiser: ``ldh.DenoiserTrainer.train_step`` at world 1 / 2 / 4 / 8 (whatever
the node shows) with the global batch growing with the world -- cfg3 (mvtec, 3 x 256^2) at 8 x world and mnist (28^2) at 64 x
world -- so that every rank keeps the one-GPU batch of tools/bench_denoiser_train.py.  fp32, ms, rank 0's clock.

  python tools/bench_denoiser_dp.py [--worlds 1,2,4,8] [--cases mvtec:256:8,mnist:28:64] [--iters 20] [--warmup 3]
         [--timeout 600] [--grace 30] [--share-gpu]
A case is data:H:rows per rank.  Every (case, world) is one process tree of its own (``launch.launch_ranks``: fresh rank
processes over RCCL, this process makes no GPU call) under ``--timeout``; the first one that fails ends the run, so nothing
more is started on the GPUs after it.  Worlds above the number of visible GPUs are left out (and said so).

Per row: the median ``train_step`` of ``--iters`` after ``--warmup``; ``apply()`` alone; its split -- the all-gather of the
ranks' ``flat + 4`` floats (events around the collective), and the GPU time of ``ld_dn_opt_reduce`` (both its launches) and of
``ld_dn_opt_step`` under the library's per-launch timing session, the median of five; and the reduce kernel's traffic,
(world + 1) x 4 bytes per trained parameter, over its time as GB/s of 8,000.  World 1 is the plain trainer (no gather, no
reduce: ``ld_dn_opt_sqnorm`` in its place).  The gather is not overlapped with the backward pass.

``--kernel-only`` needs one GPU: ``ld_dn_opt_reduce`` alone on W emulated copies of the case's flat gradient (random values,
``grad`` a buffer of its own), median of ``--iters`` event-timed calls -- both launches, so the one-workgroup merge of the
partials is in the time -- as GB/s of 8,000.  At W = 2 the copies of the larger nets fit the 256 MiB Infinity Cache between two
calls; W = 8 at cfg3 (0.39 GB read) does not.

``--share-gpu`` (tests only) lets the ranks share the visible GPUs over gloo with the exchange staged through host memory: it
shows that the tool runs, and its rows are marked as no measurement.
"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPTS = dict(branch_out=False, start_intermediate=False, start_timestep=2, mask_x=False, ood_AD=False, ood_confidence=False,
            classifier=False, use_gt=False)
KWARGS = {"mri": dict(mode="mri"), "mnist": dict(dim_mults=(1, 2, 4), full_attn=(False, False, True), mode="mnist"),
          "mvtec": dict(channels=3, out_dim=3, mode="mvtec")}
CASES = "mvtec:256:8,mnist:28:64"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="1,2,4,8")
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds one (case, world) process tree may take")
    ap.add_argument("--grace", type=float, default=30.0)
    ap.add_argument("--share-gpu", action="store_true")
    ap.add_argument("--kernel-only", action="store_true", help="one GPU: ld_dn_opt_reduce alone on emulated copies")
    ap.add_argument("--rank-case", default=None, help=argparse.SUPPRESS)
    return ap.parse_args()


def run_rank(a):
    """One rank of one (case, world) tree; rank 0 prints the row."""
    import torch
    import grad_bench
    import localdiffusion_hallucination_amd as ldh
    data, H, rows = a.rank_case.split(":")
    H, rows = int(H), int(rows)
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    ldh.configure_runtime()
    kw = {}
    if world > 1:
        import torch.distributed as dist
        if a.share_gpu:
            local %= max(1, torch.cuda.device_count())
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))     # RCCL
        kw = dict(group="default")
    torch.cuda.set_device(local)
    torch.manual_seed(0)                                      # every rank alike
    inf = ldh.Unet(dim=32, init_dim=32, **KWARGS[data])
    gd = ldh.GaussianDiffusion(dict(OPTS, data=data), inf, image_size=H, timesteps=1000, objective="pred_v").to(
        torch.device("cuda", local))
    tr = ldh.DenoiserTrainer(gd, ema_update_every=1, ema_update_after_step=0, **kw)
    if a.kernel_only:
        return kernel_only(a, tr, data, H)
    tr.ema_initted = True                                     # (every call lerps, as in tools/bench_denoiser_train.py)
    cfg = tr.online_model.cfg
    B = rows * world
    hr = torch.rand(B, cfg.channels, H, H, device="cuda")
    lr = torch.rand(B, cfg.cond_in_channels, H, H, device="cuda") * 2
    step_ms = grad_bench.time_ms(lambda: tr.train_step([(hr, lr)]), a.iters, a.warmup)
    apply_ms = grad_bench.time_ms(tr.apply, a.iters, a.warmup)
    gather_ms = grad_bench.time_ms(tr._exchange, a.iters, a.warmup) if world > 1 else None
    kern = {"dn_opt_reduce": [], "dn_opt_step": [], "dn_opt_sqnorm": []}
    for _ in range(5):
        split, _ = grad_bench.kernel_split(lambda set_phase: tr.apply())
        for k in kern:
            kern[k].append(split.get(k, [0.0, 0])[0])
    med = {k: sorted(v)[2] for k, v in kern.items()}
    trained = sum(c for _, c, adam in tr._segments.values() if adam)
    nbytes = 4 * (world + 1) * trained
    row = dict(data=data, H=H, rows_per_rank=rows, world=world, global_batch=B, step_ms=step_ms, apply_ms=apply_ms,
               gather_ms=gather_ms, reduce_kernels_ms=med["dn_opt_reduce"] if world > 1 else None,
               sqnorm_kernels_ms=med["dn_opt_sqnorm"] if world == 1 else None, step_kernel_ms=med["dn_opt_step"],
               trained_params=trained, gather_bytes_per_rank=4 * (tr._flat + 4) * (world - 1),
               reduce_bytes=nbytes if world > 1 else None,
               reduce_gbs=(nbytes / (med["dn_opt_reduce"] * 1e-3) / 1e9) if world > 1 and med["dn_opt_reduce"] > 0 else None,
               measurement=not (a.share_gpu and world > 1),
               note="ranks share a GPU over gloo, exchange staged through host memory: NOT a measurement"
               if a.share_gpu and world > 1 else "")
    d = tr.replica_digest()                                   # (collective: the replicas still agree after the timing loops)
    if rank == 0:
        print("ROW " + json.dumps(dict(row, digest_xor=d["weight_xor"])), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return 0


def kernel_only(a, tr, data, H):
    import torch
    import grad_bench
    from localdiffusion_hallucination_amd import _cabi as cabi
    from localdiffusion_hallucination_amd.trainable import stream
    lib, stride = cabi.lib(), tr._flat + 4
    trained = sum(c for _, c, adam in tr._segments.values() if adam)
    for world in [int(w) for w in a.worlds.split(",")]:
        gathered = torch.randn(world, stride, device=tr.device)
        sumsq = tr._work.data_ptr()

        def call():
            cabi.check(lib.ld_dn_opt_reduce(tr._table.data_ptr(), tr._n, tr._n_wg, gathered.data_ptr(), world, stride,
                                            tr._grad.data_ptr(), tr._flat, sumsq + 8, sumsq, stream(tr.device)), "dn_opt_reduce")
        ms = grad_bench.time_ms(call, a.iters, a.warmup)
        nbytes = 4 * (world + 1) * trained
        print("ROW " + json.dumps(dict(data=data, H=H, world=world, kernel_only=True, reduce_ms=ms, trained_params=trained,
                                       workgroups=tr._n_wg, reduce_bytes=nbytes, reduce_gbs=nbytes / (ms * 1e-3) / 1e9)), flush=True)
        del gathered
    return 0


def report(r):
    if r.get("kernel_only"):
        print(f"{r['data']:5s} @{r['H']:3d}^2 ld_dn_opt_reduce alone, {r['world']} emulated copies of {r['trained_params'] / 1e6:.1f} M "
              f"floats: {1e3 * r['reduce_ms']:7.1f} us, {r['reduce_bytes'] / 1e9:.3f} GB = {r['reduce_gbs']:7.1f} GB/s "
              f"({100 * r['reduce_gbs'] / 8000.0:.1f} % of 8,000)")
        return
    def ms(v):
        return "      n/a" if v is None else f"{v:9.3f}"
    gbs = "n/a" if r["reduce_gbs"] is None else f"{r['reduce_gbs']:7.1f} GB/s ({100 * r['reduce_gbs'] / 8000.0:.1f} % of 8,000)"
    print(f"{r['data']:5s} @{r['H']:3d}^2 world {r['world']} (global batch {r['global_batch']:3d}): step {ms(r['step_ms'])} ms, apply() "
          f"{ms(r['apply_ms'])} ms = gather {ms(r['gather_ms'])} + reduce {ms(r['reduce_kernels_ms'])} + step {ms(r['step_kernel_ms'])} "
          f"ms (kernels); reduce {gbs}" + (f"  [{r['note']}]" if r["note"] else ""))


def main():
    a = parse()
    if a.rank_case:
        return run_rank(a)
    from localdiffusion_hallucination_amd import launch
    n_dev = launch.visible_gpus()
    worlds = [int(w) for w in a.worlds.split(",")]
    if a.kernel_only:
        rows = []
        for case in a.cases.split(","):
            log_dir = tempfile.mkdtemp(prefix="ld_dp_bench_")
            cmd = [sys.executable, os.path.abspath(__file__), "--rank-case", case, "--kernel-only", "--worlds", a.worlds,
                   "--iters", str(a.iters), "--warmup", str(a.warmup)]
            rc = launch.launch_ranks(cmd, 1, timeout_s=a.timeout, grace_s=a.grace, log_dir=log_dir)
            got = [json.loads(ln[4:]) for ln in open(os.path.join(log_dir, "rank0.out")) if ln.startswith("ROW ")]
            for r in got:
                report(r)
            rows += got
            if rc != 0:
                print(f"case {case}: failed (status {rc}); stopping here", file=sys.stderr)
                print(json.dumps(rows))
                return 1
        print(json.dumps(rows))
        return 0
    todo = [w for w in worlds if a.share_gpu or w <= n_dev]
    if todo != worlds:
        print(f"{n_dev} GPU(s) visible: worlds {[w for w in worlds if w not in todo]} are not measured", file=sys.stderr)
    rows = []
    for case in a.cases.split(","):
        for world in todo:
            log_dir = tempfile.mkdtemp(prefix="ld_dp_bench_")
            cmd = [sys.executable, os.path.abspath(__file__), "--rank-case", case, "--iters", str(a.iters), "--warmup", str(a.warmup)] \
                + (["--share-gpu"] if a.share_gpu else [])
            rc = launch.launch_ranks(cmd, world, timeout_s=a.timeout, grace_s=a.grace, log_dir=log_dir, share_gpu=a.share_gpu)
            row = []
            try:
                row = [ln[4:] for ln in open(os.path.join(log_dir, "rank0.out")) if ln.startswith("ROW ")]
            except OSError:
                pass
            if rc != 0 or not row:
                print(f"case {case} world {world}: failed (status {rc}); stopping here", file=sys.stderr)
                print(json.dumps(rows))
                return 1
            rows.append(json.loads(row[0]))
            report(rows[-1])
            sys.stdout.flush()
    print(json.dumps(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
