#!/usr/bin/env python3
"""Times forward + backward of one trainable LinearAttention: ``ldh.LinearAttention`` on the HIP kernels against the same
module restated in eager PyTorch (autograd) on the same GPU in one process, fp32, ms per forward + backward.

  python tools/bench_linattn_grad.py [--batch 8] [--heads 4] [--iters 20] [--warmup 3] [--cases 32:256,64:128,128:64]
                                     [--timeout 300]
The default cases are the three levels of cfg3 that use linear attention (dim at H = W).  Every case runs in a child
process of its own under a time limit (``--timeout`` seconds; the HIP and the eager module share that process), and the
first case that fails or runs out of time ends the run: nothing more is started on the GPU after it.  Per case: 3 warm-up
calls, then the median of 20 calls timed with events around forward + backward.  The HIP module reads x and the upstream
gradient in channels_last (its own layout; a channel count that is not a multiple of 64 is repacked with padding either
way); eager PyTorch is timed in both memory formats.  One more HIP call under the library's per-launch timing session gives
the split of the time over the entry points, and the achieved bandwidth of the four attention passes against 8 TB/s.

How the bytes are counted -- what the pass has to move, each tensor once, the real channels only (hidden = 32 heads floats
per pixel and tensor): context = k and v read (its second look at k, for the part's maximum, is not counted); output = q
read, out written; reduce = q and dO read; apply = q, k, v and dO read, dq, dk, dv written.  The time is that of the pass's
main launch; the merges of the parts are listed with the split.  Prints one line per case, the split, and a JSON list at
the end.
"""
import argparse
import json
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localdiffusion_hallucination_amd as ldh                    # noqa: E402
from localdiffusion_hallucination_amd import _cabi as cabi       # noqa: E402
from bench_resblock_grad import HBM_PEAK_GBS, _TimedLib, time_ms  # noqa: E402

# label -> (index of the pass's main launch inside the entry point, tensors of `hidden` floats per pixel it moves)
PASSES = {"dn_la_context": (0, 2), "dn_la_out": (0, 2), "dn_la_backward_reduce": (0, 2), "dn_la_backward_apply": (0, 7)}


def eager_attention(p, x, heads):
    b, c, h, w = x.shape

    def rms(t, g):
        return F.normalize(t, dim=1) * g * c ** 0.5

    qkv = F.conv2d(rms(x, p["norm.g"]), p["to_qkv.weight"])
    q, k, v = [t.reshape(b, heads, 32, h * w) for t in qkv.chunk(3, dim=1)]
    q = q.softmax(dim=-2) * 32 ** -0.5
    k = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(b, heads * 32, h, w)
    return rms(F.conv2d(out, p["to_out.0.weight"], p["to_out.0.bias"]), p["to_out.1.g"])


class _Timed(_TimedLib):
    def __getattr__(self, name):
        if name.endswith(("_work_bytes", "_splits")):
            return getattr(self._lib, name)
        return super().__getattr__(name)


def kernel_split(run):
    """run(set_phase) does one forward + backward; returns {label: [ms, launches]} and {pass: ms of its main launch}."""
    import ctypes as C
    lib = cabi.lib()
    timed = _Timed(lib)
    real = cabi.lib
    cabi.check(lib.ld_timing_begin(4096), "timing_begin")
    try:
        cabi.lib = lambda: timed
        run(lambda phase: setattr(timed, "phase", phase))
        torch.cuda.synchronize()
    finally:
        cabi.lib = real
        n = max(1, lib.ld_timing_count())
        ms, cnt = (C.c_float * n)(), C.c_int()
        rc = lib.ld_timing_end(ms, n, C.byref(cnt))
    cabi.check(rc, "timing_end")
    split, passes = {}, {}
    for label, a, b in timed.calls:
        e = split.setdefault(label, [0.0, 0])
        e[0] += float(sum(ms[a:b]))
        e[1] += b - a
        if label in PASSES and b > a:
            passes[label] = float(ms[a + PASSES[label][0]])
    return split, passes


def run_case(dim, H, B, heads, iters, warmup, no_eager):
    ldh.configure_runtime()
    torch.manual_seed(0)
    mod = ldh.LinearAttention(dim, heads=heads).cuda()
    x = torch.randn(B, dim, H, H, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dout = (torch.randn(B, dim, H, H, device="cuda") / (B * H * H)).contiguous(memory_format=torch.channels_last)

    def hip_step(set_phase=None):
        mod.zero_grad(set_to_none=True)
        x.grad = None
        out = mod(x)
        if set_phase:
            set_phase("backward")
        out.backward(dout)

    hip = time_ms(hip_step, iters, warmup)
    split, passes = kernel_split(hip_step)
    kernels_ms = sum(v[0] for v in split.values())
    gbs = {k: PASSES[k][1] * mod.hidden * 4 * B * H * H / (ms * 1e6) for k, ms in passes.items() if ms > 0}
    eager = {}
    if not no_eager:
        p = {k: v.detach().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
        for fmt, name in ((torch.contiguous_format, "nchw"), (torch.channels_last, "nhwc")):
            xe = x.detach().contiguous(memory_format=fmt).requires_grad_(True)
            de = dout.contiguous(memory_format=fmt)

            def eager_step():
                for v in p.values():
                    v.grad = None
                xe.grad = None
                eager_attention(p, xe, heads).backward(de)

            eager[name] = time_ms(eager_step, iters, warmup)
    best = min(eager.values()) if eager else None
    return dict(dim=dim, H=H, B=B, heads=heads, hip_ms=hip, eager_nchw_ms=eager.get("nchw"), eager_nhwc_ms=eager.get("nhwc"),
                eager_over_hip=(best / hip if best else None), kernels_ms=kernels_ms, pass_ms=passes, pass_gbs=gbs,
                split={k: dict(ms=v[0], launches=v[1]) for k, v in split.items()})


def report(r):
    eg = ""
    if r["eager_nchw_ms"] is not None:
        eg = (f"eager PyTorch NCHW {r['eager_nchw_ms']:8.3f} ms, channels_last {r['eager_nhwc_ms']:8.3f} ms   "
              f"(best eager / HIP = {r['eager_over_hip']:.2f})")
    print(f"dim {r['dim']:4d} heads {r['heads']} @{r['H']:3d}^2 B={r['B']}: HIP {r['hip_ms']:8.3f} ms   {eg}")
    for k, v in sorted(r["split"].items(), key=lambda kv: -kv[1]["ms"]):
        print(f"      {k:28s} {v['ms']:9.3f} ms  {100 * v['ms'] / r['kernels_ms']:5.1f} %  ({v['launches']} launches)")
    for k, g in r["pass_gbs"].items():
        print(f"      {k:28s} main launch {r['pass_ms'][k]:.3f} ms = {g:.0f} GB/s ({100 * g / HBM_PEAK_GBS:.0f} % of "
              f"{HBM_PEAK_GBS / 1000:.0f} TB/s)")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="32:256,64:128,128:64")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds each case's process may take")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    cases = [tuple(int(v) for v in c.split(":")) for c in a.cases.split(",")]
    if a.child:
        (dim, H), = cases
        print("ROW " + json.dumps(run_case(dim, H, a.batch, a.heads, a.iters, a.warmup, a.no_eager)))
        return 0
    rows = []
    for dim, H in cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--cases", f"{dim}:{H}", "--batch", str(a.batch), "--heads",
               str(a.heads), "--iters", str(a.iters), "--warmup", str(a.warmup)] + (["--no-eager"] if a.no_eager else [])
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"dim {dim} @{H}^2: no result within {a.timeout:.0f} s; stopping here", file=sys.stderr)
            break
        row = [ln[4:] for ln in res.stdout.splitlines() if ln.startswith("ROW ")]
        if res.returncode != 0 or not row:
            print(f"dim {dim} @{H}^2: the case's process ended with status {res.returncode}; stopping here", file=sys.stderr)
            break
        rows.append(json.loads(row[0]))
        report(rows[-1])
    print(json.dumps(rows))
    return 0 if len(rows) == len(cases) else 1


if __name__ == "__main__":
    sys.exit(main())
