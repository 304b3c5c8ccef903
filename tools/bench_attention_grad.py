#!/usr/bin/env python3
"""Times forward + backward of one trainable full Attention: ``ldh.Attention`` on the HIP kernels against the same module
restated in eager PyTorch (autograd) on the same GPU in one process, fp32, ms per forward + backward.

  python tools/bench_attention_grad.py [--batch 8] [--heads 4] [--iters 20] [--warmup 3] [--cases 128:32,256:32]
                                       [--timeout 300]
The default cases are cfg3's two uses of full attention (dim at H = W): the last stage of the down and up paths and
``mid_attn``.  Every case runs in a child process of its own under a time limit (``--timeout`` seconds; the HIP and the eager
module share that process), and the first case that fails or runs out of time ends the run: nothing more is started on the
GPU after it.  Per case: 3 warm-up calls, then the median of 20 calls timed with events around forward + backward.  The HIP
module reads x and the upstream gradient in channels_last (its own layout); eager PyTorch is timed in two forms -- the
reference's einsum / softmax lines and ``F.scaled_dot_product_attention`` -- each in both memory formats, and the best of
the four is quoted.  One more HIP call under the library's per-launch timing session gives the split of the time over the
entry points, and the achieved FLOP/s of the three attention passes against the 157 TFLOP/s fp32 matrix peak.

How the FLOPs are counted -- tile products of 2 n^2 32 FLOP per (sample, head), exponentials and rescales not counted: the
forward has two (q k^T, p v), the backward's row pass three (q k^T, dO v^T, ds k), its column pass four (k q^T, v dO^T, p^T
dO, ds^T q).  Prints one line per case, the split, and a JSON list at the end.
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

FP32_MATRIX_PEAK_TFLOPS = 157.0
# pass -> (entry point's label, index of its launch inside the entry point, tile products)
PASSES = {"forward": ("dn_fa_forward", 0, 2), "backward rows (dq)": ("dn_fa_backward", 0, 3),
          "backward columns (dk, dv)": ("dn_fa_backward", 1, 4)}


def eager_attention(p, x, heads, sdpa):
    b, c, h, w = x.shape
    qkv = F.conv2d(F.normalize(x, dim=1) * p["norm.g"] * c ** 0.5, p["to_qkv.weight"])
    q, k, v = [t.reshape(b, heads, 32, h * w).transpose(-1, -2) for t in qkv.chunk(3, dim=1)]
    if sdpa:
        out = F.scaled_dot_product_attention(q, k, v)
    else:
        sim = torch.einsum("bhid,bhjd->bhij", q, k) * 32 ** -0.5
        out = torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), v)
    out = out.transpose(-1, -2).reshape(b, heads * 32, h, w)
    return F.conv2d(out, p["to_out.weight"], p["to_out.bias"])


class _Timed(_TimedLib):
    def __getattr__(self, name):
        if name.endswith(("_work_bytes", "_splits")):
            return getattr(self._lib, name)
        return super().__getattr__(name)


def kernel_split(run):
    """run(set_phase) does one forward + backward; returns {label: [ms, launches]} and {pass: ms of its launch}."""
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
        for name, (lab, idx, _) in PASSES.items():
            if lab == label and b > a + idx:
                passes[name] = float(ms[a + idx])
    return split, passes


def run_case(dim, H, B, heads, iters, warmup, no_eager):
    ldh.configure_runtime()
    torch.manual_seed(0)
    mod = ldh.Attention(dim, heads=heads).cuda()
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
    n = H * H
    tflops = {k: PASSES[k][2] * 2 * n * n * 32 * B * heads / (ms * 1e9) for k, ms in passes.items() if ms > 0}
    eager = {}
    if not no_eager:
        p = {k: v.detach().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
        for sdpa in (False, True):
            for fmt, name in ((torch.contiguous_format, "nchw"), (torch.channels_last, "nhwc")):
                xe = x.detach().contiguous(memory_format=fmt).requires_grad_(True)
                de = dout.contiguous(memory_format=fmt)

                def eager_step():
                    for v in p.values():
                        v.grad = None
                    xe.grad = None
                    eager_attention(p, xe, heads, sdpa).backward(de)

                eager[("sdpa_" if sdpa else "einsum_") + name] = time_ms(eager_step, iters, warmup)
    best = min(eager.values()) if eager else None
    return dict(dim=dim, H=H, B=B, heads=heads, hip_ms=hip, eager_ms=eager, eager_over_hip=(best / hip if best else None),
                kernels_ms=kernels_ms, pass_ms=passes, pass_tflops=tflops,
                split={k: dict(ms=v[0], launches=v[1]) for k, v in split.items()})


def report(r):
    eg = ""
    if r["eager_ms"]:
        eg = "eager PyTorch " + ", ".join(f"{k} {v:.3f} ms" for k, v in r["eager_ms"].items()) + \
            f"   (best eager / HIP = {r['eager_over_hip']:.2f})"
    print(f"dim {r['dim']:4d} heads {r['heads']} @{r['H']:3d}^2 B={r['B']}: HIP {r['hip_ms']:8.3f} ms   {eg}")
    for k, v in sorted(r["split"].items(), key=lambda kv: -kv[1]["ms"]):
        print(f"      {k:28s} {v['ms']:9.3f} ms  {100 * v['ms'] / r['kernels_ms']:5.1f} %  ({v['launches']} launches)")
    for k, t in r["pass_tflops"].items():
        print(f"      {k:28s} {r['pass_ms'][k]:.3f} ms = {t:.1f} TFLOP/s ({100 * t / FP32_MATRIX_PEAK_TFLOPS:.0f} % of "
              f"{FP32_MATRIX_PEAK_TFLOPS:.0f})")
    mb = 3 * 32 * r["heads"] * 4 * r["B"] * r["H"] ** 2 / 1e6
    print(f"      qkv is {mb:.1f} MB = {mb / HBM_PEAK_GBS:.4f} ms at {HBM_PEAK_GBS / 1000:.0f} TB/s, what a pass would take were it memory-bound")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="128:32,256:32")
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
