"""What tools/bench_resblock_grad.py, bench_linattn_grad.py and bench_attention_grad.py share: the event timing, the
per-launch split of one forward + backward over the library's entry points, the eager timing in both memory formats, and
the runner that gives every case a child process of its own under a time limit."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from localdiffusion_hallucination_amd import _cabi as cabi       # noqa: E402

HBM_PEAK_GBS = 8000.0


def time_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(iters):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(times))


class TimedLib:
    """The library with the launches of every entry point attributed to a label; forward and backward are told apart by
    ``phase``."""

    def __init__(self, lib):
        self._lib, self.calls, self.phase = lib, [], "forward"

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(("ld_dn_", "ld_seg_", "ld_pc_conv")) or name.endswith(("_work_bytes", "_splits")):
            return fn

        def wrapped(*args):
            label = name[3:]
            if name == "ld_pc_conv" or name.startswith(("ld_dn_conv16", "ld_dn_conv_f16")):
                label += " (forward)" if self.phase == "forward" else " (data gradient)"
            if name in ("ld_dn_pack_nhwc", "ld_dn_pack_nhwc_to16"):
                label += f" ({self.phase})"
            n0 = self._lib.ld_timing_count()
            rc = fn(*args)
            self.calls.append((label, n0, self._lib.ld_timing_count()))
            return rc
        return wrapped


def kernel_split(run):
    """run(set_phase) does one forward + backward under the library's timing session; returns {label: [ms, launches]} and,
    call by call in order, (label, [ms of each of its launches])."""
    lib = cabi.lib()
    timed = TimedLib(lib)
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
    split, calls = {}, []
    for label, a, b in timed.calls:
        e = split.setdefault(label, [0.0, 0])
        e[0] += float(sum(ms[a:b]))
        e[1] += b - a
        calls.append((label, [float(v) for v in ms[a:b]]))
    return split, calls


def eager_ms(mod, fn, x, extra, dout, iters, warmup):
    """{"nchw": ms, "nhwc": ms} of forward + backward of ``fn(params, x, *extra)``, the module restated in eager PyTorch on
    clones of its parameters, with x and dout in either memory format."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
    res = {}
    for fmt, name in ((torch.contiguous_format, "nchw"), (torch.channels_last, "nhwc")):
        ins = [x.detach().contiguous(memory_format=fmt)] + [e.detach().clone() for e in extra]
        for t in ins:
            t.requires_grad_(True)
        de = dout.contiguous(memory_format=fmt)
        leaves = list(p.values()) + ins

        def step():
            for v in leaves:
                v.grad = None
            fn(p, *ins).backward(de)

        res[name] = time_ms(step, iters, warmup)
    return res


def print_split(split, kernels_ms):
    for k, v in sorted(split.items(), key=lambda kv: -kv[1]["ms"]):
        print(f"      {k:28s} {v['ms']:9.3f} ms  {100 * v['ms'] / kernels_ms:5.1f} %  ({v['launches']} launches)")


# what "bf16" means at each training precision switch a bench tool exposes (the HIP side's; the eager side stays fp32)
SWITCH_HELP = {
    "conv_precision": "the HIP side's convolutions: fp32, or bf16 operands on the bf16 matrix cores (fp32 accumulation)",
    "act_storage": "bf16 (with --conv-precision bf16): the HIP side keeps the activations only convolutions read as bf16",
    "conv_out_storage": "bf16 (with --conv-precision bf16): the HIP side's ResnetBlocks keep the convolution outputs GroupNorm reads as bf16",
    "attn_precision": "the HIP side's LinearAttention cores: fp32, or bf16 operands on the bf16 matrix cores (fp32 accumulation)",
    "full_attn_precision": "the HIP side's full-softmax Attention cores: fp32, or bf16 operands on the bf16 matrix cores (fp32 accumulation)",
}


def add_switch_flags(ap, helps):
    """``--conv-precision {fp32,bf16}`` and its like (default fp32, ``args.conv_precision``) for every switch in ``helps``,
    {switch: help text}."""
    for switch, text in helps.items():
        ap.add_argument("--" + switch.replace("_", "-"), default="fp32", choices=["fp32", "bf16"], help=text)


def switch_values(a, switches):
    """{switch: its flag's value}: the keyword arguments of a model that takes them, and the entries of a JSON row."""
    return {s: getattr(a, s) for s in switches}


AMP_HELP = ("the HIP side's convolutions on the fp16 matrix cores (TrainableModule.amp: fp16 operands, fp32 accumulation; not "
            "together with --conv-precision bf16); a trainer also runs its loss scaler")


AMP_ATTN_HELP = ("the HIP side's attention cores on the fp16 matrix cores (amp_attn of LinearAttention / Attention / TrainableUnet: "
                 "fp16 operands, fp32 accumulation; not together with a bf16 attention switch); a trainer needs --amp fp16 with it")


def amp_tag(row):
    """What a report line says about ``--amp`` and ``--amp-attn``: nothing unless they were given."""
    return (f" / amp {row['amp']}" if row.get("amp", "no") != "no" else "") + \
        (f" / amp attn {row['amp_attn']}" if row.get("amp_attn", "fp32") != "fp32" else "")


def main(tool, cases, run_case, report, heads=False, switches=(), amp=False, amp_attn=False):
    """The tool's command line.  A case is ``a:b[:c...]`` (numbers, or names such as a layer kind); ``run_case(*case, args)``
    returns the case's JSON row and ``report(row)`` prints it.  ``switches``: the training precision switches the tool takes
    a flag for, e.g. ``("conv_precision", "act_storage")`` (``add_switch_flags``); ``amp``: the tool also takes ``--amp
    no|fp16`` (``args.amp``); ``amp_attn``: and ``--amp-attn fp32|fp16`` (``args.amp_attn``).  Every case runs in a child process
    (``tool --child``) under ``--timeout``; the first one that fails or runs out of time ends the run, so that nothing more is
    started on the GPU after it."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    if heads:
        ap.add_argument("--heads", type=int, default=4)
    add_switch_flags(ap, {s: SWITCH_HELP[s] for s in switches})
    if amp:
        ap.add_argument("--amp", default="no", choices=["no", "fp16"], help=AMP_HELP)
    if amp_attn:
        ap.add_argument("--amp-attn", default="fp32", choices=["fp32", "fp16"], help=AMP_ATTN_HELP)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default=cases)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds each case's process may take")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    todo = [tuple(int(v) if v.isdigit() else v for v in c.split(":")) for c in a.cases.split(",")]
    if a.child:
        (case,) = todo
        print("ROW " + json.dumps(run_case(*case, a)))
        return 0
    passed_on = [w for k in ("batch", "heads", "iters", "warmup", "amp", "amp_attn") + tuple(switches) if hasattr(a, k)
                 for w in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
    rows = []
    for case in todo:
        name = ":".join(str(v) for v in case)
        cmd = [sys.executable, os.path.abspath(tool), "--child", "--cases", name] + passed_on + \
            (["--no-eager"] if a.no_eager else [])
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"case {name}: no result within {a.timeout:.0f} s; stopping here", file=sys.stderr)
            break
        row = [ln[4:] for ln in res.stdout.splitlines() if ln.startswith("ROW ")]
        if res.returncode != 0 or not row:
            print(f"case {name}: the case's process ended with status {res.returncode}; stopping here", file=sys.stderr)
            break
        rows.append(json.loads(row[0]))
        report(rows[-1])
        sys.stdout.flush()
    print(json.dumps(rows))
    return 0 if len(rows) == len(todo) else 1
