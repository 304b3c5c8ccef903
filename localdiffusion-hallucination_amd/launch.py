"""``launch_ranks``: start the rank processes of a one-node multi-GPU run without an outside launcher.

The parent makes no GPU call (it counts the GPUs from the KFD topology and the ``*_VISIBLE_DEVICES`` variables, not through
HIP) and never replaces its own program: every rank is a fresh child process with ``RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_ADDR / MASTER_PORT`` set and its stdout / stderr in files of its own.  A rank that exits non-zero most likely leaves
its peers stuck in a collective, so they get ``grace_s`` to finish and are then killed by PID; ``timeout_s`` bounds the whole
run.  This is what ``bench.py --gpus N`` does for the benchmark, restated for the tools.
"""
import os
import socket
import subprocess
import sys
import tempfile
import time

from .tuning import process_env

MAX_RANKS = 16          # processes with a GPU open at the same time


def visible_gpus():
    """The number of GPUs a child would see, without a GPU call: the KFD topology's nodes that have SIMDs, cut down by the
    first ``*_VISIBLE_DEVICES`` variable that is set (a comma-separated list; empty means none)."""
    n = 0
    top = "/sys/class/kfd/kfd/topology/nodes"
    try:
        for node in os.listdir(top):
            try:
                for line in open(os.path.join(top, node, "properties")):
                    if line.startswith("simd_count") and int(line.split()[1]) > 0:
                        n += 1
            except (OSError, ValueError, IndexError):
                pass
    except OSError:
        return 0
    env = process_env()
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = env.get(var)
        if v is not None:
            n = min(n, len([x for x in v.split(",") if x.strip()]))
    return n


def _tail(path, lines=30):
    try:
        return "".join(open(path, errors="replace").readlines()[-lines:])
    except OSError:
        return ""


def launch_ranks(argv, gpus, *, timeout_s, grace_s, log_dir=None, share_gpu=False, out=None):
    """Run ``argv`` (a full command, e.g. ``[sys.executable, "tool.py", ...]``) as ``gpus`` rank processes and wait.

    Returns 0 when every rank exited 0, else non-zero after printing the exit codes and the tail of the FIRST failing
    rank's stderr to ``out`` (default ``sys.stderr``).  Rank r's output is ``<log_dir>/rank<r>.out`` and ``.err`` (``log_dir``
    None: a fresh temporary directory).  ``share_gpu`` (tests: several ranks on one GPU) lifts the check against the number
    of visible GPUs and wraps ``LOCAL_RANK`` around it; more than ``MAX_RANKS`` ranks, or more than there are GPUs, is
    refused with ``ValueError`` before anything starts."""
    out = sys.stderr if out is None else out
    if not isinstance(gpus, int) or isinstance(gpus, bool) or gpus < 1 or gpus > MAX_RANKS:
        raise ValueError(f"launch_ranks: gpus = {gpus!r} (1..{MAX_RANKS})")
    if not (timeout_s > 0 and grace_s >= 0):
        raise ValueError(f"launch_ranks: timeout_s {timeout_s!r} must be positive and grace_s {grace_s!r} non-negative")
    n_dev = visible_gpus()
    if gpus > n_dev and not share_gpu:
        raise ValueError(f"launch_ranks: {gpus} ranks but {n_dev} GPU(s) visible (KFD topology / *_VISIBLE_DEVICES)")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    log_dir = log_dir or tempfile.mkdtemp(prefix="ld_ranks_")
    os.makedirs(log_dir, exist_ok=True)
    procs, errs, files = [], [], []
    try:
        for r in range(gpus):
            child = process_env()
            child.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            child.update(RANK=str(r), LOCAL_RANK=str(r % max(1, n_dev) if share_gpu else r), WORLD_SIZE=str(gpus),
                         MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            errs.append(os.path.join(log_dir, f"rank{r}.err"))
            fo, fe = open(os.path.join(log_dir, f"rank{r}.out"), "wb"), open(errs[-1], "wb")
            files += [fo, fe]
            procs.append(subprocess.Popen(list(argv), env=child, stdin=subprocess.DEVNULL, stdout=fo, stderr=fe))
        t0 = time.monotonic()
        first_bad, deadline, why = None, t0 + timeout_s, None
        while any(p.poll() is None for p in procs):
            now = time.monotonic()
            if first_bad is None:
                bad = [r for r, p in enumerate(procs) if p.poll() not in (None, 0)]
                if bad:
                    first_bad = bad[0]
                    deadline = min(deadline, now + grace_s)      # the others are most likely stuck in a collective now
            if now > deadline:
                why = (f"rank {first_bad} failed and the others did not finish within {grace_s:g} s" if first_bad is not None
                       else f"timeout: {timeout_s:g} s")
                break
            time.sleep(0.02)
    finally:
        for p in procs:                                          # exact PIDs of the children this function started
            if p.poll() is None:
                p.kill()
        codes = [p.wait() for p in procs]
        for f in files:
            f.close()
    if any(codes) or why:
        bad = first_bad if first_bad is not None else next((r for r, c in enumerate(codes) if c), 0)
        print(f"launch_ranks: rank exit codes {codes}" + (f" ({why})" if why else "") + f"; per-rank output in {log_dir}", file=out)
        print(f"---- tail of {errs[bad]} ----\n{_tail(errs[bad])}", file=out)
        return 1
    return 0
