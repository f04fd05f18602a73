#!/usr/bin/env python3
"""Kernel temporal segmentation: end-to-end time on the GPU (device events after warm-up) against the float64 numpy
restatement of tests/kts_ref.py on 16 host threads, and each stage's floor.

    python tools/bench_kts.py [--reps 5] [--no-cpu] [--json out.json]

Workloads: one video at (n, ncp) = (700, 70), (2000, 200), (1000, 999), and the 75 lengths of tools/eval_corpus.corpus()
(ncp = n // 10) as one kts_seg_batch call.  D = 1024, planted shots.  Per-stage times come from a kernel trace of this
script (rocprofv3 --kernel-trace --stats); the floors printed here are what those stages are held against.  The script
also launches 200 back-to-back one-element kernels ("empty" launches) so the same trace shows the launch cadence that the
dynamic program's one-launch-per-step form is compared with.
"""
import argparse
import importlib
import json
import os
import sys
import time

for _k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_k, "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kts_ref  # noqa: E402

seg = importlib.import_module("video-summarization_amd").segmentation

FP32_MFMA_TFLOPS = 157.3      # MI355X dense fp32 matrix peak
HBM_TBS = 8.0                 # MI355X HBM3E peak


def floors(ns, ncps, D):
    """(gram, table, dp) floors in microseconds for a batch."""
    gram = sum(2.0 * n * n * D for n in ns) / (FP32_MFMA_TFLOPS * 1e12) * 1e6
    # K read twice (row scan), W written, read + written by the column scan, read + written by the J pass, column totals
    table = sum(4.0 * n * n * 2 + 8.0 * (n + 1) ** 2 * 5 for n in ns) / (HBM_TBS * 1e12) * 1e6
    dp = sum(sum((n - k) ** 2 / 2.0 * 8.0 for k in range(1, m + 1)) for n, m in zip(ns, ncps)) / (HBM_TBS * 1e12) * 1e6
    return gram, table, dp


def gpu_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def cpu_time(xs, ncps):
    t = time.perf_counter()
    for x, m in zip(xs, ncps):
        x64 = x.astype(np.float64)
        kts_ref.kts_segmentation(x64 @ x64.T, m, 1.0)
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.set_num_threads(16)
    dev = torch.device("cuda", 0)
    work = [("n700_ncp70", [700], [70]), ("n2000_ncp200", [2000], [200]), ("n1000_ncp999", [1000], [999])]
    corpus_ns = [int(f.shape[0]) for f in importlib.import_module("tools.eval_corpus").corpus()[0]]
    work.append(("corpus75", corpus_ns, [n // 10 for n in corpus_ns]))
    rows = []
    for name, ns, ncps in work:
        xs = [kts_ref.planted(n, 1024, max(2, n // 50), 1000 + i) for i, n in enumerate(ns)]
        xd = [torch.from_numpy(x).to(dev) for x in xs]
        ms = gpu_time(lambda: seg.kts_seg_batch(xd, ncps, 1.0), args.reps)
        cpu = None if args.no_cpu else cpu_time(xs, ncps)
        g, tb, dp = floors(ns, ncps, 1024)
        row = dict(workload=name, videos=len(ns), frames=sum(ns), ncp=sum(ncps), gpu_ms=round(ms, 3),
                   cpu16_ms=None if cpu is None else round(cpu, 1), speedup=None if cpu is None else round(cpu / ms, 1),
                   floor_gram_us=round(g, 2), floor_table_us=round(tb, 2), floor_dp_us=round(dp, 2),
                   dp_steps=max(ncps))
        rows.append(row)
        print(json.dumps(row), flush=True)
    # launch cadence of back-to-back one-element kernels, for the trace
    z = torch.zeros(1, device=dev)
    for _ in range(20):                 # warm-up: the first launches load the kernel
        z.add_(1.0)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(200):
        z.add_(1.0)
    b.record()
    b.synchronize()
    row = dict(workload="empty_launch_x200", per_launch_us=round(a.elapsed_time(b) * 1e3 / 200, 2))
    rows.append(row)
    print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
