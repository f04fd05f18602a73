#!/usr/bin/env python3
"""KTS with the dot, cosine and rbf kernels: end-to-end time of kts_seg_batch on the GPU, and of the Gram stage alone.

    python tools/bench_kts_kernels.py [--reps 30] [--out profiles/kts_kernels_bench.txt]

Workloads (tools/bench_kts.py's): the 75 lengths of tools/eval_corpus.corpus() as one kts_seg_batch call (ncp = n // 10),
and one video of n = 2000 (ncp = 200); D = 1024, planted shots.  "dot" is the path kts_seg_batch had before the other
two kernels (one exact-fp32 GEMM per video behind a zero-padded copy) and is the baseline; "cosine" and "rbf" run the
one-launch ragged Gram of csrc/vs_segment_gram.hip.  gram() alone is timed for the three kinds.  All variants run in
one process, alternating, --reps times each after a warm-up; the table gives medians and min - max of device-event
times.  The Gram's floor is its lower-triangle FLOPs (n (n + 1) D per video) over the fp32-MFMA peak plus one launch;
hold it against the kernel's own time from a kernel trace of this script (rocprofv3 --kernel-trace --stats).
"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kts_ref  # noqa: E402

seg = importlib.import_module("video-summarization_amd").segmentation

FP32_MFMA_TFLOPS = 157.3      # MI355X dense fp32 matrix peak
LAUNCH_US = 1.45              # one dependent kernel boundary


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, reps):
    """{name: [ms] * reps}: one warm-up of each, then reps rounds over the variants in turn."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(event_ms(fn))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    corpus_ns = [int(f.shape[0]) for f in importlib.import_module("tools.eval_corpus").corpus()[0]]
    work = [("corpus75", corpus_ns, [n // 10 for n in corpus_ns]), ("n2000_d1024", [2000], [200])]
    lines = ["KTS kernels: medians of %d alternating repeats, device events, ms (min - max)" % args.reps]
    for name, ns, ncps in work:
        xd = [torch.from_numpy(kts_ref.planted(n, 1024, max(2, n // 50), 1000 + i)).to(dev) for i, n in enumerate(ns)]
        floor_us = sum(n * (n + 1.0) * 1024 for n in ns) / (FP32_MFMA_TFLOPS * 1e12) * 1e6 + LAUNCH_US
        variants = {}
        for kind in ("dot", "cosine", "rbf"):
            variants["kts_seg_batch " + kind] = lambda kind=kind: seg.kts_seg_batch(xd, ncps, 1.0, kernel=kind)
        for kind in ("dot", "cosine", "rbf"):
            variants["gram " + kind] = lambda kind=kind: seg.gram(xd, kind)
        times = alternate(variants, args.reps)
        lines.append("%s: %d videos, %d frames, D 1024; Gram floor (lower triangle at %.1f TFLOP/s + one launch) %.1f us"
                     % (name, len(ns), sum(ns), FP32_MFMA_TFLOPS, floor_us))
        base = float(np.median(times["kts_seg_batch dot"]))
        for k, t in times.items():
            med = float(np.median(t))
            rel = "  %.2fx of dot" % (med / base) if k.startswith("kts_seg_batch") else ""
            lines.append("  %-22s %8.3f  (%.3f - %.3f)%s" % (k, med, min(t), max(t), rel))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
