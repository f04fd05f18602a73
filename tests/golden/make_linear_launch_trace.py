#!/usr/bin/env python
"""Records tests/golden/linear_launch_trace.json on an MI355X: for every case of tests/linear_launch_cases.py the device
kernels the library launched, in order, and the SHA-256 of what they wrote.  tests/test_hip_linear_launch_trace.py replays
the cases against it, so a change of the Linear launchers that starts another kernel - or the same kernel on another grid
with another summation order - fails there.

Run it at the commit whose behaviour is the reference:  python tests/golden/make_linear_launch_trace.py [--out FILE]

Every case runs twice.  Nothing is written if two runs of a case disagree, or if the recorded names do not tell apart two
cases known to run different instantiations of gemm_nt_128 (names without template arguments would prove nothing).
"""
import argparse
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import linear_launch_cases as llc      # noqa: E402

# pairs of cases the launcher sends to different instantiations of gemm_nt_128 (128x128 / 256x256 tiles; 32- / 64-wide k-tiles)
MUST_DIFFER = (("vs_linear_bf16 M=128 N=256 K=512 relu=0 pe=0", "vs_linear_bf16 M=129 N=256 K=512 relu=0 pe=0"),
               ("vs_linear_bf16 M=129 N=256 K=448 relu=0 pe=0", "vs_linear_bf16 M=129 N=256 K=512 relu=0 pe=0"),
               ("vs_linear_f32 M=16128 N=1024 K=256 relu=1 pe=0/tiled", "vs_linear_f32 M=16129 N=1024 K=256 relu=1 pe=0/tiled"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(HERE, "linear_launch_trace.json"))
    args = ap.parse_args()
    vsa = importlib.import_module("video-summarization_amd")
    recorded = {}
    for name, rows, fn in llc.cases():
        first, second = llc.trace(vsa, rows, fn), llc.trace(vsa, rows, fn)
        if first != second:
            sys.exit("case %r: two runs disagree\n  %r\n  %r" % (name, first, second))
        recorded[name] = first
        print("%-72s %3d kernels  %s" % (name, len(first[0]), first[1][:16]), flush=True)
    for a, b in MUST_DIFFER:
        if recorded[a][0] == recorded[b][0]:
            sys.exit("the kernel names do not tell %r from %r: %r" % (a, b, recorded[a][0]))
    table = sorted({n for names, _ in recorded.values() for n in names})
    index = {n: i for i, n in enumerate(table)}
    doc = {"names": table,
           "cases": {name: {"kernels": [index[n] for n in names], "sha256": digest} for name, (names, digest) in recorded.items()}}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d kernel names, %d bytes" % (args.out, len(recorded), len(table), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
