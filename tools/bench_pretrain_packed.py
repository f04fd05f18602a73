#!/usr/bin/env python3
"""Pretraining step (reference src/pretrain.py:49-86) on packed ragged batches against the padded step on the SAME videos:
forward + backward of ``main + 0.5 center + repel`` through ``PretrainModel.forward_packed`` and ``PretrainModel.forward``,
and the loss head alone (``_PretrainHeadPacked`` against ``_PretrainHead`` on random hidden states of the same shapes).

    python tools/bench_pretrain_packed.py [--models A,P] [--dtypes fp32,bf16] [--seed 7] [--rounds 3] [--leg-timeout 300]

Batches: 64 videos of ``synth.corpus_lengths(64, seed)`` (100 to 650 frames) and the reference's B = 4 with
``synth.corpus_lengths(4, seed)``.  Models: A = M-A (H4 / d256 / L4), P = the ``pretrain.py`` default (H8 / d512 / L3).
``--dtypes``: exact fp32 and ``set_train_dtype("bf16")`` of the encoder (the head is exact fp32 in both forms and in every
mode; in bf16 the PADDED attention runs on the bf16 matrix pipe and the packed one is exact fp32).  ``bf16+attn``: bf16 with
``packed_attention=True`` - the packed attention on the bf16 pipe as well.

Each (model, dtype) runs in a child process of its own under a time limit; this process never opens the GPU.  A leg is timed
as a host clock around `iters` steps that end in a device synchronisation, after 3 warm-up steps of the same shape; padded and
packed legs alternate for ``--rounds`` rounds and the table shows the median with the spread (min..max) of the rounds."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="A,P")
ap.add_argument("--dtypes", default="fp32,bf16")
ap.add_argument("--batches", default="64,4")
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--dropout", type=float, default=0.2)
ap.add_argument("--leg-timeout", type=int, default=300)
ap.add_argument("--leg", default=None, help="(internal) one child: model,dtype")
args = ap.parse_args()
MODELS = {"A": (4, 256, 4), "P": (8, 512, 3)}


def driver():
    synth = importlib.import_module("video-summarization_amd.synth")
    print("pretraining step, packed ragged batches vs the padded step on the same videos: fwd + bwd of main + 0.5 center + repel, "
          "dropout %g, median of %d alternating rounds (min..max)" % (args.dropout, args.rounds), flush=True)
    for B in (int(v) for v in args.batches.split(",")):
        ls = synth.corpus_lengths(B, args.seed)
        print("B=%d  lengths %d..%d (seed %d)  rows %d packed / %d padded  fill sum T / (B Tmax) = %.3f  attention sum T^2 / (B Tmax^2) = %.3f"
              % (B, min(ls), max(ls), args.seed, sum(ls), B * max(ls), sum(ls) / (B * max(ls)), sum(t * t for t in ls) / (B * max(ls) ** 2)), flush=True)
    for model in args.models.split(","):
        for dtype in args.dtypes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", "%s,%s" % (model, dtype), "--seed", str(args.seed), "--batches", args.batches,
                   "--rounds", str(args.rounds), "--dropout", str(args.dropout)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
            except subprocess.TimeoutExpired:
                print("model %s %s: no result within %d s - stopping" % (model, dtype, args.leg_timeout), flush=True)
                sys.exit(1)
            if r.returncode != 0:
                print("model %s %s: exit status %d - stopping\n%s" % (model, dtype, r.returncode, r.stderr[-2000:]), flush=True)
                sys.exit(1)
            H, d, L = MODELS[model]
            print("model %s (H%d / d%d / L%d)  %s" % (model, H, d, L, dtype), flush=True)
            for row in (json.loads(line) for line in r.stdout.strip().split("\n") if line.startswith("{")):
                a, b = row["padded"], row["packed"]
                print("  B=%-3d %-5s (ran %s / %s)  padded %8.3f ms (%.3f..%.3f)  packed %8.3f ms (%.3f..%.3f)  packed / padded = %.3f"
                      % (row["B"], row["what"], row["ran"][0], row["ran"][1], a[0], a[1], a[2], b[0], b[1], b[2], b[0] / a[0]), flush=True)


def leg():
    import torch
    pkg = importlib.import_module("video-summarization_amd")
    pre = importlib.import_module("video-summarization_amd.pretrain")
    model, dtype = args.leg.split(",")
    H, d, L = MODELS[model]
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    m = pkg.PretrainModel(feature_dim=d, num_heads=H, num_layers=L, sparsity=0.5, dropout=args.dropout, num_classes=1, use_pos=True)
    m.encoder.load_state_dict(pkg.synth.make_state_dict(d, L, 1234))
    m = m.to(dev).train()
    m.encoder.set_train_dtype(dtype.split("+")[0], packed_attention=dtype.endswith("+attn"))

    def timed(fn, iters):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    def compare(padded, packed, iters):
        """alternating rounds -> [median, min, max] per form"""
        res = {"padded": [], "packed": []}
        for _ in range(args.rounds):
            res["padded"].append(timed(padded, iters))
            res["packed"].append(timed(packed, iters))
        return {k: [statistics.median(v), min(v), max(v)] for k, v in res.items()}

    for B in (int(v) for v in args.batches.split(",")):
        ls = pkg.synth.corpus_lengths(B, args.seed)
        tmax, rows = max(ls), sum(ls)
        iters = 30 if B >= 16 else 150                  # >= a few hundred ms per timed window
        g = torch.Generator().manual_seed(args.seed)
        xp = torch.randn(rows, 1024, generator=g).to(dev)
        vid = torch.randn(B, 512, generator=g).to(dev)
        x = torch.full((B, tmax, 1024), 1000.0, device=dev)
        off = 0
        for b, n in enumerate(ls):
            x[b, :n] = xp[off:off + n]
            off += n
        mask = x[:, :, 0] == 1000                       # pretrain.py:57
        ran = {}

        def padded_step():
            main, center, repel = m(x, vid, mask)
            m.zero_grad(set_to_none=True)
            (main + 0.5 * center + 1. * repel).backward()
            ran["padded"] = m.encoder.last_train_dtype

        def packed_step():
            main, center, repel = m.forward_packed(xp, vid, ls)
            m.zero_grad(set_to_none=True)
            (main + 0.5 * center + 1. * repel).backward()
            ran["packed"] = m.encoder.last_train_dtype + ("+attn" if m.encoder.last_packed_attention_dtype != "fp32" else "")

        r = compare(padded_step, packed_step, iters)
        print(json.dumps(dict(r, B=B, what="step", ran=[ran["padded"], ran["packed"]])), flush=True)
        if dtype != "fp32":
            continue                                     # the head is exact fp32 in every mode: measured once
        hp = torch.randn(rows, d, generator=g).to(dev).requires_grad_(True)
        sp = torch.randn(rows, 1, generator=g).to(dev).requires_grad_(True)
        h = torch.zeros(B, tmax, d, device=dev)
        s = torch.zeros(B, tmax, 1, device=dev)
        off = 0
        for b, n in enumerate(ls):
            h[b, :n], s[b, :n] = hp.detach()[off:off + n], sp.detach()[off:off + n]
            off += n
        h.requires_grad_(True)
        s.requires_grad_(True)
        W, bias = m.video_transform.weight, m.video_transform.bias
        leaves_padded, leaves_packed = [h, s, W, bias], [hp, sp, W, bias]

        def padded_head():
            lo = pre._PretrainHead.apply(h, s, vid, mask, W, bias, m.sharpening_t, True)
            torch.autograd.grad(lo[0] + 0.5 * lo[1] + lo[2], leaves_padded)

        def packed_head():
            lo = pre._PretrainHeadPacked.apply(hp, sp, vid, ls, tmax, W, bias, m.sharpening_t, True)
            torch.autograd.grad(lo[0] + 0.5 * lo[1] + lo[2], leaves_packed)

        r = compare(padded_head, packed_head, 4 * iters)
        print(json.dumps(dict(r, B=B, what="head", ran=["fp32", "fp32"])), flush=True)


if args.leg:
    leg()
else:
    driver()
