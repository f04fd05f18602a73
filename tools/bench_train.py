#!/usr/bin/env python3
"""Training step timing: forward under autograd + loss + backward on the HIP training path, at the
reference's own regime (train.py: batch 4, a few hundred frames) and at the bench shape (B=64, T=1024), M-A.
Beside it, for context only, the same step composed from torch ops on the same GPU (tests/torch_ref.py, rocBLAS /
ATen kernels - what the reference's nn.Module does on a GPU, minus its per-layer .cpu() copy of the attention maps).

    python tools/bench_train.py [--dropout 0.3] [--torch] [--optim {torch,torch-fused,native}]

``--packed``: training on packed ragged batches against the padded step on the SAME videos (lengths drawn with a fixed seed
from ``synth.corpus_lengths``: 100 to 650 frames), forward + loss + backward, exact fp32, bf16, bf16 Linears alone and bf16 with the
opt-in packed bf16 attention (``bf16+attn``), at ``--batches`` (default
the reference's 4, and 64).  Every timed leg runs in a child process of its own under a time limit; beside the times it prints
the batch's fill sum T_i / (B Tmax) - the expected ratio of the Linears - and sum T_i^2 / (B Tmax^2), that of the attention,
and the bytes of the activation record in both forms.

    python tools/bench_train.py --packed [--batches 4,64] [--seed 7] [--leg-timeout 240]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("video-summarization_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--dropout", type=float, default=0.3)
ap.add_argument("--torch", action="store_true", help="also time the composed-torch step (context)")
ap.add_argument("--shapes", default="4x320,4x640,16x1024,64x1024")
ap.add_argument("--model", default="A")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--optim", choices=("torch", "torch-fused", "native"), default="torch",
                help="optimizer of the WHOLE train_step line: torch.optim.Adam (default), its fused=True form, or the native "
                     "Adam (video-summarization_amd/optim.py: one HIP launch, write-through into the packed weights)")
ap.add_argument("--only-step", action="store_true", help="time only the whole fp32 train_step, repeated (for a spread)")
ap.add_argument("--repeats", type=int, default=5, help="repetitions of --only-step")
ap.add_argument("--only-bf16", action="store_true", help="time only the set_train_dtype('bf16') step (for a kernel profile)")
ap.add_argument("--packed", action="store_true", help="packed ragged batches against the padded step on the same videos")
ap.add_argument("--batches", default="4,64", help="--packed: batch sizes")
ap.add_argument("--seed", type=int, default=7, help="--packed: seed of the length draw")
ap.add_argument("--leg-timeout", type=int, default=240, help="--packed: seconds each timed leg may take")
ap.add_argument("--packed-leg", default=None, help="(internal) one timed leg: B,dtype,form")
args = ap.parse_args()


def packed_driver():
    """one child process per timed leg (this process never opens the GPU), then the table"""
    H_, d_, L_ = (4, 256, 4) if args.model == "A" else (4, 512, 3)
    print("packed ragged batches vs the padded step on the same videos: model M-%s, dropout %g, fwd + loss + bwd, %d iterations per leg"
          % (args.model, args.dropout, args.iters), flush=True)
    for B in (int(v) for v in args.batches.split(",")):
        ls = pkg.synth.corpus_lengths(B, args.seed)
        tmax, rows = max(ls), sum(ls)
        fill, att = rows / (B * tmax), sum(t * t for t in ls) / (B * tmax * tmax)
        print("B=%d  lengths %d..%d (seed %d)  rows %d packed / %d padded  fill sum T / (B Tmax) = %.3f  attention sum T^2 / (B Tmax^2) = %.3f"
              % (B, min(ls), tmax, args.seed, rows, B * tmax, fill, att), flush=True)
        # "bf16-linear": VS_TRAIN_FLAG_BF16_LINEAR alone in BOTH forms (exact attention) - what the packed form runs under
        # set_train_dtype("bf16"), whose padded form has the bf16 attention kernels on top.  "bf16+attn": the packed form with
        # set_train_dtype("bf16", packed_attention=True) - bf16 Linears plus the packed bf16 attention - against the padded bf16 step
        for dtype in ("fp32", "bf16", "bf16-linear", "bf16+attn"):
            res = {}
            for form in ("padded", "packed"):
                cmd = [sys.executable, os.path.abspath(__file__), "--packed-leg", "%d,%s,%s" % (B, dtype, form), "--seed", str(args.seed),
                       "--model", args.model, "--dropout", str(args.dropout), "--iters", str(args.iters)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
                except subprocess.TimeoutExpired:
                    print("  %s %s: no result within %d s - stopping" % (dtype, form, args.leg_timeout), flush=True)
                    sys.exit(1)
                if r.returncode != 0:
                    print("  %s %s: exit status %d - stopping\n%s" % (dtype, form, r.returncode, r.stderr[-2000:]), flush=True)
                    sys.exit(1)
                res[form] = json.loads(r.stdout.strip().split("\n")[-1])
            a, b = res["padded"], res["packed"]
            print("  %-11s (ran %s / %s)  padded %.3f ms  packed %.3f ms  packed / padded = %.3f  | record %.1f MiB padded, %.1f MiB packed (%.3f)"
                  % (dtype, a["ran"], b["ran"], a["ms"], b["ms"], b["ms"] / a["ms"], a["record"] / 2 ** 20, b["record"] / 2 ** 20,
                     b["record"] / a["record"]), flush=True)


if args.packed and not args.packed_leg:
    packed_driver()
    sys.exit(0)

dev = torch.device("cuda:0")
H, d, L = (4, 256, 4) if args.model == "A" else (4, 512, 3)
sd = pkg.synth.make_state_dict(d, L, 1234)
m = pkg.SimNet(num_heads=H, d_model=d, num_layers=L, sparsity=0.0, dropout=args.dropout)
m.load_state_dict(sd)
m = m.to(dev).train()


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


if args.packed_leg:
    import ctypes
    B, dtype, form = args.packed_leg.split(",")
    B = int(B)
    ls = pkg.synth.corpus_lengths(B, args.seed)
    tmax = max(ls)
    g = torch.Generator().manual_seed(args.seed)
    xp = torch.randn(sum(ls), 1024, generator=g).to(dev)
    tp = torch.rand(sum(ls), generator=g).to(dev)
    x = torch.full((B, tmax, 1024), 1000.0, device=dev)
    target = torch.full((B, tmax), 1000.0, device=dev)
    off = 0
    for b, n in enumerate(ls):
        x[b, :n], target[b, :n] = xp[off:off + n], tp[off:off + n]
        off += n
    mask = x[:, :, 0] == 1000
    if dtype == "bf16+attn":
        m.set_train_dtype("bf16", packed_attention=True)
    else:
        m.set_train_dtype("bf16" if dtype == "bf16-linear" else dtype)
    if dtype == "bf16-linear":
        m._train_flags = lambda packed=False: pkg._lib.VS_TRAIN_FLAG_BF16_LINEAR

    def padded_step():
        pred, _ = m(x, mask)
        loss = pkg.mse_with_mask_loss(pred, target, mask)
        m.zero_grad(set_to_none=True)
        loss.backward()

    def packed_step():
        pred, _ = m.forward_packed_train(xp, ls)
        loss = pkg.mse_packed_loss(pred, tp, ls)
        m.zero_grad(set_to_none=True)
        loss.backward()

    ms = timed(packed_step if form == "packed" else padded_step, args.iters)
    lib, handle = pkg._lib.load(), m._packed_weights(dev).handle
    record = (lib.vs_train_saved_bytes_packed(handle, (ctypes.c_int32 * B)(*ls), B) if form == "packed"
              else lib.vs_train_saved_bytes(handle, B, tmax))
    ran = m.last_train_dtype + ("+attn" if form == "packed" and m.last_packed_attention_dtype != "fp32" else "")
    print(json.dumps({"B": B, "dtype": dtype, "form": form, "ms": ms, "record": int(record), "ran": ran}))
    sys.exit(0)

for shape in args.shapes.split(","):
    B, T = (int(v) for v in shape.split("x"))
    x = torch.randn(B, T, 1024, device=dev)
    lengths = [T - (37 * i) % (T // 3) for i in range(B)]
    for b, n in enumerate(lengths):
        x[b, n:] = 1000.0
    mask = x[:, :, 0] == 1000
    target = torch.rand(B, T, device=dev)

    def step():
        pred, _ = m(x, mask)
        loss = pkg.mse_with_mask_loss(pred, target, mask)
        m.zero_grad(set_to_none=True)
        loss.backward()

    # the reference's whole train_step (train.py:111-131): autocast forward, masked MSE, GradScaler, Adam - every step
    # re-packs the parameters the optimizer wrote (vs_weights_update) and rebuilds the dgrad transposes
    if args.optim == "native":
        optim = pkg.Adam(m.parameters(), lr=1e-5, weight_decay=1e-5).attach(m)      # no re-pack: the step writes the packed copy too
    else:
        optim = torch.optim.Adam(m.parameters(), lr=1e-5, weight_decay=1e-5, fused=True if args.optim == "torch-fused" else None)
    scaler = torch.amp.GradScaler("cuda")

    def full_step():
        with torch.autocast("cuda"):
            pred, _ = m(x, mask)
            loss = pkg.mse_with_mask_loss(pred, target, mask)
        optim.zero_grad(set_to_none=True)
        scaler.scale(loss).backward()
        scaler.step(optim)
        scaler.update()

    def fwd_only():
        pred, _ = m(x, mask)
        return pred

    if args.only_step:
        ts = [timed(full_step, args.iters) for _ in range(args.repeats)]
        print("B=%3d T=%4d  optim %-11s WHOLE train_step (fp32) ms: %s | min %.3f median %.3f max %.3f"
              % (B, T, args.optim, " ".join("%.3f" % t for t in ts), min(ts), sorted(ts)[len(ts) // 2], max(ts)), flush=True)
        continue
    if args.only_bf16:
        m.set_train_dtype("bf16")
        print("B=%3d T=%4d  bf16 fwd+loss+bwd %.3f ms" % (B, T, timed(step, args.iters)), flush=True)
        m.set_train_dtype("fp32")
        continue
    with torch.no_grad():
        ev = timed(lambda: m.eval()(x, mask), args.iters)
    m.train()
    f = timed(fwd_only, args.iters)
    s = timed(step, args.iters)
    fs = timed(full_step, args.iters)
    m.set_train_dtype("bf16")           # the autocast counterpart: bf16 Linear / dgrad / wgrad GEMMs
    s16 = timed(step, args.iters)
    fs16 = timed(full_step, args.iters)
    m.set_train_dtype("fp16")           # ... and with the reference's own 16-bit type (tiled GEMMs everywhere, no A-stationary form)
    sh16 = timed(step, args.iters)
    fsh16 = timed(full_step, args.iters)
    m.set_train_dtype("fp32")
    flops_f = B * T * (2 * 1024 * d + L * (24 * d * d + 4 * T * d))
    # backward: 2x the Linear flops (dgrad + wgrad) + 3.5x the attention flops (7 products for the forward's 2)
    flops_b = B * T * (2 * 2 * 1024 * d + L * (2 * 24 * d * d + 14 * T * d)) - B * T * 2 * 1024 * d   # no input gradient
    line = "B=%3d T=%4d  scoring fwd %.3f ms | train fwd %.3f ms | fwd+loss+bwd %.3f ms (bwd %.3f ms) | %.1f TF fwd, %.1f TF bwd, %.0f frames/s | WHOLE train_step (autocast + GradScaler + Adam [%s] + re-pack) %.3f ms = %.0f frames/s trained" % (
        B, T, ev, f, s, s - f, flops_f / f / 1e9, flops_b / (s - f) / 1e9, B * T / s * 1e3, args.optim, fs, B * T / fs * 1e3)
    line += " | bf16 GEMMs (set_train_dtype): fwd+loss+bwd %.3f ms, whole train_step %.3f ms = %.0f frames/s" % (s16, fs16, B * T / fs16 * 1e3)
    line += " | fp16 GEMMs: fwd+loss+bwd %.3f ms, whole train_step %.3f ms = %.0f frames/s" % (sh16, fsh16, B * T / fsh16 * 1e3)
    if args.torch:
        import torch_ref
        params = {k: v.to(dev).clone().requires_grad_(v.dtype.is_floating_point and "pos_embedding" not in k) for k, v in sd.items()}

        def tstep():
            pred, _ = torch_ref.forward_with_masks(params, x, mask, H)
            loss = (((pred.squeeze(2) - target) * (~mask).float()) ** 2).mean()
            for p_ in params.values():
                p_.grad = None
            loss.backward()
        line += " | composed torch (no dropout) %.3f ms" % timed(tstep, max(2, args.iters // 2))
    print(line, flush=True)
