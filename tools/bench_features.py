#!/usr/bin/env python3
"""GoogLeNet pool5 frame features on the device: features.GoogLeNetFeatures.extract against the float32 restatement of the same
network (tests/googlenet_ref.py) run by torch's own ops on the same GPU, in one process.

    python tools/bench_features.py [--reps 30] [--out profiles/features_bench.txt] [--no-torch] [--once]

Timed, after warm-up of every shape, as medians over --reps with min and max, the two paths ALTERNATING inside every repeat (other
work shares the host); a timing is a host clock around calls that end in a device synchronise:
  N = 64 frames and N = 1 frame at 224 x 224, uint8 frames in, [N, 1024] out
  frames/s and achieved TFLOP/s (2 * MACs of the 57 convs, from the shapes) against the 157.3 TFLOP/s fp32-MFMA roof
  the ten costliest layers of the N = 64 forward, each conv timed alone through vs_cnn_conv
  frames -> summary at T = 320: extract, then summary.summarize (score, KTS, keyshot summary); the front end's share
The two paths' outputs are compared at the sizes timed before anything is timed.  If torch's convolution cannot run here, the
file says so and reports ours alone.  --once: one extract of each size and nothing else (for a kernel trace)."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import googlenet_ref as ref  # noqa: E402

pkg = importlib.import_module("video-summarization_amd")
features, summary, L = pkg.features, pkg.summary, pkg._lib
ROOF_TFLOPS = 157.3


def clock(fn, dev, calls=1):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3 / calls


def alternate(fns, reps, dev, calls=1):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ts[k].append(clock(fn, dev, calls))
    return [dict(median_ms=round(float(np.median(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4)) for t in ts]


def conv_layers(h, w):
    """[(name, cin, cout, k, stride, pad, h_in, w_in, h_out, w_out)] of the 57 convs for an h x w frame"""
    size = {name: (hh, ww) for name, _, hh, ww in ref.layer_sizes(h, w)}
    out = []
    for prefix, cout, cin, k, stride, pad in features.conv_table():
        top = prefix.split(".")[0]
        ho, wo = size[top]
        hi, wi = (h, w) if top == "conv1" else (ho, wo)             # every conv but conv1 keeps its input's size
        out.append((prefix, cin, cout, k, stride, pad, hi, wi, ho, wo))
    return out


def conv_flops(h, w):
    return sum(2 * ho * wo * cout * cin * k * k for _, cin, cout, k, _, _, _, _, ho, wo in conv_layers(h, w))


def time_layers(n, h, w, dev, reps):
    """each conv of the forward alone: median ms over reps, from device events"""
    lib = L.load()
    rows = []
    g = torch.Generator().manual_seed(1)
    for name, cin, cout, k, stride, pad, hi, wi, ho, wo in conv_layers(h, w):
        first = name == "conv1"
        x = (torch.randint(0, 256, (n, hi, wi, 3), generator=g, dtype=torch.uint8) if first else torch.randn(n, hi, wi, cin, generator=g)).to(dev)
        keep = [t.to(dev) for t in (torch.randn(cout, cin, k, k, generator=g) * 0.05, torch.ones(cout), torch.zeros(cout), torch.zeros(cout),
                                     torch.ones(cout))]
        P = L.CnnConvParams()
        for f, t in zip(("weight", "gamma", "beta", "running_mean", "running_var"), keep):
            setattr(P, f, t.data_ptr())
        packed = torch.empty(lib.vs_cnn_packed_floats(cout, cin, k), dtype=torch.float32, device=dev)
        out = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(lib.vs_cnn_pack_conv(C.byref(P), cout, cin, k, packed.data_ptr(), stream))
        kind = L.VS_CNN_INPUT_U8_NHWC if first else L.VS_CNN_INPUT_F32_NHWC

        def run():
            L.check(lib.vs_cnn_conv(x.data_ptr(), kind, n, hi, wi, cin, packed.data_ptr(), cout, k, stride, pad, out.data_ptr(), 0, cout, stream))

        run()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); run(); b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        ms = float(np.median(ts))
        flops = 2 * n * ho * wo * cout * cin * k * k
        rows.append(dict(layer=name, shape="%dx%dx%d %d->%d k%d" % (n, hi, wi, cin, cout, k), median_ms=round(ms, 4),
                         tflops=round(flops / ms / 1e9, 2), share_of_roof=round(flops / ms / 1e9 / ROOF_TFLOPS, 3)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_bench.txt"))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    dev = torch.device("cuda", 0)
    sd = features.make_state_dict(11)
    model = features.GoogLeNetFeatures()
    model.load_state_dict(sd, strict=True)
    model = model.to(dev)
    g = torch.Generator().manual_seed(2)
    frames = {n: torch.randint(0, 256, (n, 224, 224, 3), generator=g, dtype=torch.uint8).to(dev) for n in (64, 1)}
    if args.once:
        for n in (64, 1):
            model.extract(frames[n])
            model.extract(frames[n])
        torch.cuda.synchronize(dev)
        return
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    sd32 = ref.cast(sd, torch.float32, dev)

    def torch_way(n):
        with torch.no_grad():
            return ref.forward(sd32, ref.normalise(frames[n], torch.float32))

    have_torch = not args.no_torch
    if have_torch:
        try:
            for n in (1, 64):
                t = time.perf_counter()
                want = torch_way(n)
                torch.cuda.synchronize(dev)
                emit(what="torch's first forward (its library picks its convolution algorithms here)", n=n, seconds=round(time.perf_counter() - t, 1))
                got = model.extract(frames[n])
                d = ((got - want).abs().max() / want.abs().max()).item()
                emit(what="ours against torch's float32 forward on this GPU, distance / max |torch|", n=n, distance=d)
                assert d < 1e-4, d
        except Exception as e:       # the library behind torch's convolution is absent or cannot run here
            have_torch = False
            emit(what="torch's convolution cannot run on this machine: ours is reported alone", error=repr(e)[:300])
    flops = conv_flops(224, 224)
    emit(what="work", gflop_per_frame=round(flops / 1e9, 3), roof_tflops=ROOF_TFLOPS)
    for n, calls in ((64, 1), (1, 10)):
        fns = [lambda: model.extract(frames[n])] + ([lambda: torch_way(n)] if have_torch else [])
        for fn in fns:
            for _ in range(3):
                fn()
        res = alternate(fns, args.reps, dev, calls)
        for who, r in zip(("ours: GoogLeNetFeatures.extract", "torch: float32 restatement, torch ops"), res):
            tf = flops * n / r["median_ms"] / 1e9
            emit(what=who, n=n, h=224, w=224, calls_per_timing=calls, frames_per_s=round(n / r["median_ms"] * 1e3, 1), tflops=round(tf, 2),
                 share_of_fp32_mfma_roof=round(tf / ROOF_TFLOPS, 4), **r)
        if have_torch:
            emit(what="ours / torch (median time; below 1 = ours is faster)", n=n, ratio=round(res[0]["median_ms"] / res[1]["median_ms"], 3))
    rows = sorted(time_layers(64, 224, 224, dev, 10), key=lambda r: -r["median_ms"])
    total = sum(r["median_ms"] for r in rows)
    emit(what="the 57 convs of the N = 64 forward, each timed alone: sum", ms=round(total, 3))
    for r in rows[:10]:
        emit(what="costliest layers", share_of_conv_time=round(r["median_ms"] / total, 3), **r)

    # frames -> summary at T = 320
    T = 320
    video = torch.randint(0, 256, (T, 224, 224, 3), generator=g, dtype=torch.uint8).to(dev)
    scorer = pkg.SimNet(num_heads=4, d_model=256, num_layers=4, sparsity=0.0, dropout=0.3)
    scorer.load_state_dict(pkg.synth.make_state_dict(256, 4, 1234))
    scorer = scorer.to(dev).eval()
    feats = model.extract(video)

    def front():
        return model.extract(video)

    def back():
        return summary.summarize(scorer, [feats], num_seg=20, v_max=1.0)

    for _ in range(2):
        front(); back()
    a, b = alternate([front, back], max(5, args.reps // 3), dev)
    emit(what="frames -> summary, T = 320 at 224 x 224: front end (extract)", **a)
    emit(what="frames -> summary, T = 320: everything after it (summary.summarize: score + KTS + keyshot summary)", **b)
    emit(what="frames -> summary, T = 320: the front end's share of the time", share=round(a["median_ms"] / (a["median_ms"] + b["median_ms"]), 4))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
